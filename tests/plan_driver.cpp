// Test driver (CPU): the product's refusal policy and LDS fit arithmetic (triton-racer-sim_amd/csrc/trsim_plan.hpp, the header alone) printed for
// tests/test_host_tables.py, which builds it with AddressSanitizer + UBSan.
//   plan_driver policy                         every built variant as the handle's state x every feature bit a caller can add
//   plan_driver fit <H> <W> <lds_step>...      every built variant x 1..64 envs per workgroup beside each lds_step
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../triton-racer-sim_amd/csrc/trsim_plan.hpp"

using namespace trsim;

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "policy")) {
        for (Variant state = 0; state < kVariants; ++state) {
            if (!variant_built(state)) continue;
            for (const Variant add : {kVDyn, kVHills, kVLens, kVLight}) {
                const Variant set = variant_clash(state, add);
                std::printf("clash %u %u %d %u %d %s\n", state, add, variant_built(state | add) ? 1 : 0, set, set ? (variant_built(add | set) ? 1 : 0) : -1,
                            variant_refusal(add, set));
            }
        }
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "fit")) {
        const int H = std::atoi(argv[2]), W = std::atoi(argv[3]);
        for (int a = 4; a < argc; ++a) {
            const int lds_step = std::atoi(argv[a]);
            for (Variant v = 0; v < kVariants; ++v) {
                if (!variant_built(v)) continue;
                for (int epw = 1; epw <= 64; ++epw)
                    std::printf("fit %d %u %d %d %d %d %d %d\n", lds_step, v, epw, step_lds_layout(lds_step, epw, H, W, v, 1).total, steps_that_fit(lds_step, epw, H, W, v),
                                worker_lds_layout(lds_step, epw, H, W, v).total, (int)lds_fit(lds_step, epw, H, W, v, false), (int)lds_fit(lds_step, epw, H, W, v, true));
            }
        }
        return 0;
    }
    return 2;
}
