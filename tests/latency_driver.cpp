// Test driver (CPU): the slot arithmetic of the observation ring (triton-racer-sim_amd/csrc/trsim_plan.hpp, ObsRing — the header alone) printed for
// tests/test_latency_cpu.py, which builds it with AddressSanitizer + UBSan and compares it with a deque model.
//   latency_driver ring <max_ticks> <steps> <L_0> <L_1> ...
//        "ring <slots>", then per step T = 0..steps: "step <T> <slot of step T> <slot of step T + 1>" and per env "obs <T> <env> <arrived> <slot of the observation>"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../triton-racer-sim_amd/csrc/trsim_plan.hpp"

using namespace trsim;

int main(int argc, char** argv)
{
    if (argc < 5 || std::strcmp(argv[1], "ring")) return 2;
    ObsRing R;
    R.max_ticks = std::atoi(argv[2]);
    const int steps = std::atoi(argv[3]);
    if (R.max_ticks < 1 || R.max_ticks > kMaxLatencyTicks || !R.on()) return 2;
    std::printf("ring %d\n", R.slots());
    for (long long T = 0; T <= steps; ++T) {
        std::printf("step %lld %d %d\n", T, R.slot_of_step(T), R.slot_of_step(T + 1));
        for (int a = 4; a < argc; ++a) {
            const int L = std::atoi(argv[a]);
            std::printf("obs %lld %d %d %d\n", T, a - 4, ObsRing::arrived(T, L) ? 1 : 0, R.slot_of_obs(T, L));
        }
    }
    return 0;
}
