// Test driver (CPU): the product's refusal policy and LDS fit arithmetic (triton-racer-sim_amd/csrc/trsim_plan.hpp, the header alone) printed for
// tests/test_host_tables.py, which builds it with AddressSanitizer + UBSan.
//   plan_driver policy                         every built variant as the handle's state x every feature bit a caller can add
//   plan_driver fit <H> <W> <lds_step>...      every built variant x 1..64 envs per workgroup beside each lds_step
//   plan_driver slices <n_envs>                the controls of a step call (Controls) after k = 0..16 steps: strides 0 and n_envs x brk / reset given or not, and the
//                                              synthetic call; then the same for after(a).after(b), a, b = 0..8.  Offsets in floats from each array's base, -1 = null
//   plan_driver fetch                          fetch_layout / fetch_reserve for every subset of the eight items, n_envs in {1, 5, 70}, with and without a 64x64 frame
//   plan_driver lds <W> <lds_step> <epw> <n_phys>   for H = 2..600 and every built variant: every region offset of step_lds_layout and worker_lds_layout, where the
//                                              lit palettes and the worker's hand-off slots begin, and for each of the hill_batch(H) row tables of a HILLS
//                                              variant the offsets of its three planes (in the step kernel's layout and in the worker's) and its end
//   plan_driver geometry <H> <W>               rows per pass, idle raster threads, passes and the last pass's rows, hill_batch, light_copies, the dynamic filter's window
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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
    if (argc >= 6 && !std::strcmp(argv[1], "lds")) {
        const int W = std::atoi(argv[2]), lds_step = std::atoi(argv[3]), epw = std::atoi(argv[4]), n_phys = std::atoi(argv[5]);
        for (int H = 2; H <= 600; ++H)
            for (Variant v = 0; v < kVariants; ++v) {
                if (!variant_built(v)) continue;
                const bool hilly = (v & kVHills) != 0, dyn = (v & kVDyn) != 0;
                const StepLds S = step_lds_layout(lds_step, epw, H, W, v, n_phys);
                const WorkerLds K = worker_lds_layout(lds_step, epw, H, W, v);
                std::printf("step %d %u %d %d %d %d %d %d %d %d\n", H, v, S.cam, S.prog, S.pitch, S.hill, S.light, S.light + epw * 32, S.dyn, S.total);
                std::printf("worker %d %u %d %d %d %d %d %d %d\n", H, v, K.ctl, K.ctl + (int)wlds_slot_off(epw), K.dyn, K.hill, K.light, K.light + kCamDepth * epw * 32, K.total);
                std::printf("sizes %d %u %d %d %d %d\n", H, v, tabs_lds_bytes(H, v), light_lds_extra(H, W, epw, hilly, dyn), light_lds_extra(H, W, kCamDepth * epw, hilly, dyn), dyn_lds_bytes(H));
                if (!hilly) continue;
                for (int k = 0; k < hill_batch(H); ++k)
                    for (const int base : {S.hill, K.hill}) {
                        const int tab = base + k * hill_table_bytes(H);
                        std::printf("table %d %u %d %s %d %d %d %d\n", H, v, k, base == S.hill ? "step" : "worker", tab, tab + hill_table_pal_off(H), tab + hill_table_depth_off(H),
                                    tab + hill_table_bytes(H));
                    }
                std::printf("hbar %d %u %d %d %d\n", H, v, hill_batch(H), S.hill + hill_batch(H) * hill_table_bytes(H), K.hill + hill_batch(H) * hill_table_bytes(H));
            }
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "geometry")) {
        const int H = std::atoi(argv[2]), W = std::atoi(argv[3]), gpr = W / 4, rpp = raster_rows_per_pass(gpr);
        std::printf("geometry %d %d %d %d %d %d %d %d %d %d %d\n", H, W, gpr, rpp, kRasterThreads - rpp * gpr, (H + rpp - 1) / rpp, H - ((H - 1) / rpp) * rpp, hill_batch(H),
                    light_copies(gpr), dyn_window_lo(H), dyn_window_hi(H));
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "slices")) {
        const int n = std::atoi(argv[2]);
        std::vector<float> st((size_t)17 * n), th(st.size()), br(st.size());
        std::vector<uint8_t> rs((size_t)n);
        auto off = [](const float* p, const std::vector<float>& base) { return p ? (long)(p - base.data()) : -1l; };
        auto show = [&](const char* tag, const Controls& c, int a, int b, const Controls& r) {
            std::printf("%s %d %d %d %d %d %d %ld %ld %ld %d %d %d\n", tag, c.stride, c.brk ? 1 : 0, c.reset ? 1 : 0, c.synth, a, b, off(r.steer, st), off(r.thr, th), off(r.brk, br),
                        r.reset ? (r.reset == rs.data() ? 1 : -1) : 0, r.synth, r.stride);
        };
        std::vector<Controls> calls;
        for (const int stride : {0, n})
            for (int m = 0; m < 4; ++m) calls.push_back(Controls{st.data(), th.data(), (m & 1) ? br.data() : nullptr, (m & 2) ? rs.data() : nullptr, 0, stride});
        for (const int stride : {0, n}) calls.push_back(Controls{nullptr, nullptr, nullptr, nullptr, 1, stride});
        for (const Controls& c : calls) {
            for (int k = 0; k <= 16; ++k) show("slice", c, k, 0, c.after(k));
            for (int a = 0; a <= 8; ++a)
                for (int b = 0; b <= 8; ++b) show("compose", c, a, b, c.after(a).after(b));
        }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "fetch")) {
        for (const size_t n : {(size_t)1, (size_t)5, (size_t)70})
            for (const size_t img : {(size_t)0, (size_t)64 * 64 * 3 * n})
                for (unsigned mask = 0; mask < (1u << kFetchItems); ++mask) {
                    size_t bytes[kFetchItems];
                    for (int i = 0; i < kFetchItems; ++i) bytes[i] = ((mask >> i) & 1u) ? (i == 0 ? img : (i == kFetchItems - 1 ? n : n * 4)) : 0;
                    const FetchLayout L = fetch_layout(bytes);
                    std::printf("fetch %zu %zu %u %zu %zu", n, img, mask, fetch_reserve(bytes[0], n), L.end);
                    for (int i = 0; i < kFetchItems; ++i) std::printf(" %zu:%zu", L.off[i], bytes[i]);
                    std::printf("\n");
                }
        return 0;
    }
    return 2;
}
