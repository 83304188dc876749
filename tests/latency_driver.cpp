// Test driver (CPU): the slot and byte arithmetic of the observation ring (triton-racer-sim_amd/csrc/trsim_plan.hpp, ObsRing and obs_bytes — the header alone)
// printed for tests/test_latency_cpu.py, which builds it with AddressSanitizer + UBSan and compares it with a deque model and with the same sums in Python.
//   latency_driver ring <max_ticks> <steps> <L_0> <L_1> ...
//        "ring <slots>", then per step T = 0..steps: "step <T> <slot of step T> <slot of step T + 1>" and per env "obs <T> <env> <arrived> <slot of the observation>"
//   latency_driver bytes <n_envs> <H> <W> <depth> <render> <max_ticks>
//        what trs_set_latency allocates (obs_bytes), one "<name> <bytes>" per line
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../triton-racer-sim_amd/csrc/trsim_plan.hpp"

using namespace trsim;

static int bytes_mode(char** a)
{
    ObsRing R;
    R.max_ticks = std::atoi(a[5]);
    if (R.max_ticks < 1 || R.max_ticks > kMaxLatencyTicks) return 2;
    const ObsBytes b = obs_bytes(R, std::atoi(a[0]), std::atoi(a[1]), std::atoi(a[2]), std::atoi(a[4]) != 0, std::atoi(a[3]) != 0);
    const struct { const char* name; size_t v; } rows[] = {
        {"img_env", b.img_env}, {"dep_env", b.dep_env}, {"img_stride", b.img_stride}, {"dep_stride", b.dep_stride}, {"ring_img", b.ring_img},
        {"ring_dep", b.ring_dep}, {"ring_tel", b.ring_tel}, {"tel", b.tel}, {"flag", b.flag}, {"ticks", b.ticks}};
    for (const auto& r : rows) std::printf("%s %zu\n", r.name, r.v);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 8 && !std::strcmp(argv[1], "bytes")) return bytes_mode(argv + 2);
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
