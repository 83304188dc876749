// Test driver (CPU): the owner of "which frame buffer holds the uniform rows" and the store-count arithmetic of the resident worker's lagged arrivals
// (triton-racer-sim_amd/csrc/trsim_plan.hpp, the header alone) printed for tests/test_uniform_rows_cpu.py, which builds it with AddressSanitizer + UBSan.
//   uniform_rows_driver flags <event>...                          the state after each event: "state <event> <ok0> <ok1> <mask of the variant last named>"
//        events: invalidate | variant:<v> | render:<first>:<n> (launch_step: mask, then rendered) | worker:<start>:<consumed> (worker_launch ... its normal exit)
//   uniform_rows_driver counts <H> <W> <uni_rows> <epw> <depth>   a raster wave's program order replayed for every wave, ragged workgroup, mask, start parity and
//        queue pattern: "counts <wave> <n_loc> <mask> <start&1> <pattern> <lag> <nstep> <nuni> <waits> <worst count - issued> <steps whose stores differ from worker_step_stores>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_plan.hpp"

using namespace trsim;
using u64 = unsigned long long;

namespace {

// what the wave's 64 threads walk (raster_thread, trsim_device.hpp): thread tid owns column group tid % gpr and the rows r0, r0 + rows_per_pass, ...; the first
// uni_rows of them are uniform rows.  A wave instruction is issued when any lane has a row: the maximum over the lanes, twice with a depth frame.
void wave_rows(int H, int W, int uni_rows, int wave, bool depth, int& nu, int& ng)
{
    const int gpr = W / 4, rpp = kRasterThreads / gpr;
    nu = ng = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const int r0 = (wave * 64 + lane) / gpr, vstart = r0 < rpp ? r0 : H;
        int u = 0, g = 0;
        for (int v = vstart; v < H; v += rpp) (v < uni_rows ? u : g)++;
        nu = std::max(nu, u); ng = std::max(ng, g);
    }
    if (depth) { nu *= 2; ng *= 2; }
}

// posts queued behind step s when the wave begins it (`ahead` in trs_worker_kernel): 0 = a lock-step consumer, 7 = the ring is full, 2 = alternating, 3 = a pseudo-random walk
int ahead_of(int pattern, u64 s)
{
    switch (pattern) {
    case 0: return 0;
    case 1: return 7;
    case 2: return (s & 1) ? 0 : 2;
    default: return (int)(((s * 2654435761ull) >> 7) % 5);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "flags")) {
        UniformRows U;
        Variant v = 0;
        for (int a = 2; a < argc; ++a) {
            const std::string ev = argv[a];
            unsigned long long x = 0, y = 0;
            if (ev == "invalidate") U.invalidate();
            else if (std::sscanf(ev.c_str(), "variant:%llu", &x) == 1) v = (Variant)x;
            else if (std::sscanf(ev.c_str(), "render:%llu:%llu", &x, &y) == 2) { (void)U.skip_mask(v); U.rendered(v, x, y); }
            else if (std::sscanf(ev.c_str(), "worker:%llu:%llu", &x, &y) == 2) { if (y > x) U.rendered(v, x, y - x); }
            else return 2;
            std::printf("state %s %d %d %u\n", ev.c_str(), U.ok[0] ? 1 : 0, U.ok[1] ? 1 : 0, U.skip_mask(v));
        }
        return 0;
    }
    if (argc == 7 && !std::strcmp(argv[1], "counts")) {
        const int H = std::atoi(argv[2]), W = std::atoi(argv[3]), uni_rows = std::atoi(argv[4]), epw = std::atoi(argv[5]);
        const bool depth = std::atoi(argv[6]) != 0;
        const int waves = kRasterThreads / 64, steps = 40;
        for (int wave = 0; wave < waves; ++wave)
            for (int n_loc = 1; n_loc <= epw; ++n_loc)
                for (unsigned mask = 0; mask < 4; ++mask)
                    for (u64 start : {1000ull, 1001ull})
                        for (int pattern = 0; pattern < 4; ++pattern) {
                            int nu, ng, own = 0;
                            wave_rows(H, W, uni_rows, wave, depth, nu, ng);
                            for (int j = wave; j < n_loc; j += waves) ++own;
                            const int nuni = nu * n_loc, nstep = (nu + ng) * n_loc + 2 * own;
                            const int lag = worker_lag(nstep, nuni, true);
                            // the plain path of trs_worker_kernel in program order: `total` store instructions issued so far, end[k] after step start + k
                            long long total = 0, worst = -(1ll << 40);
                            int waits = 0, wrong = 0;
                            std::vector<long long> end;
                            u64 owed = start;
                            for (u64 s = start; s < start + steps; ++s) {
                                const int ahead = ahead_of(pattern, s);
                                if (owed < s && ahead == 0 && pattern == 3) owed = s;          // nothing posted yet when the wave came round: it drained and arrived for everything
                                const u64 keep = std::min<u64>((u64)ahead + 1, (u64)lag);
                                const bool skipu = worker_skips_uniform(mask, start, s);
                                const bool sweep = ahead == 0 && !skipu;
                                const long long before = total;
                                if (sweep) total += nuni;
                                for (int j = 0; j < n_loc; ++j) {
                                    if (!sweep && !skipu) total += nu;
                                    if (j == 0)
                                        while (s - owed >= keep) {
                                            const int cnt = worker_wait_count(mask, start, owed, s, nstep, nuni, skipu ? 0 : (sweep ? nuni : nu));
                                            const long long issued = total - end[(size_t)(owed - start)];
                                            worst = std::max(worst, (long long)cnt - issued);
                                            ++waits; ++owed;
                                        }
                                    total += ng;
                                    if (j % waves == wave) total += 2;
                                }
                                end.push_back(total);
                                if (total - before != worker_step_stores(nstep, nuni, skipu)) ++wrong;
                            }
                            std::printf("counts %d %d %u %d %d %d %d %d %d %lld %d\n", wave, n_loc, mask, (int)(start & 1), pattern, lag, nstep, nuni, waits, worst, wrong);
                        }
        return 0;
    }
    return 2;
}
