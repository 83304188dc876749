// Test driver (CPU): the host side of the scripted expert (triton-racer-sim_amd/csrc/trsim_expert.hpp — the header alone) printed for
// tests/test_expert_cpu.py, which builds it with AddressSanitizer + UBSan and compares it with Python statements of the rules.
//   expert_driver config <look> <n_points> <struct_size delta> <nan field: 0 | 1>     "ok" or the refusal's text
//   expert_driver capture <every> <skip> <capacity> <struct_size delta> <rows: 0 | 1> <frames: 0 | 1> <render: 0 | 1>     "ok" or the refusal's text
//   expert_driver defaults                                                            the default config, one "name value" per line
//   expert_driver yaw <file of float32 [n][2] tangents>                               per point the bit pattern of track_yaw as 8 hex digits
//   expert_driver plan <every> <skip> <capacity> <first tick with a frame> <n_0> <n_1> ...
//        calls of n_0, n_1, ... ticks with the tick counter carried from call to call and a new plan per call: "call <c> tick <k> slot <s>" per tick
//        (s = -1: not captured) and "call <c> used <slots>" behind each call
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_expert.hpp"

using namespace trsim;

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "config") && argc == 6) {
        trs_expert_config c;
        expert_defaults(&c);
        c.look = std::atoi(argv[2]);
        c.struct_size += (uint32_t)std::atoi(argv[4]);
        if (std::atoi(argv[5])) c.k_head = std::numeric_limits<float>::quiet_NaN();
        const char* why = expert_config_error(&c, std::atoi(argv[3]));
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (!std::strcmp(argv[1], "capture") && argc == 9) {
        static float rows[8];
        static uint8_t frames[8];
        trs_expert_capture c{};
        c.struct_size = (uint32_t)sizeof c + (uint32_t)std::atoi(argv[5]);
        c.every = std::atoi(argv[2]); c.skip = std::atoi(argv[3]); c.capacity = std::atoi(argv[4]);
        c.d_rows = std::atoi(argv[6]) ? rows : nullptr;
        c.d_frames_or_null = std::atoi(argv[7]) ? frames : nullptr;
        const char* why = expert_capture_error(&c, std::atoi(argv[8]) != 0);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (!std::strcmp(argv[1], "defaults")) {
        trs_expert_config c;
        expert_defaults(&c);
        std::printf("struct_size %u\nlook %d\nk_cte %.9g\nk_head %.9g\nthr_hi %.9g\nthr_lo %.9g\ntarget_speed %.9g\nbrake_over %.9g\nbrake_val %.9g\nalpha %.9g\nsigma %.9g\nseed %llu\n",
                    c.struct_size, c.look, c.k_cte, c.k_head, c.thr_hi, c.thr_lo, c.target_speed, c.brake_over, c.brake_val, c.alpha, c.sigma, (unsigned long long)c.seed);
        return 0;
    }
    if (!std::strcmp(argv[1], "yaw") && argc == 3) {
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) return 2;
        std::vector<float> tan;
        float pair[2];
        while (std::fread(pair, sizeof pair, 1, f) == 1) { tan.push_back(pair[0]); tan.push_back(pair[1]); }
        std::fclose(f);
        const int n = (int)(tan.size() / 2);
        std::vector<float> yaw((size_t)n);
        build_track_yaw(tan.data(), n, yaw.data());
        for (int p = 0; p < n; ++p) {
            uint32_t bits;
            std::memcpy(&bits, &yaw[(size_t)p], 4);
            std::printf("%08x\n", bits);
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "plan") && argc >= 7) {
        trs_expert_capture c{};
        c.struct_size = sizeof c;
        static float rows[8];
        c.every = std::atoi(argv[2]); c.skip = std::atoi(argv[3]); c.capacity = std::atoi(argv[4]); c.d_rows = rows;
        if (expert_capture_error(&c, true)) return 2;
        const uint32_t first_frame = (uint32_t)std::atoi(argv[5]);
        uint32_t k = 0;
        for (int a = 6; a < argc; ++a) {
            CapturePlan plan = CapturePlan::of(&c);
            for (int t = 0; t < std::atoi(argv[a]); ++t, ++k) std::printf("call %d tick %u slot %d\n", a - 6, k, plan.slot_for(k, k >= first_frame));
            std::printf("call %d used %d\n", a - 6, plan.used);
        }
        return 0;
    }
    return 2;
}
