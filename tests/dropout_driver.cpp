// dropout_driver.cpp — csrc/trsim_dropout.hpp on the CPU, built by tests/test_dropout_cpu.py with -fsanitize=address,undefined: the host-only rules of
// dropout behind conv7 (the defaults and refusals of trs_dropout_config, the threshold T and the scale s of a rate, the key chain and keep()) printed for
// the test to compare with its numpy restatement.
//   dropout_driver defaults                                      struct_size, the rate's bit pattern, sites, seed
//   dropout_driver config                                        "ok" when the defaults pass and every bad field is refused with a text that names it
//   dropout_driver ts <rate bits>...                             T and the bit pattern of s per rate (given as a hex bit pattern)
//   dropout_driver keep <rate bits> <seed> <t> <site> <n> <width>   one line of width characters 0 / 1 per frame slot
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "triton-racer-sim_amd/csrc/trsim_dropout.hpp"

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(const char* s) { const unsigned u = (unsigned)std::strtoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "defaults") {
        trs_dropout_config c; trsim::dropout_defaults(&c);
        std::printf("%u\n%08x\n%u\n%llu\n", c.struct_size, bits(c.rate), c.sites, (unsigned long long)c.seed);
        return 0;
    }
    if (cmd == "config") {
        trs_dropout_config d; trsim::dropout_defaults(&d);
        if (trsim::dropout_config_error(&d) || d.struct_size != sizeof d) { std::puts("defaults refused"); return 0; }
        if (!trsim::dropout_config_error(nullptr)) { std::puts("NULL accepted"); return 0; }
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        struct Case { const char* field; trs_dropout_config c; } cases[16];
        int k = 0;
        auto bad = [&](const char* field, auto set) { cases[k].field = field; cases[k].c = d; set(cases[k].c); ++k; };
        bad("struct_size", [](trs_dropout_config& c) { c.struct_size = 8; });
        bad("struct_size", [](trs_dropout_config& c) { c.struct_size = 0; });
        bad("rate", [](trs_dropout_config& c) { c.rate = 1.0f; });
        bad("rate", [](trs_dropout_config& c) { c.rate = -0.1f; });
        bad("rate", [](trs_dropout_config& c) { c.rate = 1.5f; });
        bad("rate", [&](trs_dropout_config& c) { c.rate = nan; });
        bad("rate", [&](trs_dropout_config& c) { c.rate = inf; });
        bad("sites", [](trs_dropout_config& c) { c.sites = 0x10; });
        bad("sites", [](trs_dropout_config& c) { c.sites = 0x8000000F; });
        for (int i = 0; i < k; ++i) {
            const char* why = trsim::dropout_config_error(&cases[i].c);
            if (!why || !std::strstr(why, cases[i].field)) { std::printf("case %d (%s): %s\n", i, cases[i].field, why ? why : "accepted"); return 0; }
        }
        trs_dropout_config ok = d; ok.rate = 0.0f; ok.sites = 0; ok.seed = ~0ull;
        if (trsim::dropout_config_error(&ok)) { std::puts("a valid config refused"); return 0; }
        ok.rate = -0.0f;                                       // -0 is 0: inside [0, 1)
        if (trsim::dropout_config_error(&ok) || trsim::dropout_threshold(ok.rate) != 0) { std::puts("-0 refused"); return 0; }
        unsigned char one = 7;
        const char* checks[] = {trsim::dropout_keep_error(0, 0, 1, 1, &one), trsim::dropout_keep_error(1, 4, 1, 1, &one), trsim::dropout_keep_error(1, -1, 1, 1, &one),
                                trsim::dropout_keep_error(1, 0, -1, 1, &one), trsim::dropout_keep_error(1, 0, 1, -1, &one), trsim::dropout_keep_error(1, 0, 1, 1, nullptr)};
        for (const char* why : checks)
            if (!why) { std::puts("a bad keep call accepted"); return 0; }
        if (trsim::dropout_keep_error(1, 3, 0, 0, nullptr) || trsim::dropout_keep_error(1, 0, 2, 3, &one)) { std::puts("a valid keep call refused"); return 0; }
        std::puts("ok");
        return 0;
    }
    if (cmd == "ts") {
        for (int i = 2; i < argc; ++i) {
            const unsigned T = trsim::dropout_threshold(from_bits(argv[i]));
            std::printf("%u %08x\n", T, bits(trsim::dropout_scale(T)));
        }
        return 0;
    }
    if (cmd == "keep" && argc == 8) {
        trs_dropout_config c; trsim::dropout_defaults(&c);
        c.rate = from_bits(argv[2]); c.seed = std::strtoull(argv[3], nullptr, 0);
        const long long t = std::strtoll(argv[4], nullptr, 0);
        const int site = std::atoi(argv[5]), n = std::atoi(argv[6]); const long long width = std::strtoll(argv[7], nullptr, 0);
        if (trsim::dropout_config_error(&c)) return 3;
        std::vector<unsigned char> keep((size_t)n * (size_t)width);             // exactly n x width: a write past it is the sanitizer's to find
        if (trsim::dropout_keep_error(t, site, n, width, keep.data())) return 3;
        trsim::dropout_keep_host(c, t, site, n, width, keep.data());
        std::string line((size_t)width, '0');
        for (int i = 0; i < n; ++i) {
            for (long long k = 0; k < width; ++k) line[(size_t)k] = keep[(size_t)i * (size_t)width + (size_t)k] ? '1' : '0';
            std::puts(line.c_str());
        }
        return 0;
    }
    return 2;
}
