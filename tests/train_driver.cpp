// train_driver.cpp — csrc/trsim_train.hpp on the CPU, built by tests/test_train_cpu.py with -fsanitize=address,undefined: the host-only rules of training
// the pilot's tail (the scale's exponent from a bit pattern, alpha_t and the two constants 1 - beta, 2^e, the layout of the master / m / v / gradient
// buffers, the sizes of the debug items, the config's refusals) printed for the test to compare with its numpy restatement.
//   train_driver exp <bits>...        the exponent s per bit pattern (decimal or 0x...)
//   train_driver alpha <t>...         alpha_t per t under the default config as hex bit patterns, then 1 - beta1 and 1 - beta2
//   train_driver pow2 <e>...          2^e as hex bit patterns
//   train_driver layout <F>           the nine offsets
//   train_driver debug <n> <F>        the floats of items 0 .. 34, then of the unknown items 35 and -1
//   train_driver config               "ok" when the defaults pass and every bad field is refused with a text that names it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "triton-racer-sim_amd/csrc/trsim_train.hpp"

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "exp") {
        for (int i = 2; i < argc; ++i) std::printf("%d\n", trsim::train_scale_exponent((uint32_t)std::strtoull(argv[i], nullptr, 0)));
        return 0;
    }
    if (cmd == "alpha") {
        trs_train_config c; trsim::train_defaults(&c);
        for (int i = 2; i < argc; ++i) std::printf("%08x\n", bits(trsim::train_alpha(c, std::strtoll(argv[i], nullptr, 0))));
        std::printf("%08x\n%08x\n", bits(trsim::train_one_minus(c.beta1)), bits(trsim::train_one_minus(c.beta2)));
        return 0;
    }
    if (cmd == "pow2") {
        for (int i = 2; i < argc; ++i) std::printf("%08x\n", bits(trsim::train_pow2(std::atoi(argv[i]))));
        return 0;
    }
    if (cmd == "layout" && argc == 3) {
        const trsim::TrainLayout L = trsim::TrainLayout::of((size_t)std::strtoull(argv[2], nullptr, 0));
        for (int a = 0; a <= trsim::kTrainArrays; ++a) std::printf("%zu\n", L.off[a]);
        return 0;
    }
    if (cmd == "debug" && argc == 4) {
        const int n = std::atoi(argv[2]); const size_t F = (size_t)std::strtoull(argv[3], nullptr, 0);
        for (int w = 0; w <= 35; ++w) std::printf("%zu\n", trsim::train_debug_floats(w, n, F));
        std::printf("%zu\n", trsim::train_debug_floats(-1, n, F));
        return 0;
    }
    if (cmd == "config") {
        trs_train_config d; trsim::train_defaults(&d);
        if (trsim::train_config_error(&d) || d.struct_size != sizeof d || d.train_mask != 0xFu) { std::puts("defaults refused"); return 0; }
        if (!trsim::train_config_error(nullptr)) { std::puts("NULL accepted"); return 0; }
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        struct Case { const char* field; trs_train_config c; } cases[16];
        int k = 0;
        auto bad = [&](const char* field, auto set) { cases[k].field = field; cases[k].c = d; set(cases[k].c); ++k; };
        bad("struct_size", [](trs_train_config& c) { c.struct_size = 8; });
        bad("lr", [](trs_train_config& c) { c.lr = 0.0f; });
        bad("lr", [&](trs_train_config& c) { c.lr = nan; });
        bad("lr", [&](trs_train_config& c) { c.lr = inf; });
        bad("lr", [](trs_train_config& c) { c.lr = -1e-3f; });
        bad("beta1", [](trs_train_config& c) { c.beta1 = 1.0f; });
        bad("beta1", [&](trs_train_config& c) { c.beta1 = nan; });
        bad("beta2", [](trs_train_config& c) { c.beta2 = -0.5f; });
        bad("beta2", [](trs_train_config& c) { c.beta2 = 1.5f; });
        bad("eps", [](trs_train_config& c) { c.eps = 0.0f; });
        bad("eps", [&](trs_train_config& c) { c.eps = nan; });
        bad("train_mask", [](trs_train_config& c) { c.train_mask = 0; });
        bad("train_mask", [](trs_train_config& c) { c.train_mask = 0x1F; });
        for (int i = 0; i < k; ++i) {
            const char* why = trsim::train_config_error(&cases[i].c);
            if (!why || !std::strstr(why, cases[i].field)) { std::printf("case %d (%s): %s\n", i, cases[i].field, why ? why : "accepted"); return 0; }
        }
        trs_train_config ok = d; ok.beta1 = 0.0f; ok.beta2 = 0.0f; ok.train_mask = 0x8;
        if (trsim::train_config_error(&ok)) { std::puts("a valid config refused"); return 0; }
        std::puts("ok");
        return 0;
    }
    return 2;
}
