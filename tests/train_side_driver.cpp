// train_side_driver.cpp — the 28-array session's host-only rules of csrc/trsim_train.hpp on the CPU, built by tests/test_train_side_cpu.py with
// -fsanitize=address,undefined: where the 14 trained arrays lie (TrainSideLayout), the sizes of the side debug items, the train mask's rule with the
// branch's bits and the refusals of the array count, printed for the test to compare with its restatement.
//   train_side_driver layout <F>      the fifteen offsets, where W1Y begins, then the nine offsets of the 22-array kernels' view (tail())
//   train_side_driver debug <n>       the floats of side items 0 .. 31, then of the unknown items 32 and -1
//   train_side_driver config          "ok" when every mask rule holds
//   train_side_driver count           one line per (pilot arrays, n_arrays): "ok", "arg" or "limit"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "triton-racer-sim_amd/csrc/trsim_train.hpp"

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "layout" && argc == 3) {
        const trsim::TrainSideLayout L = trsim::TrainSideLayout::of((size_t)std::strtoull(argv[2], nullptr, 0));
        for (int a = 0; a <= trsim::kTrainSideArrays; ++a) std::printf("%zu\n", L.off[a]);
        std::printf("%zu\n", L.w1y());
        const trsim::TrainLayout T = L.tail();
        for (int a = 0; a <= trsim::kTrainArrays; ++a) std::printf("%zu\n", T.off[a]);
        return 0;
    }
    if (cmd == "debug" && argc == 3) {
        const int n = std::atoi(argv[2]);
        for (int w = 0; w <= 32; ++w) std::printf("%zu\n", trsim::train_side_debug_floats(w, n));
        std::printf("%zu\n%zu\n%d\n", trsim::train_side_debug_floats(-1, n), trsim::side_frame_floats(), trsim::kSideValues);
        return 0;
    }
    if (cmd == "config") {
        trs_train_config d; trsim::train_defaults(&d);
        auto with = [&](uint32_t mask) { trs_train_config c = d; c.train_mask = mask; return c; };
        struct Case { uint32_t mask; int n_arrays; bool fine; } cases[] = {
            {0xFu, 8, true}, {0xFu, 14, true}, {0x7Fu, 14, true}, {0x20u, 14, true}, {0x41u, 14, true}, {0x8u, 14, true},
            {0x7Fu, 8, false}, {0x10u, 8, false}, {0x80u, 14, false}, {0xFFu, 14, false}, {0x0u, 14, false}, {0x0u, 8, false}, {0x100u, 14, false}};
        for (const Case& k : cases) {
            const trs_train_config c = with(k.mask);
            const char* why = trsim::train_config_error_ex(&c, k.n_arrays);
            if ((why == nullptr) != k.fine || (why && !std::strstr(why, "train_mask"))) { std::printf("mask %#x with %d arrays: %s\n", k.mask, k.n_arrays, why ? why : "accepted"); return 0; }
        }
        trs_train_config bad = with(0x20u); bad.lr = 0.0f;                      // the other fields by the one rule, whatever the mask
        const char* why = trsim::train_config_error_ex(&bad, 14);
        if (!why || !std::strstr(why, "lr")) { std::puts("lr = 0 accepted under a side mask"); return 0; }
        bad = with(0x20u); bad.struct_size = 8;
        why = trsim::train_config_error_ex(&bad, 14);
        if (!why || !std::strstr(why, "struct_size")) { std::puts("struct_size accepted under a side mask"); return 0; }
        if (!trsim::train_config_error_ex(nullptr, 14)) { std::puts("NULL accepted"); return 0; }
        if (trsim::kTrainMaskAllSide != 0x7Fu || trsim::train_mask_bit(0) != 0 || trsim::train_mask_bit(7) != 3 || trsim::train_mask_bit(8) != 4 || trsim::train_mask_bit(13) != 6) {
            std::puts("mask bits"); return 0;
        }
        std::puts("ok");
        return 0;
    }
    if (cmd == "count") {
        for (int pilot : {22, 28, 42})
            for (int n : {8, 14, 0, 7, 22, 28}) {
                bool limit = false;
                const char* why = trsim::train_count_error(pilot, n, &limit);
                std::printf("%d %d %s\n", pilot, n, !why ? "ok" : (limit ? "limit" : "arg"));
            }
        return 0;
    }
    return 2;
}
