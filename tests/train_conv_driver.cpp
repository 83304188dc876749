// train_conv_driver.cpp — csrc/trsim_train_conv.hpp on the CPU, built by tests/test_train_conv_cpu.py with -fsanitize=address,undefined: the host-only
// rules of training the pilot's last convolutions printed for the test to compare with its numpy restatement.
//   train_conv_driver mask                           "ok" when every bad (mask, arrays) is refused and the good ones pass; the lowest trained layer
//   train_conv_driver layout                         the nine offsets of the master / m / v / gradient buffers
//   train_conv_driver pack <j>                       pack_layer (trsim_pilot_plan.hpp) on a kernel whose values carry their own number: "ok <count>" when every
//                                                    K[kh][kw][ci][co] lies at train_conv_packed_index and the index is a bijection onto the pack
//   train_conv_driver index <j> <kh kw ci co>...     the packed index of each quadruple
//   train_conv_driver split <j> <ih> <iw> <n> <cu>   P, chunks, chunks per slice, slices, then first and end of every slice
//   train_conv_driver sizes <ih3> <iw3> <n_cap> <cu> <lowest>   the gradient buffer's floats, the four delta buffers' values, the partial sums' floats
//   train_conv_driver fits <ih3> <iw3> <n_cap> <cu> <lowest>    "ok <most floats any n needs>" when for every n in 1 .. n_cap and every layer from `lowest` up the
//                                                    partial sums of the split at n, slices(n) (kernel + COUT), fit train_conv_sizes(n_cap).part_floats, and delta and G fit theirs
//   train_conv_driver debug <j> <ih> <iw> <n>        the floats of items 0 .. 8, then of the unknown items 9 and -1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "triton-racer-sim_amd/csrc/trsim_pilot_plan.hpp"
#include "triton-racer-sim_amd/csrc/trsim_train_conv.hpp"

using namespace trsim;

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "mask") {
        const float x = 0.0f;
        const float* all[8] = {&x, &x, &x, &x, &x, &x, &x, &x};
        const float* only7[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &x, &x};
        const float* no_bias5[8] = {&x, &x, &x, nullptr, &x, &x, &x, &x};
        if (train_conv_mask_error(0xF, all) || train_conv_mask_error(0x8, only7) || train_conv_mask_error(0x5, no_bias5)) { std::puts("a valid mask refused"); return 0; }
        if (!train_conv_mask_error(0, all) || !train_conv_mask_error(0x10, all) || !train_conv_mask_error(0x1F, all) || !train_conv_mask_error(0x80000000u, all)) { std::puts("a bad mask accepted"); return 0; }
        if (!train_conv_mask_error(0xF, nullptr) || !train_conv_mask_error(0xF, only7) || !train_conv_mask_error(0x2, no_bias5) || !train_conv_mask_error(0x1, only7)) { std::puts("a NULL array accepted"); return 0; }
        if (train_conv_lowest(0xF) != 0 || train_conv_lowest(0x8) != 3 || train_conv_lowest(0xA) != 1 || train_conv_lowest(0x4) != 2) { std::puts("lowest layer wrong"); return 0; }
        std::puts("ok");
        return 0;
    }
    if (cmd == "layout") {
        const ConvTrainLayout L = ConvTrainLayout::of();
        for (int a = 0; a <= kConvTrainArrays; ++a) std::printf("%zu\n", L.off[a]);
        return 0;
    }
    if (cmd == "pack" && argc == 3) {
        const int j = std::atoi(argv[2]);
        const PilotLayer l = pilot_layer_geometry(3 + j, 12 - 2 * j, 17 - 2 * j);
        const ConvGeom g = train_conv_geom(j, l.IH, l.IW);
        if (g.CIN != l.CIN || g.COUT != l.COUT || g.OH != l.OH || g.OW != l.OW || l.run_pad != l.run || l.COUT_PAD != l.COUT) { std::puts("geometry differs"); return 0; }
        // value number e cannot be one binary16 for 147,456 values: two passes carry e % 2048 and e / 2048, both exact in binary16, so a value that is found
        // at its index in both passes is the value number e and no other
        std::vector<float> K(g.kernel_count()), B(g.COUT, 0.0f);
        for (int pass = 0; pass < 2; ++pass) {
            for (size_t e = 0; e < K.size(); ++e) K[e] = pass == 0 ? (float)(e % 2048) : (float)(e / 2048);
            const PackedLayer p = pack_layer(l, K.data(), B.data());
            if (p.w.size() != K.size()) { std::printf("pack holds %zu values\n", p.w.size()); return 0; }
            std::vector<char> hit(K.size(), 0);
            for (int kh = 0; kh < 3; ++kh)
                for (int kw = 0; kw < 3; ++kw)
                    for (int ci = 0; ci < g.CIN; ++ci)
                        for (int co = 0; co < g.COUT; ++co) {
                            const size_t at = train_conv_packed_index(g, kh, kw, ci, co);
                            if (at >= p.w.size() || hit[at]) { std::printf("index %zu out of range or hit twice\n", at); return 0; }
                            hit[at] = 1;
                            if (p.w[at] != host_f2h(K[((size_t)(kh * 3 + kw) * g.CIN + ci) * g.COUT + co])) { std::printf("K[%d][%d][%d][%d] is not at %zu\n", kh, kw, ci, co, at); return 0; }
                        }
        }
        std::printf("ok %zu\n", K.size());
        return 0;
    }
    if (cmd == "index" && argc >= 3 && (argc - 3) % 4 == 0) {
        const ConvGeom g = train_conv_geom(std::atoi(argv[2]), 5, 5);
        for (int i = 3; i < argc; i += 4) std::printf("%zu\n", train_conv_packed_index(g, std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3])));
        return 0;
    }
    if (cmd == "split" && argc == 7) {
        const ConvGeom g = train_conv_geom(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
        const ConvSplit s = train_conv_split(g, std::atoi(argv[5]), std::atoi(argv[6]));
        std::printf("%ld %d %d %d\n", s.P, s.chunks, s.per_slice, s.slices);
        for (int i = 0; i < s.slices; ++i) std::printf("%ld %ld\n", s.first(i), s.end(i));
        return 0;
    }
    if (cmd == "sizes" && argc == 7) {
        const ConvTrainSizes z = train_conv_sizes(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
        std::printf("%zu %zu %zu %zu %zu %zu\n", z.grad_floats, z.q_halfs[0], z.q_halfs[1], z.q_halfs[2], z.q_halfs[3], z.part_floats);
        return 0;
    }
    if (cmd == "fits" && argc == 7) {
        const int ih3 = std::atoi(argv[2]), iw3 = std::atoi(argv[3]), n_cap = std::atoi(argv[4]), cu = std::atoi(argv[5]), lowest = std::atoi(argv[6]);
        const ConvTrainSizes z = train_conv_sizes(ih3, iw3, n_cap, cu, lowest);
        size_t most = 0;
        for (int n = 1; n <= n_cap; ++n)
            for (int j = lowest; j < kConvTrainLayers; ++j) {
                const ConvGeom g = train_conv_geom(j, ih3 - 2 * j, iw3 - 2 * j);
                const ConvSplit s = train_conv_split(g, n, cu);
                const size_t need = (size_t)s.slices * (g.kernel_count() + g.COUT), out = (size_t)g.out_pixels(n) * g.COUT;
                if (need > z.part_floats || out > z.q_halfs[j] || out > z.grad_floats || s.slices > train_conv_max_slices(g, n_cap, cu)) {
                    std::printf("n = %d, layer %d: %d slices need %zu floats of %zu (delta %zu of %zu)\n", n, j, s.slices, need, z.part_floats, out, z.q_halfs[j]);
                    return 0;
                }
                most = std::max(most, need);
            }
        std::printf("ok %zu\n", most);
        return 0;
    }
    if (cmd == "debug" && argc == 6) {
        const ConvGeom g = train_conv_geom(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
        for (int w = 0; w <= 9; ++w) std::printf("%zu\n", train_conv_debug_floats(g, w, std::atoi(argv[5])));
        std::printf("%zu\n", train_conv_debug_floats(g, -1, std::atoi(argv[5])));
        return 0;
    }
    return 2;
}
