// Drives csrc/trsim_jpeg_tables.hpp on the host (tests/test_jpeg_cpu.py builds this file with the address and undefined-behaviour sanitizers):
//   jpeg_driver quant <quality>               the luminance and the chrominance quantisation table, natural order
//   jpeg_driver header <H> <W> <quality>      the header bytes SOI..SOS as hex, as build_tables() files them for the kernel
//   jpeg_driver huffman                       dc0 ac0 dc1 ac1 as the kernel reads them: length << 16 | code per symbol
//   jpeg_driver zigzag                        natural index of the k-th coefficient, recovered from the kernel's zz_pos
//   jpeg_driver geometry <H> <W>              MCU rows and columns, blocks per MCU row, header bytes | the dummy flag of every (my, mx, Y block) |
//                                             the image row behind every padded Y row | the two image rows behind every padded chroma row
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../triton-racer-sim_amd/csrc/trsim_jpeg_tables.hpp"

using namespace trsim::jpeg;

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const char* cmd = argv[1];
    auto arg = [&](int i) { return i < argc ? std::atoi(argv[i]) : 0; };
    std::unique_ptr<Tables> t(new Tables);
    if (!std::strcmp(cmd, "quant")) {
        build_tables(120, 160, arg(2), t.get());
        for (int c = 0; c < 2; ++c) {
            uint8_t q[64];
            quant_table(arg(2), c, q);
            std::printf("q%d", c);
            for (int i = 0; i < 64; ++i) {
                if (t->qv[c][i] != q[i] << 3) return 3;
                std::printf(" %d", q[i]);
            }
            std::printf("\n");
        }
    } else if (!std::strcmp(cmd, "header")) {
        build_tables(arg(2), arg(3), arg(4), t.get());
        if ((int)header_bytes(arg(2), arg(3), arg(4)).size() != kHeaderBytes) return 3;
        for (int i = 0; i < kHeaderBytes; ++i) std::printf("%02x", t->header[i]);
        std::printf("\n");
    } else if (!std::strcmp(cmd, "huffman")) {
        build_tables(120, 160, 75, t.get());
        const char* names[4] = {"dc0", "ac0", "dc1", "ac1"};
        for (int k = 0; k < 4; ++k) {
            const bool ac = k & 1;
            const uint32_t* tab = ac ? t->ac[k >> 1] : t->dc[k >> 1];
            std::printf("%s", names[k]);
            for (int i = 0; i < (ac ? 256 : 12); ++i) std::printf(" %u", tab[i]);
            std::printf("\n");
        }
    } else if (!std::strcmp(cmd, "zigzag")) {
        build_tables(120, 160, 75, t.get());
        int nat[64];
        for (int i = 0; i < 64; ++i) nat[t->zz_pos[i]] = i;
        for (int k = 0; k < 64; ++k) std::printf("%d%s", nat[k], k == 63 ? "\n" : " ");
    } else if (!std::strcmp(cmd, "geometry")) {
        const Geometry g = geometry(arg(2), arg(3));
        std::printf("%d %d %d %d\n", g.mcu_rows, g.mcu_cols, blocks_per_stripe(g), kHeaderBytes);
        for (int my = 0; my < g.mcu_rows; ++my)
            for (int mx = 0; mx < g.mcu_cols; ++mx)
                for (int k = 0; k < 4; ++k) std::printf("%d", y_dummy(g, my, mx, k) ? 1 : 0);
        std::printf("\n");
        for (int r = 0; r < 16 * g.mcu_rows; ++r) std::printf("%d ", y_src_row(g, r));
        std::printf("\n");
        for (int r = 0; r < 8 * g.mcu_rows; ++r) {
            int r0, r1;
            c_src_rows(g, r, &r0, &r1);
            std::printf("%d,%d ", r0, r1);
        }
        std::printf("\n");
    } else if (!std::strcmp(cmd, "blocks")) {
        // jpeg_driver blocks <H> <W> <quality> <raw RGB file>: the quantised blocks of every MCU in zig-zag order, one line per block, from the
        // header's sample_planes and arithmetic alone (the dummy blocks' DC is left to the caller: it is a rule about neighbours, checked on the GPU)
        const int H = arg(2), W = arg(3);
        const Geometry g = geometry(H, W);
        build_tables(H, W, arg(4), t.get());
        std::vector<uint8_t> px((size_t)H * W * 3);
        FILE* f = argc > 5 ? std::fopen(argv[5], "rb") : nullptr;
        if (!f || std::fread(px.data(), 1, px.size(), f) != px.size()) return 4;
        std::fclose(f);
        const int ys = 16 * g.mcu_cols, cs = 8 * g.mcu_cols;
        std::vector<uint8_t> yp((size_t)16 * g.mcu_rows * ys), cp[2];
        cp[0].resize((size_t)8 * g.mcu_rows * cs); cp[1].resize(cp[0].size());
        sample_planes(g, px.data(), yp.data(), cp[0].data(), cp[1].data());
        for (int my = 0; my < g.mcu_rows; ++my)
            for (int mx = 0; mx < g.mcu_cols; ++mx)
                for (int k = 0; k < kBlocksPerMcu; ++k) {
                    int ws[64], out[64];
                    for (int r = 0; r < 8; ++r) {
                        const uint8_t* sp = k < 4 ? &yp[(size_t)(16 * my + 8 * (k >> 1) + r) * ys + 16 * mx + 8 * (k & 1)] : &cp[k - 4][(size_t)(8 * my + r) * cs + 8 * mx];
                        int d[8];
                        for (int c = 0; c < 8; ++c) d[c] = sp[c] - 128;
                        fdct_pass<true>(d);
                        for (int c = 0; c < 8; ++c) ws[r * 8 + c] = d[c];
                    }
                    for (int c = 0; c < 8; ++c) {
                        int d[8];
                        for (int r = 0; r < 8; ++r) d[r] = ws[r * 8 + c];
                        fdct_pass<false>(d);
                        for (int r = 0; r < 8; ++r) out[t->zz_pos[r * 8 + c]] = k < 4 && y_dummy(g, my, mx, k) ? 0 : quantise(d[r], t->qv[k >= 4][r * 8 + c]);
                    }
                    for (int i = 0; i < 64; ++i) std::printf("%d%s", out[i], i == 63 ? "\n" : " ");
                }
    } else if (!std::strcmp(cmd, "bits")) {
        // jpeg_driver bits: magnitude_bits and extra_bits of every value a coefficient or a DC difference can take
        for (int v = -2047; v <= 2047; ++v) std::printf("%d %d %u\n", v, magnitude_bits(v), extra_bits(v, magnitude_bits(v)));
    } else {
        return 2;
    }
    return 0;
}
