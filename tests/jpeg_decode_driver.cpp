// Drives csrc/trsim_jpeg_decode.hpp on the host (tests/test_jpeg_decode_cpu.py builds this file with the address and undefined-behaviour sanitizers).
// Every file is decoded from a heap buffer of exactly its length, so that a read beyond the file is a sanitizer report.
//   jpeg_decode_driver decode <H> <W> <file> ...   per file one line: the status, and behind status 0 the frame uint8[H][W][3] as hex
//   jpeg_decode_driver fuzz <H> <W> <file>         every prefix of the file, and the file with each byte up to the scan's start altered in turn
//                                                  (xor 0xFF, xor 0x01, + 1); prints how many inputs ended in each status
// The loop below is plain data movement over whole planes; every rule it applies is a function of the header.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_jpeg_decode.hpp"

using namespace trsim::jpeg;

static int decode_file(const uint8_t* bytes, int len, int H, int W, std::vector<uint8_t>* frame)
{
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(len > 0 ? len : 1));       // (heap: the sanitizer guards both ends)
    if (len > 0) std::memcpy(exact, bytes, len);
    SpanFile f{exact, len};
    FileHeader h;
    int st = parse_header(f, H, W, &h);
    if (st == kDecoded) {
        const Geometry g = geometry(H, W);
        const int ys = 16 * g.mcu_cols, cs = 8 * g.mcu_cols;
        std::vector<DecodeTables> t(1);
        build_tables(f, h, &t[0]);
        std::vector<uint8_t> yp((size_t)16 * g.mcu_rows * ys), cp[2];
        cp[0].resize((size_t)8 * g.mcu_rows * cs); cp[1].resize(cp[0].size());
        BitReader<SpanFile> r;
        r.start(&f, h.scan);
        int pred[3] = {0, 0, 0};
        for (int my = 0; my < g.mcu_rows && st == kDecoded; ++my)
            for (int mx = 0; mx < g.mcu_cols && st == kDecoded; ++mx)
                for (int k = 0; k < kBlocksPerMcu && st == kDecoded; ++k) {
                    const int c = k < 4 ? 0 : k - 3;
                    int16_t coef[64] = {0};
                    st = decode_block(r, t[0].huff[h.td[c]], t[0].huff[2 + h.ta[c]], t[0].zz, &pred[c], coef);
                    if (st != kDecoded) break;
                    int32_t ws[64];
                    for (int col = 0; col < 8; ++col) {
                        int32_t d[8];
                        for (int row = 0; row < 8; ++row) d[row] = coef[row * 8 + col] * (int32_t)t[0].q[c][row * 8 + col];
                        idct_pass(d, 11);
                        for (int row = 0; row < 8; ++row) ws[row * 8 + col] = d[row];
                    }
                    for (int row = 0; row < 8; ++row) {
                        int32_t d[8];
                        for (int col = 0; col < 8; ++col) d[col] = ws[row * 8 + col];
                        idct_pass(d, 18);
                        uint8_t* out = k < 4 ? &yp[(size_t)(16 * my + 8 * (k >> 1) + row) * ys + 16 * mx + 8 * (k & 1)] : &cp[k - 4][(size_t)(8 * my + row) * cs + 8 * mx];
                        for (int col = 0; col < 8; ++col) out[col] = (uint8_t)sample_of(d[col]);
                    }
                }
        if (st == kDecoded) {
            frame->assign((size_t)H * W * 3, 0);
            planes_to_frame(g, yp.data(), ys, cp[0].data(), cp[1].data(), cs, frame->data());
        }
    }
    std::free(exact);
    return st;
}

static std::vector<uint8_t> read_file(const char* path)
{
    std::vector<uint8_t> d;
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(4);
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
    std::fclose(f);
    return d;
}

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const int H = std::atoi(argv[2]), W = std::atoi(argv[3]);
    std::vector<uint8_t> frame;
    if (!std::strcmp(argv[1], "decode")) {
        for (int i = 4; i < argc; ++i) {
            const std::vector<uint8_t> d = read_file(argv[i]);
            const int st = decode_file(d.data(), (int)d.size(), H, W, &frame);
            std::printf("%d", st);
            if (st == kDecoded) {
                std::printf(" ");
                for (uint8_t v : frame) std::printf("%02x", v);
            }
            std::printf("\n");
        }
    } else if (!std::strcmp(argv[1], "fuzz")) {
        const std::vector<uint8_t> d = read_file(argv[4]);
        SpanFile f{d.data(), (int)d.size()};
        FileHeader h;
        if (parse_header(f, H, W, &h) != kDecoded) return 3;
        long count[5] = {0, 0, 0, 0, 0};
        for (size_t n = 0; n <= d.size(); ++n) ++count[decode_file(d.data(), (int)n, H, W, &frame)];
        std::vector<uint8_t> m = d;
        for (int i = 0; i < h.scan; ++i)
            for (int how = 0; how < 3; ++how) {
                m[i] = how == 0 ? d[i] ^ 0xFF : how == 1 ? d[i] ^ 0x01 : (uint8_t)(d[i] + 1);
                ++count[decode_file(m.data(), (int)m.size(), H, W, &frame)];
                m[i] = d[i];
            }
        std::printf("%ld %ld %ld %ld %ld\n", count[0], count[1], count[2], count[3], count[4]);
    } else {
        return 2;
    }
    return 0;
}
