// trsim_jpeg_tables.hpp — the tub image format (include/trsim_spec.h, "tub image (JPEG)") as tables and integer arithmetic: quantisation tables
// for a quality, the header bytes SOI..SOS, the Huffman tables in the form the kernel reads, the MCU geometry with its edge and dummy-block rules,
// the per-sample arithmetic (colour, downsampling, the two DCT passes, the quantiser) and the forward sample rule of a 2 x 2 quad (sample_quad; over a
// whole frame on the host: sample_planes).  Compiles without HIP (tests/jpeg_driver.cpp drives it under the sanitizers).  trs_jpeg_kernel and
// trs_jpeg_codec_kernel take every rule from here, and apply sample_quad through the one stage both share (sample_stripe, trsim_jpeg_device.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define TRS_JPEG_HD __host__ __device__ inline
#else
#define TRS_JPEG_HD inline
#endif

namespace trsim {
namespace jpeg {

constexpr int kHeaderBytes = 623;            // SOI 2 | APP0 18 | DQT 2 x 69 | SOF0 19 | DHT 33 + 183 + 33 + 183 | SOS 14
constexpr int kBlocksPerMcu = 6;             // Y00 Y01 Y10 Y11 Cb Cr
constexpr int kMaxBlockBits = 20 + 63 * 26;  // DC: a code of <= 9 bits + 11 extra; every AC: a code of <= 16 bits + 10 extra (ZRL and EOB stand for zeros, which cost less)
constexpr int kMaxBlockBytes = (kMaxBlockBits + 7) / 8;   // 208
constexpr int kThreads = 256;                // threads of a workgroup of trs_jpeg_kernel: one lane per block of an MCU row in the entropy stage
constexpr int kWgsPerCu = 4;                 // trs_jpeg_kernel runs min(frames, kWgsPerCu x CU count) workgroups, each looping over frames
constexpr int kMaxLdsBytes = 160 * 1024;

// ---- JPEG standard, Annex K ------------------------------------------------------------------------------------------------------------
constexpr uint8_t kLumBase[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChrBase[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// natural index of the k-th coefficient of the zig-zag scan
constexpr uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Huffman table specifications: the number of codes of each length 1..16, then the symbols in code order
struct HuffSpec { uint8_t ident; uint8_t counts[16]; int n; const uint8_t* symbols; };
constexpr uint8_t kDcSymbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumSymbols[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChrSymbols[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
// in the header's order: DC0, AC0, DC1, AC1 (ident: class << 4 | table)
constexpr HuffSpec kHuff[4] = {
    {0x00, {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, kDcSymbols},
    {0x10, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, kAcLumSymbols},
    {0x01, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, kDcSymbols},
    {0x11, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, kAcChrSymbols},
};

// ---- what the kernel reads: one block per quality, built on the host and copied to the device ---------------------------------------------
struct Tables {
    uint32_t ac[2][256];        // [luminance | chrominance][run << 4 | size]: length << 16 | code (0: not a symbol of the table)
    uint32_t dc[2][16];         // [..][size 0..11]
    int32_t qv[2][64];          // quantisation steps << 3 (the DCT's output is scaled by 8), natural order
    uint8_t zz_pos[64];         // position in the zig-zag scan of natural index i
    uint8_t header[kHeaderBytes + 1];
};

inline void quant_table(int quality, int chroma, uint8_t out[64])      // natural order; quality in 1..100
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const uint8_t* base = chroma ? kChrBase : kLumBase;
    for (int i = 0; i < 64; ++i) {
        const int v = (base[i] * scale + 50) / 100;
        out[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

// length << 16 | code per symbol: the codes of one length count up in symbol order, and double when the length grows
inline void huff_codes(const HuffSpec& s, uint32_t* out, int n_out)
{
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int j = 0; j < s.counts[len - 1]; ++j, ++k, ++code) out[s.symbols[k]] = (uint32_t)len << 16 | code;
        code <<= 1;
    }
}

inline std::vector<uint8_t> header_bytes(int H, int W, int quality)
{
    std::vector<uint8_t> o;
    auto put = [&o](std::initializer_list<int> b) { for (int v : b) o.push_back((uint8_t)v); };
    auto be16 = [&o](int v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)(v & 255)); };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0}); be16(16); put({'J', 'F', 'I', 'F', 0, 1, 1, 0}); be16(1); be16(1); put({0, 0});
    for (int t = 0; t < 2; ++t) {
        uint8_t q[64];
        quant_table(quality, t, q);
        put({0xFF, 0xDB}); be16(67); put({t});
        for (int k = 0; k < 64; ++k) o.push_back(q[kZigzag[k]]);
    }
    put({0xFF, 0xC0}); be16(17); put({8}); be16(H); be16(W); put({3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (const HuffSpec& s : kHuff) {
        put({0xFF, 0xC4}); be16(19 + s.n); put({s.ident});
        for (int i = 0; i < 16; ++i) o.push_back(s.counts[i]);
        for (int i = 0; i < s.n; ++i) o.push_back(s.symbols[i]);
    }
    put({0xFF, 0xDA}); be16(12); put({3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return o;
}

// the quantisation steps << 3 of a quality, as the quantiser takes them (Tables::qv, and the camera codec's block steps)
inline void quant_steps(int quality, int32_t qv[2][64])
{
    for (int c = 0; c < 2; ++c) {
        uint8_t q[64];
        quant_table(quality, c, q);
        for (int i = 0; i < 64; ++i) qv[c][i] = (int32_t)q[i] << 3;
    }
}

inline void build_tables(int H, int W, int quality, Tables* t)
{
    huff_codes(kHuff[0], t->dc[0], 16); huff_codes(kHuff[1], t->ac[0], 256);
    huff_codes(kHuff[2], t->dc[1], 16); huff_codes(kHuff[3], t->ac[1], 256);
    quant_steps(quality, t->qv);
    for (int k = 0; k < 64; ++k) t->zz_pos[kZigzag[k]] = (uint8_t)k;
    const std::vector<uint8_t> h = header_bytes(H, W, quality);
    for (int i = 0; i <= kHeaderBytes; ++i) t->header[i] = i < (int)h.size() ? h[i] : 0;
}

// ---- geometry: MCUs of 16 x 16 pixels in raster order, blocks Y00 Y01 Y10 Y11 Cb Cr ------------------------------------------------------------
struct Geometry {
    int H, W;
    int mcu_rows, mcu_cols;     // ceil(H / 16), ceil(W / 16)
    int blk_rows, blk_cols;     // ceil(H / 8), ceil(W / 8): the Y blocks that hold image samples
    int c_rows;                 // ceil(H / 2): rows of the downsampled chroma plane that come from image rows
};
TRS_JPEG_HD Geometry geometry(int H, int W)
{
    Geometry g;
    g.H = H; g.W = W;
    g.mcu_rows = (H + 15) / 16; g.mcu_cols = (W + 15) / 16;
    g.blk_rows = (H + 7) / 8; g.blk_cols = (W + 7) / 8;
    g.c_rows = (H + 1) / 2;
    return g;
}
TRS_JPEG_HD int blocks_per_stripe(const Geometry& g) { return kBlocksPerMcu * g.mcu_cols; }
// Y block k (0..3) of MCU (my, mx) lies wholly beyond the image's block rows or columns: all AC zero, the DC of the block before it in the MCU
TRS_JPEG_HD bool y_dummy(const Geometry& g, int my, int mx, int k) { return 2 * my + (k >> 1) >= g.blk_rows || 2 * mx + (k & 1) >= g.blk_cols; }
// the image row / column a sample of the padded Y plane is taken from: the last row and column replicate
TRS_JPEG_HD int y_src_row(const Geometry& g, int r) { return r < g.H ? r : g.H - 1; }
TRS_JPEG_HD int y_src_col(const Geometry& g, int c) { return c < g.W ? c : g.W - 1; }
// the two image rows / columns behind row r / column c of the padded, downsampled chroma plane: the full-resolution plane replicates its last row
// (to an even height) and column (to 16 * mcu_cols), and the DOWNSAMPLED plane replicates its last row below c_rows
TRS_JPEG_HD void c_src_rows(const Geometry& g, int r, int* r0, int* r1)
{
    const int rr = r < g.c_rows ? r : g.c_rows - 1;
    *r0 = y_src_row(g, 2 * rr); *r1 = y_src_row(g, 2 * rr + 1);
}
TRS_JPEG_HD void c_src_cols(const Geometry& g, int c, int* c0, int* c1) { *c0 = y_src_col(g, 2 * c); *c1 = y_src_col(g, 2 * c + 1); }

// ---- per-sample arithmetic -----------------------------------------------------------------------------------------------------------------
constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }
TRS_JPEG_HD int luma(int r, int g, int b) { return (fix16(.299) * r + fix16(.587) * g + fix16(.114) * b + 32768) >> 16; }
TRS_JPEG_HD int chroma_b(int r, int g, int b) { return (-fix16(.16874) * r - fix16(.33126) * g + fix16(.5) * b + (128 << 16) + 32767) >> 16; }
TRS_JPEG_HD int chroma_r(int r, int g, int b) { return (fix16(.5) * r - fix16(.41869) * g - fix16(.08131) * b + (128 << 16) + 32767) >> 16; }
TRS_JPEG_HD int downsample(int a, int b, int c, int d, int out_col) { return (a + b + c + d + 1 + (out_col & 1)) >> 2; }

// the forward sample rule: the samples of the 2 x 2 quad (qr, qc) of the padded planes — Y rows 2 qr, 2 qr + 1 and columns 2 qc, 2 qc + 1, and the
// one sample (qr, qc) of either downsampled chroma plane.  px(r, c): the three RGB bytes of image pixel (r, c)
struct QuadSamples { uint8_t y[2][2], cb, cr; };
template <class Px>
TRS_JPEG_HD QuadSamples sample_quad(const Geometry& g, int qr, int qc, Px px)
{
    QuadSamples s;
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const uint8_t* p = px(y_src_row(g, 2 * qr + dy), y_src_col(g, 2 * qc + dx));
            s.y[dy][dx] = (uint8_t)luma(p[0], p[1], p[2]);
        }
    int r0, r1, c0, c1;
    c_src_rows(g, qr, &r0, &r1);
    c_src_cols(g, qc, &c0, &c1);
    const uint8_t *a = px(r0, c0), *b = px(r0, c1), *c = px(r1, c0), *d = px(r1, c1);
    s.cb = (uint8_t)downsample(chroma_b(a[0], a[1], a[2]), chroma_b(b[0], b[1], b[2]), chroma_b(c[0], c[1], c[2]), chroma_b(d[0], d[1], d[2]), qc);
    s.cr = (uint8_t)downsample(chroma_r(a[0], a[1], a[2]), chroma_r(b[0], b[1], b[2]), chroma_r(c[0], c[1], c[2]), chroma_r(d[0], d[1], d[2]), qc);
    return s;
}
// ... over a whole uint8[H][W][3] frame: yp[16 mcu_rows][16 mcu_cols], cb and cr [8 mcu_rows][8 mcu_cols]
inline void sample_planes(const Geometry& g, const uint8_t* src, uint8_t* yp, uint8_t* cb, uint8_t* cr)
{
    const int ys = 16 * g.mcu_cols, cs = 8 * g.mcu_cols;
    for (int qr = 0; qr < 8 * g.mcu_rows; ++qr)
        for (int qc = 0; qc < cs; ++qc) {
            const QuadSamples s = sample_quad(g, qr, qc, [&](int r, int c) { return src + ((size_t)r * g.W + c) * 3; });
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) yp[(size_t)(2 * qr + dy) * ys + 2 * qc + dx] = s.y[dy][dx];
            cb[(size_t)qr * cs + qc] = s.cb;
            cr[(size_t)qr * cs + qc] = s.cr;
        }
}

TRS_JPEG_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// one pass of the integer forward DCT over d[0..7] in place.  FIRST (rows, samples - 128): output scaled by 4 beyond the DCT's own factor; the
// second pass (columns) removes that again and leaves the coefficients scaled by 8
template <bool FIRST>
TRS_JPEG_HD void fdct_pass(int d[8])
{
    constexpr int n = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    const int e = (t12 + t13) * 4433;
    d[2] = descale(e + t13 * 6270, n);
    d[6] = descale(e - t12 * 15137, n);
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    d[7] = descale(t4 * 2446 + z1 + z3, n);
    d[5] = descale(t5 * 16819 + z2 + z4, n);
    d[3] = descale(t6 * 25172 + z2 + z3, n);
    d[1] = descale(t7 * 12299 + z1 + z4, n);
}
// qv: the quantisation step << 3
TRS_JPEG_HD int quantise(int c, int qv)
{
    const int a = (c < 0 ? -c : c) + (qv >> 1);
    const int v = a >= qv ? a / qv : 0;
    return c < 0 ? -v : v;
}
// number of bits of |v| (the "size" of a coefficient); v in -2047..2047
TRS_JPEG_HD int magnitude_bits(int v)
{
    const int a = v < 0 ? -v : v;
    return a ? 32 - __builtin_clz((unsigned)a) : 0;
}
// the size's extra bits: v, or v - 1 for a negative v, in `bits` bits
TRS_JPEG_HD uint32_t extra_bits(int v, int bits) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << bits) - 1u); }

// LDS one MCU row needs in the kernel (csrc/trsim_jpeg.hip lays it out in this order), per MCU column: samples 16 x 16 Y + 2 x 8 x 8 chroma,
// a 6 x 64 int32 workspace (the raw RGB rows before the DCT, the bit stream after it) and 6 coefficient blocks of 66 int16
constexpr int kCoefStride = 66;              // int16 per block: 33 dwords, so that a lane per block reads conflict-free
struct StripeLds { int off_tab, off_y, off_c, off_ws, off_coef, off_scan, total; };
inline StripeLds stripe_lds(int W)
{
    const int mw = (W + 15) / 16;
    auto up = [](int v) { return (v + 15) & ~15; };
    StripeLds l;
    l.off_tab = 0;
    l.off_y = up((int)sizeof(Tables));
    l.off_c = l.off_y + 256 * mw;
    l.off_ws = l.off_c + 128 * mw;
    l.off_coef = l.off_ws + up(kBlocksPerMcu * 256 * mw + 16);
    l.off_scan = l.off_coef + up(kBlocksPerMcu * kCoefStride * 2 * mw);
    l.total = l.off_scan + 64;
    return l;
}
static_assert(kMaxBlockBytes <= 256 - 8, "a block's bits must fit in its share of the workspace");
static_assert(48 * 16 <= kBlocksPerMcu * 256, "the 16 raw RGB rows of an MCU column must fit in its share of the workspace");

}  // namespace jpeg
}  // namespace trsim
