// trsim_jpeg_decode.hpp — reading a tub image (include/trsim_spec.h, "tub image (JPEG), decoding") as rules that compile for host and device: the
// marker walk with its status decision, the Huffman tables taken from the file, the bit reader, symbol and block decoding, the inverse DCT pass,
// the triangle upsampling and the colour formulas, sample planes to a whole frame on the host (planes_to_frame), and the LDS plan of the kernel.
// csrc/trsim_jpeg_decode.hip holds the kernel's data movement and tests/jpeg_decode_driver.cpp a plain host loop; both take every rule from here.  The
// kernel's form of planes_to_frame, four pixels a lane, is output_mcu_row (trsim_jpeg_device.hpp), which the camera codec's kernel shares.
// Every read of a file byte goes through the `at(i)` of a file type F that knows the file's length (SpanFile here, the kernel's LDS window there): it
// answers 0 beyond the end and never reads there.  Every loop over file bytes is bounded: the marker walk moves forward by >= 2 bytes a turn and
// stops at the length, the bit reader refills at most 8 bytes a call and stops at the length or at a marker, a block decodes at most 64 symbols.
#pragma once
#include <cstddef>
#include <cstdint>

#include "trsim_jpeg_tables.hpp"

namespace trsim {
namespace jpeg {

// d_status of trs_decode_jpeg (include/trsim.h)
enum DecodeStatus : int { kDecoded = 0, kSkipped = 1, kUnsupported = 2, kSizeDiffers = 3, kCorrupt = 4 };

constexpr int kLookBits = 8;                 // bits of the first-level Huffman lookup: symbol and length in one read for codes up to this length
constexpr int kDecodeWaves = 4;              // independent waves (files in flight) of a workgroup of trs_jpeg_decode_kernel
constexpr int kDecodeWgsPerCu = 2;           // the kernel runs min(ceil(files / kDecodeWaves), kDecodeWgsPerCu x CU count) workgroups, each wave looping over files
constexpr int kMcuGroup = 4;                 // MCUs decoded before the 64 lanes transform their blocks
constexpr int kWindowBytes = 512;            // file bytes a wave holds in LDS at a time
constexpr int kDecCoefStride = 72;             // int16 per coefficient block in LDS (natural order): 36 dwords, so that 8 blocks x 4 dwords of a row hit 32 banks
constexpr int kWsRowStride = 9, kWsBlockStride = 72;   // dwords: the 8 x 8 intermediate of a block between the passes, conflict-free by column and by row
constexpr int kChromaRing = 3;               // MCU rows of chroma samples kept: the one being written, the one being output and the one above it

struct SpanFile {                            // a file in host memory (or any directly addressable memory)
    const uint8_t* p; int len;
    TRS_JPEG_HD int size() const { return len; }
    TRS_JPEG_HD int at(int i) const { return (unsigned)i < (unsigned)len ? p[i] : 0; }
};

TRS_JPEG_HD int zigzag_natural(int k)        // natural index of the k-th coefficient of the zig-zag scan (kZigzag, for host and device)
{
    constexpr uint8_t t[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63];
}

// ---- the marker walk ---------------------------------------------------------------------------------------------------------------------------
struct FileHeader {
    int scan;                // offset of the first entropy-coded byte
    int dqt[4];              // offset of the 64 entries (zig-zag order) of quantisation table t, -1: none
    int dht[2][2];           // [DC | AC][table]: offset of the 16 counts, the symbols follow them; -1: none
    int tq[3], td[3], ta[3]; // per component: quantisation, DC and AC table
};

// SOI .. SOS of a file that is expected to hold an H x W frame -> kDecoded and *h, or the status that ends the file.  Decisions are taken in file
// order: the first segment that is unsupported or broken decides; the size is compared at SOS.
template <class F>
TRS_JPEG_HD int parse_header(F& f, int H, int W, FileHeader* h)
{
    const int n = f.size();
    for (int t = 0; t < 4; ++t) h->dqt[t] = -1;
    h->dht[0][0] = h->dht[0][1] = h->dht[1][0] = h->dht[1][1] = -1;
    if (n < 2 || f.at(0) != 0xFF || f.at(1) != 0xD8) return kCorrupt;
    int pos = 2, fh = -1, fw = -1;
    for (;;) {
        if (pos + 4 > n || f.at(pos) != 0xFF) return kCorrupt;
        const int m = f.at(pos + 1);
        if (m == 0xFF) return kUnsupported;                               // fill bytes
        if (m <= 0x01 || (m >= 0xD0 && m <= 0xD9)) return kCorrupt;       // markers without a segment have no place before the scan
        const int length = f.at(pos + 2) << 8 | f.at(pos + 3), seg = pos + 4, end = pos + 2 + length;
        if (length < 2 || end > n) return kCorrupt;
        if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
            if (m == 0xEE && end - seg >= 5 && f.at(seg) == 'A' && f.at(seg + 1) == 'd' && f.at(seg + 2) == 'o' && f.at(seg + 3) == 'b' && f.at(seg + 4) == 'e')
                return kUnsupported;
        } else if (m == 0xDB) {
            for (int q = seg; q < end; q += 65) {
                const int pt = f.at(q);
                if (pt >> 4) return kUnsupported;                         // 16-bit tables
                if ((pt & 15) > 3 || q + 65 > end) return kCorrupt;
                h->dqt[pt & 15] = q + 1;
            }
        } else if (m == 0xC4) {
            for (int q = seg; q < end;) {
                const int cls = f.at(q) >> 4, ident = f.at(q) & 15;
                if (cls > 1 || ident > 3 || q + 17 > end) return kCorrupt;
                if (ident > 1) return kUnsupported;                       // baseline has two tables per class
                int total = 0, code = 0;
                for (int l = 1; l <= 16; ++l) {                           // more codes of a length than there is room for
                    const int c = f.at(q + l);
                    total += c; code += c;
                    if (code > 1 << l) return kCorrupt;
                    code <<= 1;
                }
                if (total > 256 || q + 17 + total > end) return kCorrupt;
                h->dht[cls][ident] = q + 1;
                q += 17 + total;
            }
        } else if (m == 0xC0) {
            if (fh >= 0 || length < 8 || length != 8 + 3 * f.at(seg + 5)) return kCorrupt;
            if (f.at(seg) != 8 || f.at(seg + 5) != 3) return kUnsupported;
            for (int c = 0; c < 3; ++c)
                if (f.at(seg + 6 + 3 * c) != c + 1 || f.at(seg + 7 + 3 * c) != (c ? 0x11 : 0x22)) return kUnsupported;
            for (int c = 0; c < 3; ++c) {
                h->tq[c] = f.at(seg + 8 + 3 * c);
                if (h->tq[c] > 3) return kCorrupt;
            }
            fh = f.at(seg + 1) << 8 | f.at(seg + 2);
            fw = f.at(seg + 3) << 8 | f.at(seg + 4);
        } else if (m == 0xDA) {
            if (fh < 0 || length < 6 || length != 6 + 2 * f.at(seg)) return kCorrupt;
            if (f.at(seg) != 3) return kUnsupported;
            for (int c = 0; c < 3; ++c) {
                const int t = f.at(seg + 2 + 2 * c);
                if (f.at(seg + 1 + 2 * c) != c + 1 || (t >> 4) > 1 || (t & 15) > 1) return kUnsupported;
                h->td[c] = t >> 4; h->ta[c] = t & 15;
            }
            if (f.at(seg + 7) != 0 || f.at(seg + 8) != 63 || f.at(seg + 9) != 0) return kUnsupported;
            if (fw <= 4) return kUnsupported;                             // a chroma plane of width <= 2: libjpeg-turbo leaves the triangle filter
            if (fh != H || fw != W || fh < 1) return kSizeDiffers;
            for (int c = 0; c < 3; ++c)
                if (h->dqt[h->tq[c]] < 0 || h->dht[0][h->td[c]] < 0 || h->dht[1][h->ta[c]] < 0) return kCorrupt;
            h->scan = end;
            return kDecoded;
        } else {
            return kUnsupported;                                          // other frame types (progressive, extended, arithmetic), DRI, DNL, ...
        }
        pos = end;
    }
}

// ---- Huffman tables as the decoder reads them ------------------------------------------------------------------------------------------------
struct HuffTable {
    uint16_t look[1 << kLookBits];   // by the next kLookBits bits: length << 8 | symbol of a code of up to kLookBits bits, 0: a longer code or none
    int32_t maxcode[18];             // [l]: the largest code of length l, -1: none
    int32_t valoff[18];              // [l]: index in sym[] of the first code of length l, minus that code
    uint8_t sym[256];                // the symbols in code order
};
struct DecodeTables {
    HuffTable huff[4];               // DC0 DC1 AC0 AC1 (the tables the scan selects; an absent one is never read)
    uint16_t q[3][64];               // per component, NATURAL order
    uint8_t zz[64];                  // zigzag_natural(k): where the serial chain looks it up (a table in constant memory would put a global load into the chain)
};

// table `t` from the 16 counts at `off` and the symbols behind them (parse_header has checked their sum and that no length is over-subscribed)
template <class F>
TRS_JPEG_HD void build_huffman(F& f, int off, HuffTable* t)
{
    for (int i = 0; i < (1 << kLookBits); ++i) t->look[i] = 0;
    int code = 0, k = 0;
    t->maxcode[0] = t->maxcode[17] = -1; t->valoff[0] = t->valoff[17] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = f.at(off + l - 1);
        t->valoff[l] = k - code;
        for (int j = 0; j < n && k < 256; ++j, ++k, ++code) {
            const int s = f.at(off + 16 + k);
            t->sym[k] = (uint8_t)s;
            if (l <= kLookBits)
                for (int i = 0; i < 1 << (kLookBits - l); ++i) t->look[(code << (kLookBits - l) | i) & ((1 << kLookBits) - 1)] = (uint16_t)(l << 8 | s);
        }
        t->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
}

template <class F>
TRS_JPEG_HD void build_tables(F& f, const FileHeader& h, DecodeTables* t)
{
    for (int cls = 0; cls < 2; ++cls)
        for (int id = 0; id < 2; ++id)
            if (h.dht[cls][id] >= 0) build_huffman(f, h.dht[cls][id], &t->huff[2 * cls + id]);
    for (int k = 0; k < 64; ++k) t->zz[k] = (uint8_t)zigzag_natural(k);
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) t->q[c][t->zz[k]] = (uint16_t)f.at(h.dqt[h.tq[c]] + k);
}

// ---- entropy decoding ------------------------------------------------------------------------------------------------------------------------
// The scan's bits, most significant first, a 0x00 behind a 0xFF dropped.  The bits end at the file's end or at a marker; cnt < 0 after a skip means that
// bits beyond that end were taken: the file is corrupt.
template <class F>
struct BitReader {
    F* f; int pos; int cnt; uint64_t acc;    // acc: the next cnt bits from bit 63 down, zeros below them
    TRS_JPEG_HD void start(F* file, int at) { f = file; pos = at; cnt = 0; acc = 0; }
    TRS_JPEG_HD void fill()                  // cnt >= 32 afterwards, unless the bits end before that
    {
        if (cnt >= 32) return;
        if (pos + 4 <= f->size()) {          // four bytes at once (four independent reads) where none of them is a 0xFF
            const int b0 = f->at(pos), b1 = f->at(pos + 1), b2 = f->at(pos + 2), b3 = f->at(pos + 3);
            if (b0 != 0xFF && b1 != 0xFF && b2 != 0xFF && b3 != 0xFF) {
                acc |= (uint64_t)((uint32_t)b0 << 24 | (uint32_t)b1 << 16 | (uint32_t)b2 << 8 | (uint32_t)b3) << (32 - cnt);
                cnt += 32; pos += 4;
                return;
            }
        }
        while (cnt < 32) {
            if (pos >= f->size()) break;
            const int b = f->at(pos);
            if (b == 0xFF) {
                if (pos + 1 >= f->size() || f->at(pos + 1) != 0) break;      // a marker, or a lone 0xFF at the end
                pos += 2;
            } else {
                ++pos;
            }
            acc |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    TRS_JPEG_HD uint32_t peek(int n) const { return (uint32_t)(acc >> (64 - n)); }     // n in 1..32
    TRS_JPEG_HD void skip(int n) { acc <<= n; cnt -= n; }                              // n in 0..32
};

// an extra-bits value v of s bits (s >= 1) -> the number it stands for
TRS_JPEG_HD int extend(int v, int s) { return v >= 1 << (s - 1) ? v : v - (1 << s) + 1; }

// the next symbol of table t, or -1: no code of the table, or one that runs past the end of the bits.  Leaves >= 16 bits filled where the file has
// them: the extra bits of the symbol (<= 11) need no refill.
template <class F>
TRS_JPEG_HD int decode_symbol(BitReader<F>& r, const HuffTable& t)
{
    r.fill();
    const int e = t.look[r.peek(kLookBits)];
    if (e) {
        r.skip(e >> 8);
        return r.cnt < 0 ? -1 : e & 255;
    }
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int c = (int)r.peek(l);
        if (c <= t.maxcode[l]) {
            const int idx = c + t.valoff[l];
            r.skip(l);
            return r.cnt < 0 || (unsigned)idx > 255u ? -1 : t.sym[idx];
        }
    }
    return -1;
}

// one block: coef[0..63] in NATURAL order (zero on entry) <- the coefficients, not yet dequantised; *pred: the component's DC predictor; zz: DecodeTables::zz.
// Returns kDecoded or kCorrupt.
template <class F>
TRS_JPEG_HD int decode_block(BitReader<F>& r, const HuffTable& dc, const HuffTable& ac, const uint8_t* zz, int* pred, int16_t* coef)
{
    int s = decode_symbol(r, dc);
    if (s < 0 || s > 11) return kCorrupt;
    if (s) {
        *pred += extend((int)r.peek(s), s);
        r.skip(s);
        if (r.cnt < 0) return kCorrupt;
    }
    coef[0] = (int16_t)*pred;
    int k = 1;
    while (k < 64) {
        const int rs = decode_symbol(r, ac);
        if (rs < 0) return kCorrupt;
        s = rs & 15;
        if (!s) {
            if (rs >> 4 != 15) return kDecoded;                           // EOB
            k += 16;                                                      // ZRL
            continue;
        }
        k += rs >> 4;
        if (k > 63 || s > 10) return kCorrupt;
        coef[zz[k]] = (int16_t)extend((int)r.peek(s), s);
        r.skip(s);
        if (r.cnt < 0) return kCorrupt;
        ++k;
    }
    return k > 64 ? kCorrupt : kDecoded;                                  // (a ZRL that runs beyond the block)
}

// ---- samples ---------------------------------------------------------------------------------------------------------------------------------
// One pass of the integer inverse DCT over d[0..7] in place; n = 11 for the first pass (columns), 18 for the second (rows).  The arithmetic wraps
// modulo 2^32 (coefficients no encoder writes must not be undefined behaviour); for files made from images nothing wraps.
TRS_JPEG_HD void idct_pass(int32_t d[8], int n)
{
    typedef uint32_t u;
    const u i0 = (u)d[0], i1 = (u)d[1], i2 = (u)d[2], i3 = (u)d[3], i4 = (u)d[4], i5 = (u)d[5], i6 = (u)d[6], i7 = (u)d[7];
    u z1 = (i2 + i6) * 4433u;
    const u t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u, t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (u)-7373; z2 *= (u)-20995; z3 = z3 * (u)-16069 + z5; z4 = z4 * (u)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const u half = 1u << (n - 1);
    d[0] = (int32_t)(t10 + a3 + half) >> n; d[7] = (int32_t)(t10 - a3 + half) >> n;
    d[1] = (int32_t)(t11 + a2 + half) >> n; d[6] = (int32_t)(t11 - a2 + half) >> n;
    d[2] = (int32_t)(t12 + a1 + half) >> n; d[5] = (int32_t)(t12 - a1 + half) >> n;
    d[3] = (int32_t)(t13 + a0 + half) >> n; d[4] = (int32_t)(t13 - a0 + half) >> n;
}
TRS_JPEG_HD int sample_of(int32_t x) { return x < -128 ? 0 : x > 127 ? 255 : x + 128; }

// the 2 x 2 triangle filter on the ceil(H / 2) x ceil(W / 2) real chroma samples
TRS_JPEG_HD int chroma_cols(int W) { return (W + 1) / 2; }
// the chroma row next to row y's own (y >> 1): above for the upper image row of a pair, below for the lower; the plane's first and last row stand in for what lies beyond them
TRS_JPEG_HD int chroma_nb_row(const Geometry& g, int y) { const int r = y >> 1; return (y & 1) ? (r + 1 < g.c_rows ? r + 1 : r) : (r > 0 ? r - 1 : 0); }
TRS_JPEG_HD int tri_v(int c, int nb) { return 3 * c + nb; }
// image column x from the vertical sums: s of its own chroma column x >> 1 and s_nb of the column to the left (x even) or right (x odd), which is
// that column itself in the first and the last column
TRS_JPEG_HD int chroma_nb_col(int W, int x) { const int j = x >> 1; return (x & 1) ? (j + 1 < chroma_cols(W) ? j + 1 : j) : (j > 0 ? j - 1 : 0); }
TRS_JPEG_HD int tri_h(int s, int s_nb, int x) { return (3 * s + s_nb + 8 - (x & 1)) >> 4; }
TRS_JPEG_HD int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// y, cb, cr in 0..255 -> R | G << 8 | B << 16
TRS_JPEG_HD uint32_t ycc_to_rgb(int y, int cb, int cr)
{
    cb -= 128; cr -= 128;
    const int r = y + ((fix16(1.402) * cr + 32768) >> 16);
    const int g = y + ((-fix16(0.34414) * cb + 32768 - fix16(0.71414) * cr) >> 16);
    const int b = y + ((fix16(1.772) * cb + 32768) >> 16);
    return (uint32_t)clamp255(r) | (uint32_t)clamp255(g) << 8 | (uint32_t)clamp255(b) << 16;
}

// the frame uint8[H][W][3] at dst from the sample planes: yp (rows ystride bytes apart), cb and cr (rows cstride apart; the ceil(H / 2) x ceil(W / 2) real samples are read)
inline void planes_to_frame(const Geometry& g, const uint8_t* yp, int ystride, const uint8_t* cb, const uint8_t* cr, int cstride, uint8_t* dst)
{
    for (int y = 0; y < g.H; ++y)
        for (int x = 0; x < g.W; ++x) {
            const size_t r0 = (size_t)(y >> 1) * cstride, r1 = (size_t)chroma_nb_row(g, y) * cstride;
            const int c0 = x >> 1, c1 = chroma_nb_col(g.W, x);
            const int b = tri_h(tri_v(cb[r0 + c0], cb[r1 + c0]), tri_v(cb[r0 + c1], cb[r1 + c1]), x);
            const int r = tri_h(tri_v(cr[r0 + c0], cr[r1 + c0]), tri_v(cr[r0 + c1], cr[r1 + c1]), x);
            const uint32_t rgb = ycc_to_rgb(yp[(size_t)y * ystride + x], b, r);
            uint8_t* o = dst + ((size_t)y * g.W + x) * 3;
            o[0] = (uint8_t)rgb; o[1] = (uint8_t)(rgb >> 8); o[2] = (uint8_t)(rgb >> 16);
        }
}

// ---- the kernel's LDS, per wave and per workgroup (csrc/trsim_jpeg_decode.hip lays it out in this order) -----------------------------------------
struct DecodeLds { int off_tab, off_win, off_coef, off_ws, off_y, off_c, wave_bytes, total; };
TRS_JPEG_HD DecodeLds decode_lds(int W)
{
    const int mw = (W + 15) / 16;
    DecodeLds l;
    l.off_tab = 0;
    l.off_win = (int)((sizeof(DecodeTables) + 15) & ~(size_t)15);
    l.off_coef = l.off_win + kWindowBytes;
    l.off_ws = l.off_coef + kMcuGroup * kBlocksPerMcu * kDecCoefStride * 2;
    l.off_y = l.off_ws + 8 * kWsBlockStride * 4;
    l.off_c = l.off_y + 2 * 256 * mw;                  // Y samples of two MCU rows: the one being written and the one being output
    l.wave_bytes = l.off_c + kChromaRing * 128 * mw;   // Cb | Cr samples of kChromaRing MCU rows
    l.total = kDecodeWaves * l.wave_bytes;
    return l;
}
// the widest image a workgroup with lds_bytes of LDS decodes (0: none)
inline int decode_max_width(int lds_bytes)
{
    int mw = 0;
    while (decode_lds(16 * (mw + 1)).total <= lds_bytes && mw < 4095) ++mw;
    return 16 * mw;
}

}  // namespace jpeg
}  // namespace trsim
