// trsim_jpeg_codec.hpp — the camera codec (include/trsim_spec.h, "camera codec (JPEG round trip)"): codec(frame, q) = decode(encode(frame, q)) without
// the entropy stage between the quantiser and the dequantiser.  Every rule is a function of trsim_jpeg_tables.hpp (colour, edges, downsampling, forward
// DCT, quantiser) or of trsim_jpeg_decode.hpp (inverse DCT, clamp, triangle upsampling, colour back); what is new here is their composition over one
// block, a whole frame on the host as sample_planes, the blocks, planes_to_frame (tests/jpeg_codec_driver.cpp drives it under the sanitizers) and the
// LDS plan of trs_jpeg_codec_kernel (csrc/trsim_jpeg_codec.hip), which takes the block steps from here and its first and last stage from
// trsim_jpeg_device.hpp (sample_stripe, output_mcu_row).
#pragma once
#include <cstdint>
#include <vector>

#include "trsim_jpeg_decode.hpp"
#include "trsim_jpeg_tables.hpp"

namespace trsim {
namespace jpeg {

constexpr int kCodecThreads = 256;           // threads of a workgroup of trs_jpeg_codec_kernel: every wave transforms 8 blocks at a time, a lane per block row or column
constexpr int kCodecWgsPerCu = 4;            // the kernel runs min(frames, kCodecWgsPerCu x CU count) workgroups, each looping over frames

// ---- the round trip of one block, in the three steps between which a block changes from rows to columns and back -------------------------------
// d[0..7]: the samples (0..255) of one block row -> that row after the first pass of the forward DCT
TRS_JPEG_HD void codec_row_in(int32_t d[8])
{
    for (int j = 0; j < 8; ++j) d[j] -= 128;
    fdct_pass<true>(d);
}
// d[0..7]: column c of the block after codec_row_in of its 8 rows -> the column's coefficients, quantised with the steps qv[r * 8 + c] (each << 3, natural
// order), handed straight to the dequantiser (times the step) and through the first pass of the inverse DCT
TRS_JPEG_HD void codec_column(int32_t d[8], const int32_t* qv, int c)
{
    fdct_pass<false>(d);
    for (int r = 0; r < 8; ++r) d[r] = quantise(d[r], qv[r * 8 + c]) * (qv[r * 8 + c] >> 3);
    idct_pass(d, 11);
}
// d[0..7]: one row of the block after codec_column of its 8 columns -> the row's samples (0..255)
TRS_JPEG_HD void codec_row_out(int32_t d[8])
{
    idct_pass(d, 18);
    for (int j = 0; j < 8; ++j) d[j] = sample_of(d[j]);
}
// the 8 x 8 samples at `in` (rows in_stride bytes apart) -> `out`; qv: the 64 quantisation steps << 3 of the block's component
inline void codec_block(const uint8_t* in, int in_stride, const int32_t* qv, uint8_t* out, int out_stride)
{
    int32_t w[64], d[8];
    for (int r = 0; r < 8; ++r) {
        for (int c = 0; c < 8; ++c) d[c] = in[r * in_stride + c];
        codec_row_in(d);
        for (int c = 0; c < 8; ++c) w[r * 8 + c] = d[c];
    }
    for (int c = 0; c < 8; ++c) {
        for (int r = 0; r < 8; ++r) d[r] = w[r * 8 + c];
        codec_column(d, qv, c);
        for (int r = 0; r < 8; ++r) w[r * 8 + c] = d[r];
    }
    for (int r = 0; r < 8; ++r) {
        for (int c = 0; c < 8; ++c) d[c] = w[r * 8 + c];
        codec_row_out(d);
        for (int c = 0; c < 8; ++c) out[r * out_stride + c] = (uint8_t)d[c];
    }
}

// the triangle filter needs a chroma plane of more than two columns, as the decoder does (parse_header)
TRS_JPEG_HD bool codec_size_ok(int H, int W) { return H >= 1 && W > 4; }

// codec(frame, quality) of one uint8[H][W][3] frame on the host: plain loops over whole planes; dst must not overlap src.  false: the size is refused
inline bool codec_frame(int H, int W, int quality, const uint8_t* src, uint8_t* dst)
{
    if (!codec_size_ok(H, W) || quality < 1 || quality > 100) return false;
    const Geometry g = geometry(H, W);
    const int ys = 16 * g.mcu_cols, cs = 8 * g.mcu_cols, yr = 16 * g.mcu_rows, cr = 8 * g.mcu_rows;
    int32_t qv[2][64];
    quant_steps(quality, qv);
    std::vector<uint8_t> yp((size_t)yr * ys), cp[2], yo((size_t)yr * ys), co[2];
    for (int p = 0; p < 2; ++p) { cp[p].resize((size_t)cr * cs); co[p].resize((size_t)cr * cs); }
    sample_planes(g, src, yp.data(), cp[0].data(), cp[1].data());
    for (int my = 0; my < g.mcu_rows; ++my)
        for (int mx = 0; mx < g.mcu_cols; ++mx) {
            for (int k = 0; k < 4; ++k) {
                if (y_dummy(g, my, mx, k)) continue;                              // a dummy block holds no image sample: it is never output
                const size_t at = (size_t)(16 * my + 8 * (k >> 1)) * ys + 16 * mx + 8 * (k & 1);
                codec_block(&yp[at], ys, qv[0], &yo[at], ys);
            }
            const size_t at = (size_t)8 * my * cs + 8 * mx;
            for (int p = 0; p < 2; ++p) codec_block(&cp[p][at], cs, qv[1], &co[p][at], cs);
        }
    planes_to_frame(g, yo.data(), ys, co[0].data(), co[1].data(), cs, dst);
    return true;
}

// ---- the kernel's LDS (csrc/trsim_jpeg_codec.hip lays it out in this order), per MCU column: the 16 raw RGB rows of a stripe, its sample planes
// (16 x 16 Y + 2 x 8 x 8 chroma), the Y samples of two MCU rows after the round trip (the one being written and the one being output) and the chroma
// samples of kChromaRing; per wave: the 8 x 8 int32 intermediates of 8 blocks (kWsRowStride / kWsBlockStride: conflict-free by row and by column)
struct CodecLds { int off_q, off_raw, off_y, off_c, off_ws, off_yout, off_cring, total; };
TRS_JPEG_HD CodecLds codec_lds(int W)
{
    const int mw = (W + 15) / 16;
    CodecLds l;
    l.off_q = 0;
    l.off_raw = 128 * 4;
    l.off_y = l.off_raw + ((16 * W * 3 + 15) & ~15);
    l.off_c = l.off_y + 256 * mw;
    l.off_ws = l.off_c + 128 * mw;
    l.off_yout = l.off_ws + (kCodecThreads / 64) * 8 * kWsBlockStride * 4;
    l.off_cring = l.off_yout + 2 * 256 * mw;
    l.total = l.off_cring + kChromaRing * 128 * mw;
    return l;
}
// the widest image a workgroup with lds_bytes of LDS takes (0: none)
inline int codec_max_width(int lds_bytes)
{
    int mw = 0;
    while (codec_lds(16 * (mw + 1)).total <= lds_bytes && mw < 4095) ++mw;
    return 16 * mw;
}

}  // namespace jpeg
}  // namespace trsim
