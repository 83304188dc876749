// trsim_jpeg_device.hpp — the data movement the JPEG kernels share (device only: included by trsim_jpeg.hip, trsim_jpeg_decode.hip and
// trsim_jpeg_codec.hip): a frame's raw rows to the sample planes of an MCU row (sample_stripe: the encoder and the camera codec), where the samples of a
// transformed block row land and are read again (SampleBuffers: the decoder and the codec), and those samples to the frame's rows (output_mcu_row: the
// same two).  Every rule it applies is a function of trsim_jpeg_tables.hpp or trsim_jpeg_decode.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "trsim_jpeg_decode.hpp"

namespace trsim {
namespace jpeg {

// what one lane of the wave wrote to LDS is visible to the others behind this
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// MCU row my of the frame at src (4-byte aligned, W % 4 == 0) -> its sample planes ys[16][16 mw] and cs[Cb | Cr][8][8 mw], by the THREADS threads of a
// workgroup: the image rows go to raw4 as they lie in memory, then one 2 x 2 quad of the padded planes per thread and turn.  Ends behind a barrier.
template <int THREADS>
__device__ inline void sample_stripe(const Geometry& g, int my, const uint8_t* src, uint32_t* raw4, uint8_t* ys, uint8_t* cs)
{
    const int tid = threadIdx.x, ystride = 16 * g.mcu_cols, cstride = 8 * g.mcu_cols, row_bytes = g.W * 3, r_lo = 16 * my, nrows = min(16, g.H - r_lo);
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + (size_t)r_lo * row_bytes);
    for (int i = tid; i < nrows * (row_bytes / 4); i += THREADS) raw4[i] = s4[i];
    __syncthreads();
    const uint8_t* raw = reinterpret_cast<const uint8_t*>(raw4);
    for (int q = tid; q < 8 * cstride; q += THREADS) {
        const int qr = q / cstride, qc = q - qr * cstride;
        const QuadSamples s = sample_quad(g, 8 * my + qr, qc, [&](int r, int c) { return raw + (r - r_lo) * row_bytes + c * 3; });
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) ys[(2 * qr + dy) * ystride + 2 * qc + dx] = s.y[dy][dx];
        cs[qr * cstride + qc] = s.cb;
        cs[(8 + qr) * cstride + qc] = s.cr;
    }
    __syncthreads();
}

// The samples behind the inverse transform, kept until the output that trails it by one MCU row has read them: yout[2][16][16 mw], the Y rows of MCU
// row my in half my & 1, and cring[kChromaRing][Cb | Cr][8][8 mw], the chroma rows of MCU row my in slot my % kChromaRing.  Both 4-byte aligned.
// (__forceinline__: left to itself the compiler calls store_block_row out of line in the decoder, with this struct handed over through scratch memory)
struct SampleBuffers {
    uint8_t* yout; uint8_t* cring; int mw;
    __device__ __forceinline__ uint8_t* y_row(int my, int r) const { return yout + ((my & 1) * 16 + r) * 16 * mw; }                                     // r: 0..15, row of the MCU row
    __device__ __forceinline__ uint8_t* c_row(int plane, int r) const { return cring + ((((r >> 3) % kChromaRing) * 2 + plane) * 8 + (r & 7)) * 8 * mw; }   // r: row of the whole plane
    // row j of block k (Y00 Y01 Y10 Y11 Cb Cr) of MCU (my, mx): its samples 0..3 in lo4 and 4..7 in hi4, the first in the low byte
    __device__ __forceinline__ void store_block_row(int my, int mx, int k, int j, uint32_t lo4, uint32_t hi4) const
    {
        uint32_t* out = reinterpret_cast<uint32_t*>(k < 4 ? y_row(my, 8 * (k >> 1) + j) + 16 * mx + 8 * (k & 1) : c_row(k - 4, 8 * my + j) + 8 * mx);
        out[0] = lo4;
        out[1] = hi4;
    }
};

// image rows [16 my, 16 my + 16) of the frame at dst from the Y samples of MCU row my and the chroma ring: 4 pixels per turn of each of the STRIDE
// threads that call it (t0: the caller's index among them).  dwords: dst is 4-byte aligned and W % 4 == 0, a unit is three dword stores; otherwise
// bytes, and the last unit of a row ends at W.  Y is read a dword at a time whatever W is: x0 + 3 < 16 mw, a multiple of 4 that is not below W.
template <int STRIDE>
__device__ inline void output_mcu_row(const Geometry& g, int my, const SampleBuffers& sb, uint8_t* dst, int t0, bool dwords)
{
    const int units = (g.W + 3) >> 2, rows = min(16, g.H - 16 * my);
    for (int t = t0; t < rows * units; t += STRIDE) {
        const int ry = t / units, u = t - ry * units, y = 16 * my + ry, x0 = 4 * u;
        const int r0 = y >> 1, r1 = chroma_nb_row(g, y);
        // the vertical sums of the chroma columns 2u - 1 .. 2u + 2 (clamped to the plane), both planes
        int s[2][4];
        for (int pl = 0; pl < 2; ++pl) {
            const uint8_t* a = sb.c_row(pl, r0);
            const uint8_t* b = sb.c_row(pl, r1);
            for (int j = 0; j < 4; ++j) {
                const int c = min(max(2 * u - 1 + j, 0), chroma_cols(g.W) - 1);
                s[pl][j] = tri_v(a[c], b[c]);
            }
        }
        const uint32_t y4 = *reinterpret_cast<const uint32_t*>(sb.y_row(my, ry) + x0);
        uint32_t px[4];
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k, own = 1 + (k >> 1), nb = (k & 1) ? own + 1 : own - 1;      // (s[][0] and s[][3] are the clamped neighbours)
            px[k] = ycc_to_rgb((int)((y4 >> (8 * k)) & 255u), tri_h(s[0][own], s[0][nb], x), tri_h(s[1][own], s[1][nb], x));
        }
        uint8_t* o = dst + ((size_t)y * g.W + x0) * 3;
        if (dwords) {
            uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
            o4[0] = px[0] | px[1] << 24;
            o4[1] = px[1] >> 8 | px[2] << 16;
            o4[2] = px[2] >> 16 | px[3] << 8;
        } else {
            for (int k = 0; k < 4 && x0 + k < g.W; ++k) {
                o[3 * k] = (uint8_t)px[k]; o[3 * k + 1] = (uint8_t)(px[k] >> 8); o[3 * k + 2] = (uint8_t)(px[k] >> 16);
            }
        }
    }
}

}  // namespace jpeg
}  // namespace trsim
