// trsim_train_dev.hpp — the device-side pieces the two training units share (trsim_train.hip: the tail, trsim_train_conv.hip: conv4 .. conv7): the vector
// types, Adam's constants and update in Keras's form, the binary16 rounding of a packed weight, the small rules of a scaled gradient (2^e, the wave's largest
// bit pattern, the gated store) and the GEMM that reduces over the slow index of both operands: its transposed LDS fragment read and its staged chunk loop.
// HIP only; the rules a host compiler can check are trsim_train.hpp and trsim_train_conv.hpp.
#pragma once
#include <hip/hip_runtime.h>

namespace trsim_train_dev {

typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 h16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));

// Adam's constants as a kernel parameter: beta1, 1 - beta1, beta2, 1 - beta2, epsilon, alpha_t of the step
struct AdamK { float b1, c1, b2, c2, eps, alpha; };

constexpr int kGwFrames = 64;              // rows (frames, or pixels) per LDS chunk: four k-steps of 16
constexpr int kGwPitch = 320;              // bytes per row of a tile: 128 values and 64 B that keep the transposed reads off each other's banks
constexpr int kGwTile = kGwFrames * kGwPitch;

typedef short s16x4 __attribute__((__vector_size__(8)));                   // the builtin's own vector type
typedef __attribute__((address_space(3))) s16x4* lds_s16x4p;

// the fragment of a 32 x 32 x 16 MFMA whose 32-wide index is `col0 .. col0 + 31` of the tile's rows and whose k index is frames k0 .. k0 + 15: lane l holds
// column col0 + l % 32, frames k0 + 8 (l / 32) .. + 7.  Per 16-lane group two transposed reads of a 4-frame x 16-column block each: lane 4 q + p of the
// group points at frame q, columns 4 p .. 4 p + 3 of its block, and receives its own column of the four frames.
__device__ __forceinline__ h16x8 tr_fragment(const unsigned char* tile, int lane, int col0, int k0)
{
    const int i16 = lane & 15, row = k0 + 8 * (lane >> 5) + (i16 >> 2), col = col0 + 16 * ((lane >> 4) & 1) + 4 * (i16 & 3);
    const unsigned char* a = tile + row * kGwPitch + col * 2;
    const h16x4 lo = __builtin_bit_cast(h16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4p)(a)));
    const h16x4 hi = __builtin_bit_cast(h16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4p)(a + 4 * kGwPitch)));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The chunk loop of that GEMM, D[q column][x column] += sum over rows first .. end - 1 of q[row][.] x[row][.], for a workgroup of 256 threads: 64 rows of both
// operands per chunk, [row][value] as they lie in memory, x's tile at `tiles` and q's behind it.  A row of x holds 4 XI granules of 8 values and thread t
// stages granules t + 256 i (i < XI) of a chunk, row e / (4 XI), granule e % (4 XI); q likewise with QI.  load_x and load_q, (row, granule) -> u4v, do the
// caller's addressing and give zeros past the operand's end.  The next chunk's loads are requested while this one's MFMAs run.  Of a chunk only the k-steps
// of 16 rows that hold one of the `rows` rows of the batch are multiplied.  The wave owns x's 32-column block `xb` against q's blocks qb0 .. qb0 + PER - 1:
// the caller zeroes acc[b], element by element where it declares them (zeroed through a reference the compiler kept them out of the accumulation registers
// between chunks).  per_chunk(steps) runs once per chunk while the tiles hold it (the weight gradient's bias sums).
template <int XI, int QI, int PER, class Row, class LoadX, class LoadQ, class PerChunk>
__device__ __forceinline__ void tr_gemm_chunks(unsigned char* tiles, Row first, Row end, Row rows, int xb, int qb0, f32x16 (&acc)[PER],
                                               LoadX load_x, LoadQ load_q, PerChunk per_chunk)
{
    constexpr int XG = 4 * XI, QG = 4 * QI;
    const int tid = threadIdx.x, lane = tid & 63;
    u4v rx[XI], rq[QI];
    auto load = [&](Row c0) {
#pragma unroll
        for (int i = 0; i < XI; ++i) { const int e = tid + 256 * i; rx[i] = load_x(c0 + e / XG, e % XG); }
#pragma unroll
        for (int i = 0; i < QI; ++i) { const int e = tid + 256 * i; rq[i] = load_q(c0 + e / QG, e % QG); }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < XI; ++i) { const int e = tid + 256 * i; *reinterpret_cast<u4v*>(tiles + (e / XG) * kGwPitch + (e % XG) * 16) = rx[i]; }
#pragma unroll
        for (int i = 0; i < QI; ++i) { const int e = tid + 256 * i; *reinterpret_cast<u4v*>(tiles + kGwTile + (e / QG) * kGwPitch + (e % QG) * 16) = rq[i]; }
    };
    load(first);
    for (Row c0 = first; c0 < end; c0 += kGwFrames) {
        __syncthreads();                                                            // the chunk before has been read
        store();
        __syncthreads();
        if (c0 + kGwFrames < end) load(c0 + kGwFrames);                             // the next chunk is requested underneath
        const int steps = (int)min((Row)4, (rows - c0 + 15) >> 4);
        per_chunk(steps);
        for (int ks = 0; ks < steps; ++ks) {
            const h16x8 bx = tr_fragment(tiles, lane, 32 * xb, 16 * ks);
#pragma unroll
            for (int b = 0; b < PER; ++b) {
                const h16x8 aq = tr_fragment(tiles + kGwTile, lane, 32 * (qb0 + b), 16 * ks);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq, bx, acc[b], 0, 0, 0);
            }
        }
    }
}

// 2^e as a binary32 for |e| <= 126 (train_pow2 on the host): a scale and its inverse are exact
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }
// The wave's largest bit pattern into *dst.  Non-negative binary32 values order like their patterns, and an integer maximum has no order.
__device__ __forceinline__ void wave_max_bits(unsigned mx, unsigned* dst, int lane)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off, 64));
    if (lane == 0 && mx) atomicMax(dst, mx);
}
// how a data gradient leaves its kernel: G[at] = [x[at] > 0] . acc 2^-s, folded into the lane's largest |G| bit pattern
__device__ __forceinline__ void gated_store(float* G, const unsigned short* x, size_t at, float acc, float back, unsigned& mx)
{
    const float g = (float)__builtin_bit_cast(_Float16, x[at]) > 0.0f ? acc * back : 0.0f;
    G[at] = g;
    mx = max(mx, __float_as_uint(g) & 0x7FFFFFFFu);
}

// plain binary32, every operation rounded by itself (the build has no contraction; sqrt and / are correctly rounded)
__device__ __forceinline__ float adam(float g, float& m, float& v, float w, const AdamK& k)
{
    m = k.b1 * m + k.c1 * g;
    v = k.b2 * v + k.c2 * (g * g);
    return w - (k.alpha * m) / (sqrtf(v) + k.eps);
}

// binary32 -> binary16 as host_f2h packs the weights (trsim_pilot_plan.hpp): nearest even, 65504 beyond the range, NaN stays NaN
__device__ __forceinline__ unsigned short f2h_pack(float f)
{
    const unsigned x = __float_as_uint(f), a = x & 0x7FFFFFFFu;
    if (a >= 0x477FE000u && a <= 0x7F800000u) return (unsigned short)(((x >> 16) & 0x8000u) | 0x7BFFu);
    return __builtin_bit_cast(unsigned short, (_Float16)f);
}

}  // namespace trsim_train_dev
