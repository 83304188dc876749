// trsim_train_dev.hpp — the device-side pieces the two training units share (trsim_train.hip: the tail, trsim_train_conv.hip: conv4 .. conv7): the vector
// types, the transposed LDS fragment read of a GEMM that reduces over the slow index of both operands, Adam's update in Keras's form and the binary16
// rounding of a packed weight.  HIP only; the rules a host compiler can check are trsim_train.hpp and trsim_train_conv.hpp.
#pragma once
#include <hip/hip_runtime.h>

// Adam's constants as a kernel parameter: beta1, 1 - beta1, beta2, 1 - beta2, epsilon, alpha_t.  The one definition, in an unnamed namespace on purpose: a
// kernel's symbol carries its parameter types, and trs_train_adam1_kernel / trs_train_adam_kernel keep the symbols they had while this struct was
// trsim_train.hip's own (scripts/kernel_diff.py matches kernels by symbol).
namespace {
struct AdamK { float b1, c1, b2, c2, eps, alpha; };
}

namespace trsim_train_dev {

typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 h16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));

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
