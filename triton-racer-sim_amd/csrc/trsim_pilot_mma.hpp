// trsim_pilot_mma.hpp — the fragment-level pieces of the pilot's convolution kernels (included by trsim_pilot.hip inside its anonymous namespace, ahead of
// trsim_pilot_layers.hpp): the vector types, the binary16 conversions and the packed ReLU, the epilogue block of a 32 x 32 accumulator (block_groups), the
// accumulators' start at the bias (acc_from_bias), the K loop over a register ring of weights (ring_k_loop), and what the frame kernel and the chain share
// of a 3x3 layer whose input image lies XOR-swizzled in LDS: its staging (stage_run) and its wave item (conv3x3_item).
#pragma once

typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;   // 8 binary16 values: one MFMA operand fragment per lane (round 3: binary16 instead of bfloat16 —
                                                              // the same MFMA rate, 3 more mantissa bits: max |output - fp32| 5e-4 -> 4e-5, profiles/r03_pilot_precision.txt)
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(3))) u4v* lds_u4vp;   // an LDS address held as an integer: no "+ psmem" per access

__device__ __forceinline__ unsigned short f2h(float f)
{   // round to nearest even; beyond binary16's range: 65504 (the activations saturate, they never become infinite)
    const _Float16 h = (_Float16)__builtin_fminf(__builtin_fmaxf(f, -65504.0f), 65504.0f);
    return __builtin_bit_cast(unsigned short, h);
}

typedef __attribute__((ext_vector_type(2))) _Float16 h16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;

__device__ __forceinline__ unsigned pack_h16x2(float lo, float hi)
{   // round to nearest even, two values per dword: v_cvt_pk_f16_f32 on gfx950 (beyond 65504: +-infinity; the ReLU form below saturates)
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, h16x2));
}

// two uint8 values (already binary32, 0..255: exact in binary16 under any rounding) as a binary16 pair: v_cvt_pkrtz_f16_f32
__device__ __forceinline__ unsigned u8pair_h16(float f0, float f1) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(f0, f1)); }

typedef short s16x2 __attribute__((ext_vector_type(2)));
// ReLU on two packed binary16: the sign bit is the int16's, so max(., 0) as int16 zeroes the negatives (and -0).  One v_pk_max_i16
// for two values instead of a v_max_f32 each in front of the conversion; round-to-nearest keeps the sign, so the bits are the same.
// Non-negative binary16 values order like their int16 patterns, so min(., 0x7BFF) turns an overflowed +infinity (0x7C00) into 65504:
// activations saturate instead of poisoning the next layer (one more v_pk_min_i16 per pair).
// (The epilogues are vector-ALU work between short MFMA runs: conv1's tile of 5 MFMAs carried ~65 VALU instructions.)
__device__ __forceinline__ unsigned relu_h16x2(unsigned packed)
{
    const s16x2 v = __builtin_bit_cast(s16x2, packed), z = {0, 0}, top = {0x7BFF, 0x7BFF};
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_elementwise_max(v, z), top));
}
__device__ __forceinline__ uint2 relu_pack4(float v0, float v1, float v2, float v3)
{
    return make_uint2(relu_h16x2(pack_h16x2(v0, v1)), relu_h16x2(pack_h16x2(v2, v3)));
}
// ... without the saturation, for sums that provably stay inside binary16 (conv1 of the fused head: |bias| + sum |w| < 65504 is checked when the weights
// are loaded — its inputs are pixels / 256 <= 1)
__device__ __forceinline__ uint2 relu_pack4_bounded(float v0, float v1, float v2, float v3)
{
    const s16x2 z = {0, 0};
    return make_uint2(__builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, pack_h16x2(v0, v1)), z)),
                      __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, pack_h16x2(v2, v3)), z)));
}

// The epilogues' half exchange.  Register quad q of a 32x32 accumulator block holds channels 8q + 4h .. + 3 of pixel r in lane (r, h): the two lanes of a
// pixel hold the two halves of every 8-channel group.  So that each lane stores whole 16-byte groups — lane h = 0 groups 0 and 1, lane h = 1 groups 2
// and 3 — lane h = 0 needs its partner's half of groups 0, 1 and lane h = 1 its partner's half of groups 2, 3.  v_permlane32_swap_b32 a, b exchanges
// the upper 32 lanes of a with the lower 32 lanes of b (gfx950): with a = a word of group q and b = the same word of group q + 2, BOTH halves of the wave
// end with (own half, partner's half) of the group they store, in (a, b) order — one full-rate VALU instruction per word where rounds 2-3 used a select,
// a ds_bpermute through the LDS crossbar and two more selects (round 4; the same bytes in the same places).
__device__ __forceinline__ void half_swap(unsigned& a, unsigned& b)
{
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0]; b = r[1];
}
__device__ __forceinline__ void quad_groups(const uint2 (&w)[4], u4v& g0, u4v& g1)
{
    unsigned a0 = w[0].x, a1 = w[0].y, b0 = w[2].x, b1 = w[2].y, c0 = w[1].x, c1 = w[1].y, d0 = w[3].x, d1 = w[3].y;
    half_swap(a0, b0); half_swap(a1, b1); half_swap(c0, d0); half_swap(c1, d1);
    g0 = u4v{a0, a1, b0, b1};                               // h = 0: channels 0..7 of group 0; h = 1: channels 0..7 of group 2
    g1 = u4v{c0, c1, d0, d1};                               // h = 0: group 1; h = 1: group 3
}
// The epilogue of one 32 x 32 accumulator block whose sums started at the bias: ReLU + fp16, then the half exchange.  The lane ends with the two whole
// 16-byte groups it stores: channels 16 h .. + 7 of the block in g0, 16 h + 8 .. + 15 in g1 (of pixel r).  No LDS: until round 4 a tile went through a
// wave-private LDS stage — four broadcast bias reads and the transpose, six dependent round trips of ~200 clocks (profiles/r04_pilot_head_stamps.txt).
__device__ __forceinline__ void block_groups(const f32x16& a, u4v& g0, u4v& g1)
{
    uint2 w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = relu_pack4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    quad_groups(w, g0, g1);
}
// The accumulators of a wave item start at the layer's bias (the MFMA's C operand adds it) instead of at zero with 16 v_add per 32 x 32 block in
// the epilogue: register 4 q + j of block nb = channel cbase + nb*32 + 8 q + 4 h + j.  (fp32 sum order: bias first — the same fp16 activations up to
// the last bit of the fp32 sum; tests/test_pilot.py compares against the PyTorch mirror.)
template <int NT, int NB>
__device__ __forceinline__ void acc_from_bias(f32x16 (&acc)[NT][NB], const float4* lbias, int cbase, int h)
{
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 b = lbias[(cbase + nb * 32 + 8 * q + 4 * h) >> 2];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { acc[nt][nb][4 * q] = b.x; acc[nt][nb][4 * q + 1] = b.y; acc[nt][nb][4 * q + 2] = b.z; acc[nt][nb][4 * q + 3] = b.w; }
        }
}

// ---- the K loop of a wave item: NT x 32 pixels x NB x 32 output channels over KSTEPS k-steps of 16 input channels ----------------
// (trs_conv_frame_kernel and the chain through conv3x3_item, trs_conv_frame5_kernel with its own lambdas.)
//   wload(nb)     the weight granule of the current k-step for block nb, by buffer load: one lane offset + ONE scalar that runs with the loads (a 64-bit
//                 address per ring slot cost ~60-80 registers; a constant per (k-step, block), 144 of them at 128 input channels, was hoisted out of the item
//                 loop and spilled to vector-register lanes: a v_readlane + wait states in front of every load; the block is the immediate offset)
//   wnext()       ... advances that scalar by one k-step: the loads are issued in k order
//   pixels(k, x)  the NT pixel fragments of k-step k from LDS (k is a compile-time constant after unrolling)
// Weight prefetch: a register ring of R k-steps (R x NB granules per lane), refilled slot by slot right behind the MFMAs that consumed the slot:
// R x NT x NB x 32 MFMA clocks of lead time against an L2 round trip of 500-800 (R = 4: one tap at 64 input channels, half a tap at 128; rings of 6 and 8
// measured no faster).
// All KSTEPS k-steps are unrolled (3 x 12 or 9 x 8 ...): ONE basic block, no back edge — the compiler counts the weight loads in flight exactly (vmcnt(N)
// per k-step) instead of draining the queue at a loop head or behind a branch.  The pixel fragments are software-pipelined by hand: k-step k + 1's
// ds_reads are issued BEFORE k-step k's MFMAs (the sched_barrier that keeps "MFMAs of k, then the refill of k's ring slot" in place would otherwise also
// pin each k-step's LDS reads right in front of its own MFMAs: one LDS latency per 4 MFMAs).
// (Round 4: a second sched_barrier between those reads and the MFMAs — hipcc sinks the reads behind three of a k-step's four MFMAs — was measured in the
// frame kernels, the chain and frame5: all slower, chain 46.2 -> 48.4 us, conv7 96.1 -> 100.5: the address arithmetic then runs as a burst with no MFMA
// beside it.)
// (Round 4, profiles/r04_mfma_issue.txt: inside a wave every vector-ALU instruction between two MFMAs ADDS ~6 ticks to the MFMA's 32, and two waves per
// SIMD hide only part of each other's — a K loop is priced by its non-MFMA instructions per MFMA.  So the three `pixels` compute the XOR-swizzled LDS
// address of a tap's fragment ONCE per tap: the granule of k-step j of the tap is 2 j + h, and (2 j + h) ^ swizzle = (h ^ swizzle) ^ 2 j — the tap's byte
// address ^ 32 j, one v_xor per k-step and tile.)
// ABL: the timing-only diagnostic builds, never shipped (TRS_FRAME_ABLATE, TRS_CHAIN_ABLATE): 1 = no weight refills, 3 = no MFMA.
template <int KSTEPS, int R, int ABL, int NT, int NB, typename WLoad, typename WNext, typename Pixels>
__device__ __forceinline__ void ring_k_loop(f32x16 (&acc)[NT][NB], const float4* lbias, int cbase, int h, WLoad wload, WNext wnext, Pixels pixels)
{
    static_assert(R >= 1 && R <= KSTEPS, "ring depth in k-steps");
    u4v ring[R][NB];
#pragma unroll
    for (int d = 0; d < R; ++d) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) ring[d][nb] = wload(nb);
        wnext();
    }
    acc_from_bias(acc, lbias, cbase, h);
    h16x8 xa[NT], xb[NT];
    pixels(0, xa);
#pragma unroll
    for (int k = 0; k < KSTEPS; ++k) {
        const int d = k % R;
        h16x8 (&xc)[NT] = (k & 1) ? xb : xa;
        h16x8 (&xn)[NT] = (k & 1) ? xa : xb;
        if (k + 1 < KSTEPS) pixels(k + 1, xn);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if constexpr (ABL == 3) asm volatile("" :: "v"(ring[d][nb]), "v"(xc[nt]));
                else acc[nt][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, ring[d][nb]), xc[nt], acc[nt][nb], 0, 0, 0);
            }
        if (k + R < KSTEPS && ABL != 1) {                                   // (compile-time) refill the slot with the k-step R ahead
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) ring[d][nb] = wload(nb);
            wnext();
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- a 3x3 stride-1 layer whose input image lies in LDS: what trs_conv_frame_kernel and the chain's layers share --------------------
// The image: pixel slot p holds the pixel's cg = 1 << cgs granules of 8 channels, granule g in slot g ^ frame_swz(p), so that the 16 lanes of a
// ds_read_b128 group — 16 consecutive pixels, one logical granule — cover all 64 banks.
__device__ __forceinline__ int frame_swz(int pix, int cgs) { return cgs == 3 ? ((pix >> 1) & 7) : (pix & 15); }

// Staging by LDS-DMA (1 KB per wave instruction) of a run of `total` granules that is contiguous in memory from `src` on — whole pixels of whole rows —
// into the image slots from byte address dst on, by the wave with index wv among nw.  pix0 = the image's pixel slot of the run's first pixel (the
// swizzle follows the slot, as the readers compute it).  The XOR swizzle goes on the SOURCE address, the LDS side stays lane-linear: a slot's source is
// slot ^ swizzle — a shift, a mask and an XOR per DMA instruction (the general (unit, row, column) split of rounds 2-3 cost ~80 instructions per 1 KB:
// four loader waves then needed as long for a group as eight compute waves for its MFMAs).  Granules behind `last` are not in the activation: their
// addresses are clamped into it (the rows a last band asks for below its frame, never read by a valid pixel).
__device__ __forceinline__ void stage_run(const u4v* src, int total, int last, int pix0, int cgs, unsigned dst, int wv, int nw, int lane)
{
    for (int s0 = wv * 64; s0 < total; s0 += nw * 64) {
        const int sl = s0 + lane;
        if (sl < total) {
            const int pix = pix0 + (sl >> cgs), q = sl & ((1 << cgs) - 1);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + min((sl - q) + (q ^ frame_swz(pix, cgs)), last)),
                                             (__attribute__((address_space(3))) void*)(uintptr_t)(dst + s0 * 16), 16, 0, 0);
        }
    }
}

// One wave item: acc = bias + the 9 x HALF k-steps of NT x 32 windows x NB x 32 output channels from cbase on.  lds_b = LDS byte address of the image, IW its
// row length in pixels, lbase[nt] = the pixel slot of this lane's window nt; rw = the layer's weights [9 taps x cg granules][cpitch] as a buffer resource:
// granule (2 k + h, cout cbase + nb*32 + r) of k-step k.  HALF = k-steps per tap (8 granules per input pixel <-> 4, 16 <-> 8: the host builds the layers
// so).  ABL as in ring_k_loop, and 2 = one LDS pixel read per item.
template <int HALF, int R, int ABL, int NT, int NB>
__device__ __forceinline__ void conv3x3_item(f32x16 (&acc)[NT][NB], unsigned lds_b, int IW, const __amdgpu_buffer_rsrc_t rw, int cpitch, const float4* lbias, int cbase,
                                             const int (&lbase)[NT], int r, int h)
{
    constexpr int CGS = HALF == 4 ? 3 : 4;
    const int wvoff = (h * cpitch + cbase + r) * 16;
    int wso = 0;
    auto wload = [&](int nb) { return __builtin_bit_cast(u4v, __builtin_amdgcn_raw_buffer_load_b128(rw, wvoff + nb * 512, wso, 0)); };
    auto wnext = [&]() { wso += 2 * cpitch * 16; asm volatile("" : "+s"(wso)); };
    [[maybe_unused]] h16x8 xkeep[NT];
    unsigned tapb[NT];                                                      // LDS byte address of this lane's granule h ^ swizzle of the current tap's pixel
    auto pixels = [&](int k, h16x8 (&x)[NT]) {
        const int tap = k / HALF, j = k % HALF;
        const int tap_off = (tap / 3) * IW + tap % 3;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (j == 0) {
                const int pix = lbase[nt] + tap_off;
                tapb[nt] = lds_b + (unsigned)(((pix << CGS) + (h ^ frame_swz(pix, CGS))) << 4);
            }
            x[nt] = __builtin_bit_cast(h16x8, *(lds_u4vp)(uintptr_t)(tapb[nt] ^ (unsigned)(32 * j)));
            if constexpr (ABL == 2) {
                if (k == 0) xkeep[nt] = x[nt];
                x[nt] = xkeep[nt];
            }
        }
    };
    ring_k_loop<9 * HALF, R, ABL>(acc, lbias, cbase, h, wload, wnext, pixels);
}

// The three tick counters of the persistent kernels' diagnostic builds (TRS_FRAME_STAMPS, TRS_F5_STAMPS; never shipped): s_memtime ticks of the first
// staging, of the work and of the waits at the barrier.  ON = false: empty.
template <bool ON>
struct PhaseStamps {
    long long t0 = ON ? (long long)__builtin_amdgcn_s_memtime() : 0, ticks[3] = {0, 0, 0};
    enum { kStaging, kWork, kWait };
    __device__ __forceinline__ void mark(int i)
    {
        if constexpr (ON) { const long long t = (long long)__builtin_amdgcn_s_memtime(); ticks[i] += t - t0; t0 = t; }
    }
};
