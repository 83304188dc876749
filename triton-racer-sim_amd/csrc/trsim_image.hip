// trsim_image.hip — the image path of libtrsim.so: ImgPreprocessing.__process on whole frames (trs_preprocess: trim, colour masks,
// dynamic brightness; the Canny layer in a kernel of its own) and the pilot's float32 / 255 normalisation (trs_normalize), with their _host staging.
// The handle is reached as in the JPEG units: trsim_env.hpp and the accessors of trsim_internal.hpp.  The filter of ONE colour (the rasteriser's palette)
// and the argument check of a trs_pre_config are host-only: trsim_filter.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/trsim.h"
#include "trsim_device.hpp"
#include "trsim_env.hpp"
#include "trsim_filter.hpp"
#include "trsim_internal.hpp"

namespace {
// ---------------------------------------------------------------------------------------------
// Image path (SURVEY rows a10, a11 colour masks, a13): ImgPreprocessing.__process without the Canny layer
// (components/img_preprocessing.py:37-74,81-102) and the pilot's float32/255 normalisation
// (components/keras_pilot.py:49-55).  One 256-thread workgroup per frame; a lane handles 4 pixels (12 B).
//   pass 1: exact integer channel sums over rows 40..118 (cv2.mean, :88), wave reduce -> LDS -> delta (binary64)
//   pass 2: binary32 trim in numpy's operation order (:92-99), OpenCV 8-bit RGB->HSV + inRange masks (:65-74),
//           masks written over their destination channels (:57-63); the second read of the frame hits L2
// Bound: HBM, 2 x H*W*3 bytes per frame (one read, one write).
struct PreParams {
    const uint8_t* src; uint8_t* dst;
    const int* hsv_tab;                 // [512]: sdiv[256] | hdiv[256] (OpenCV fixed-point reciprocal tables)
    int n_img, H, W, gpr, gpe, r0, r1;  // 4-pixel groups per row / per frame; brightness rows [r0, r1)
    int dynamic, color, n_filters;
    float contrast, offset;
    double baseline;
    unsigned lo[4], hi[4];              // packed h | s<<8 | v<<16
    int dst_ch[4];
    int edge, edge_low, edge_high, edge_ch;   // Canny layer (edge kernel only)
    int off_mag, off_map, off_tab;      // edge kernel: offsets of the gradient magnitudes / edge map behind the trimmed frame; LDS offset of the tables
    unsigned char* scratch;             // edge kernel, frames too large for LDS: per-workgroup work arrays in global memory (L2 resident)
    size_t scratch_stride;
};

// four pixels (r, g, b, x) -> the 12 bytes of their group (the rasteriser's byte shuffles)
__device__ __forceinline__ u3v pack_rgb4(unsigned P0, unsigned P1, unsigned P2, unsigned P3)
{
    return u3v{__builtin_amdgcn_perm(P1, P0, 0x04020100u), __builtin_amdgcn_perm(P2, P1, 0x05040201u), __builtin_amdgcn_perm(P3, P2, 0x06050402u)};
}

__device__ __forceinline__ unsigned sum_bytes(unsigned w, unsigned mask, unsigned acc) { return __builtin_amdgcn_sad_u8(w & mask, 0u, acc); }

constexpr int kPreGpt = 19;   // 4-pixel groups a thread of trs_preprocess_kernel can hold between its two passes (dynamic brightness): 4,800 groups on 256 threads, 19,200 on 1024

// REGS: the instantiation that may hold a frame in registers between its two passes (dynamic brightness, see below and trs_preprocess's dispatch); the other
// one keeps 42 registers per thread - the occupancy the single-pass variants and the mask arithmetic live on (with the frame in registers: trim 21.5 -> 22.4 us
// per 1024 frames, trim + HSV masks 29.5 -> 30.2, and + 11 % on 1024-thread workgroups with masks; profiles/r04_image_path_regs.txt).
template <bool REGS>
__global__ __launch_bounds__(1024) void trs_preprocess_kernel(const PreParams p)   // 256 threads per frame at 120x160, 1024 for frames of 8,192+ pixel groups
{
    __shared__ int s_tab[512];
    __shared__ unsigned s_part[16][3];
    // per-value tables replace per-pixel arithmetic (the masks variant was VALU bound at ~80 integer ops per pixel):
    // s_trim[x] = the trim of byte value x for this frame's delta; s_rng[c][x] = bit f set when value x of component c
    // (h, s, v) lies inside the range of the filter that owns channel f's mask, as a BYTE mask -> the AND of three lookups is a pixel's masks (mask_pixel)
    __shared__ unsigned s_trim[256];
    __shared__ unsigned s_rng[3][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
    const size_t frame_bytes = (size_t)p.gpe * 12;
    for (int i = tid; i < 512; i += nthreads) s_tab[i] = p.hsv_tab[i];
    unsigned sel = 0;                                                       // the channels that carry a mask
    for (int i = tid; i < 768; i += nthreads) (&s_rng[0][0])[i] = range_byte_entry(p.lo, p.hi, p.dst_ch, p.n_filters, i, nullptr);
    (void)range_byte_entry(p.lo, p.hi, p.dst_ch, p.n_filters, 0, &sel);
    auto trim_table = [&](float deltaf) {                                   // this frame's trim of every byte value, in numpy's operation order (:92-99)
        if (tid < 256) {
            float x = (float)tid;
            if (p.dynamic) x = x + deltaf;
            x = x - p.offset;
            x = x * p.contrast;
            x = x + p.offset;
            x = x < 0.0f ? 0.0f : (x > 255.0f ? 255.0f : x);
            s_trim[tid] = (unsigned)(int)x;
        }
    };
    // Without dynamic brightness (the reference's default, config.py) nothing depends on the frame's own mean: the table is made once and
    // the frames stream through one pass, no channel sums and no barrier per frame (round 3).
    if (!p.dynamic) trim_table(0.0f);
    __syncthreads();
    for (int img = blockIdx.x; img < p.n_img; img += gridDim.x) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.src) + (size_t)img * frame_bytes, 0, (int)frame_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(p.dst + (size_t)img * frame_bytes, 0, (int)frame_bytes, 0x00020000);
        // Dynamic brightness needs the frame's own mean before its first pixel can be trimmed.  Where the frame fits the workgroup's registers (at most
        // kPreGpt groups per thread: 120x160 on 256 threads, 240x320 on 1024) it is read from memory ONCE - every load in flight together - and both the
        // channel sums and the second pass work on the registers (round 4, late: the sums pass used to read the brightness rows from memory and the
        // second pass the whole frame again: 6 of this variant's 36 us per 1024 frames).  Larger frames keep the two passes over memory.
        const bool in_regs = REGS && p.dynamic && (p.gpe + nthreads - 1) / nthreads <= kPreGpt;
        u3v R[REGS ? kPreGpt : 1];
        if constexpr (REGS) {
            if (in_regs) {
#pragma unroll
                for (int k = 0; k < kPreGpt; ++k) R[k] = __builtin_amdgcn_raw_buffer_load_b96(rs, (tid + k * nthreads) * 12, 0, 0);   // past the frame: zeros (the descriptor's bounds)
            }
        }
        if (p.dynamic) {
        // ---- pass 1: channel sums over the brightness rows ----
        unsigned sr = 0, sg = 0, sb = 0;
        auto add_group = [&](const u3v w) {
            // bytes: w.x = R0 G0 B0 R1 | w.y = G1 B1 R2 G2 | w.z = B2 R3 G3 B3
            sr = sum_bytes(w.x, 0xFF0000FFu, sr); sr = sum_bytes(w.y, 0x00FF0000u, sr); sr = sum_bytes(w.z, 0x0000FF00u, sr);
            sg = sum_bytes(w.x, 0x0000FF00u, sg); sg = sum_bytes(w.y, 0xFF0000FFu, sg); sg = sum_bytes(w.z, 0x00FF0000u, sg);
            sb = sum_bytes(w.x, 0x00FF0000u, sb); sb = sum_bytes(w.y, 0x0000FF00u, sb); sb = sum_bytes(w.z, 0xFF0000FFu, sb);
        };
        if (in_regs) {
            if constexpr (REGS) {
#pragma unroll
                for (int k = 0; k < kPreGpt; ++k) {
                    const int g = tid + k * nthreads;
                    if (g >= p.r0 * p.gpr && g < p.r1 * p.gpr) add_group(R[k]);
                }
            }
        } else {
            for (int g = p.r0 * p.gpr + tid; g < p.r1 * p.gpr; g += nthreads) add_group(__builtin_amdgcn_raw_buffer_load_b96(rs, g * 12, 0, 0));
        }
        sr = wave_sum_dpp(sr); sg = wave_sum_dpp(sg); sb = wave_sum_dpp(sb);   // (DPP: totals in lane 63)
        if (lane == 63) { s_part[wave][0] = sr; s_part[wave][1] = sg; s_part[wave][2] = sb; }
        __syncthreads();
        if (tid < 256) {                                                    // every thread of the table evaluates the same binary64 expression itself (exact integer
            const double cnt = (double)(p.r1 - p.r0) * (double)p.W;         // totals, any order): no serial pass by one thread, no barrier for the delta (round 3)
            double cur = 0.0;
            for (int ch = 0; ch < 3; ++ch) {
                unsigned long long tot = 0;
                for (int w = 0; w < nwaves; ++w) tot += s_part[w][ch];
                cur = cur + (cnt > 0 ? (double)tot / cnt : 0.0);
            }
            cur = cur + 0.0;
            trim_table((float)((p.baseline - cur) / 3));
        }
        __syncthreads();
        }
        // ---- pass 2: trim, masks, merge ----
        // (p.color is tested once per 4-pixel group, not per pixel: the four pixels' chains of dependent table lookups — trim, OpenCV's
        // reciprocal tables, the range bits — then interleave instead of running one behind the other)
        auto out_group = [&](const u3v w, int g) {
            // bytes: w.x = R0 G0 B0 R1 | w.y = G1 B1 R2 G2 | w.z = B2 R3 G3 B3 -> four trimmed pixels (r, g, b, 0)
            auto tr = [&](unsigned word, int k) -> unsigned { return s_trim[(word >> (8 * k)) & 255u]; };
            const unsigned t00 = tr(w.x, 0), t01 = tr(w.x, 1), t02 = tr(w.x, 2), t10 = tr(w.x, 3), t11 = tr(w.y, 0), t12 = tr(w.y, 1);
            const unsigned t20 = tr(w.y, 2), t21 = tr(w.y, 3), t22 = tr(w.z, 0), t30 = tr(w.z, 1), t31 = tr(w.z, 2), t32 = tr(w.z, 3);
            unsigned P0, P1, P2, P3;
            if (p.color) {                                                  // the components go to the masks as they come out of the trim table (round 4: not packed and unpacked again)
                P0 = mask_pixel_rgb((int)t00, (int)t01, (int)t02, s_tab, &s_rng[0][0], sel); P1 = mask_pixel_rgb((int)t10, (int)t11, (int)t12, s_tab, &s_rng[0][0], sel);
                P2 = mask_pixel_rgb((int)t20, (int)t21, (int)t22, s_tab, &s_rng[0][0], sel); P3 = mask_pixel_rgb((int)t30, (int)t31, (int)t32, s_tab, &s_rng[0][0], sel);
            } else {
                P0 = t00 | (t01 << 8) | (t02 << 16); P1 = t10 | (t11 << 8) | (t12 << 16);
                P2 = t20 | (t21 << 8) | (t22 << 16); P3 = t30 | (t31 << 8) | (t32 << 16);
            }
            const u3v out = pack_rgb4(P0, P1, P2, P3);
            __builtin_amdgcn_raw_buffer_store_b96(out, rd, g * 12, 0, 0);                         // (a group past the frame: dropped by the descriptor's bounds)
        };
        if (in_regs) {
            if constexpr (REGS) {
#pragma unroll
                for (int k = 0; k < kPreGpt; ++k) {
                    const int g = tid + k * nthreads;
                    if (g < p.gpe) out_group(R[k], g);
                }
            }
        } else {
            for (int g = tid; g < p.gpe; g += nthreads) out_group(__builtin_amdgcn_raw_buffer_load_b96(rs, g * 12, 0, 0), g);
        }
        if (p.dynamic) __syncthreads();   // s_part / s_trim are rewritten for the next frame of this workgroup
    }
}

// ImgPreprocessing with the Canny edge layer (components/img_preprocessing.py:37-54,76-79): cv2.Canny(img, a, b) on the trimmed
// 3-channel frame, OpenCV's algorithm (see oracle/trsim_oracle.c canny_u8c3 for the statement).  One 1024-thread workgroup per
// frame; LDS holds the trimmed frame (H*W*3 B), the gradient magnitudes with a zero border ((H+2) x (W+8) int16) and the
// edge map (H*W B: direction class, then 0 = weak / 1 = no / 2 = edge).  Hysteresis = repeated 8-neighbour sweeps until
// a block-wide OR reports no change.  Frames up to ~26,000 pixels (LDS).
// Round 3 (counters first, profiles/r03_image_path.txt: the kernel is bound by instruction ISSUE — its SIMDs issue ~100 % of
// the launch, 212 vector + 85 scalar instructions per pixel — not by LDS (11 % busy) or memory): the instruction count per
// pixel was cut, phase by phase (timing-only builds -DTRS_EDGE_ABLATE: Sobel 60 of 154 us, output 44):
//   * trim: one table of this frame's trim of every byte value (256 threads compute it once) instead of 9 operations per byte;
//   * Sobel: in binary32 — every value is an integer below 2^24, so the arithmetic is exact and |x| is a free source modifier —
//     on a thread that walks DOWN its 4-pixel column group (one new row of 18 values per output row instead of three), with the
//     separable form (column sums t + 2m + b and differences b - t shared by the 4 pixels); the direction class from the same
//     exact comparisons (|ys| 2^15 < |xs| 13573 etc.: all products below 2^24, the 67.5-degree test as
//     fma(|xs|, -2^16, |ys| 2^15) > |xs| 13573, whose left side is 2^15 (|ys| - 2 |xs|));
//   * output: the in-range tests of all (<= 4) filters from three table lookups (as trs_preprocess_kernel does).
#ifndef TRS_EDGE_ABLATE
#define TRS_EDGE_ABLATE 0   /* timing-only diagnostic builds of trs_preprocess_edge_kernel, never shipped (wrong results): 1 = no Sobel phase, 3 = no hysteresis, 4 = no output phase, 6 = no suppression compare (every pixel "no edge") */
#endif
constexpr int kEdgeBlock = 1024;          // 16 waves per frame (512 until round 2: the phases are latency chains of LDS reads, twice the waves hide twice as much)
constexpr int kEdgeGpt = 5;              // 4-pixel groups per thread held in registers between the two passes over a frame: 5120 groups = 20,480 pixels (120x160: 4800 groups)
constexpr int kEdgeTables = 512 * 4 + 3 * (kEdgeBlock / 64) * 4 + 16 + 2 * 256 * 4 + 3 * 256 * 4;   // s_tab | s_part | s_delta | s_trim[2] | s_rng

__device__ __forceinline__ bool has_zero_byte(unsigned w) { return ((w - 0x01010101u) & ~w & 0x80808080u) != 0u; }

// Six pixels x three channels of trimmed-frame row `row` around the 4-pixel group at column x0 (pixels x0 - 1 .. x0 + 4, replicated
// at the frame's left / right edge) as binary32, from five aligned dword reads and one v_cvt_f32_ubyteN per value.  x0 % 4 == 0.
__device__ __forceinline__ void edge_row_f(const unsigned char* simg, int W, int row, int x0, float (&v)[3][6])
{
    const unsigned* base = reinterpret_cast<const unsigned*>(simg + ((size_t)row * W + x0) * 3);
    unsigned d[5];
    d[0] = x0 ? base[-1] : 0u;
    d[1] = base[0]; d[2] = base[1]; d[3] = base[2]; d[4] = base[3];           // base[3] past the row's last group is read but not used (see below)
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int bi = 1 + 3 * j + c;                                     // byte of the 20-byte window that starts 4 bytes in front of the group
            v[c][j] = (float)((d[bi >> 2] >> (8 * (bi & 3))) & 255u);
        }
    if (x0 == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][0] = v[c][1];
    }
    if (x0 + 4 >= W) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][5] = v[c][4];
    }
}

// One output row of a 4-pixel group from its three input rows (t above, m the row itself, b below): per pixel the channel with the
// largest |dx| + |dy| (first on ties), its norm (-> mag, 4 x int16 = one 8-byte store) and its direction class (-> map).
__device__ __forceinline__ void edge_sobel_row(const float (&t)[3][6], const float (&m)[3][6], const float (&b)[3][6], short* mrow, unsigned char* maprow)
{
    // channel by channel (12 live column values instead of 36): column sums t + 2 m + b and differences b - t shared by the 4
    // pixels, then per pixel the running best (a strictly larger norm replaces it: the FIRST channel that reaches the maximum wins)
    float bn[4], xs[4], ys[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float sv[6], dv[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) { sv[j] = __builtin_fmaf(2.0f, m[c][j], t[c][j]) + b[c][j]; dv[j] = b[c][j] - t[c][j]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = q + 1;
            const float dx = sv[j + 1] - sv[j - 1];
            const float dy = dv[j - 1] + __builtin_fmaf(2.0f, dv[j], dv[j + 1]);
            const float nr = __builtin_fabsf(dx) + __builtin_fabsf(dy);
            if (c == 0 || nr > bn[q]) { bn[q] = nr; xs[q] = dx; ys[q] = dy; }
        }
    }
    unsigned cls4 = 0u, mg[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float ax = __builtin_fabsf(xs[q]), tg22x = ax * 13573.0f, ay = __builtin_fabsf(ys[q]) * 32768.0f;
        const float over = __builtin_fmaf(ax, -65536.0f, ay);                 // ay - (ax << 16), exact
        const unsigned cls = ay < tg22x ? 0u : (over > tg22x ? 1u : (xs[q] * ys[q] < 0.0f ? 3u : 2u));
        mg[q] = (unsigned)(int)bn[q];
        cls4 |= cls << (8 * q);
    }
    *reinterpret_cast<uint2*>(mrow) = make_uint2(mg[0] | (mg[1] << 16), mg[2] | (mg[3] << 16));
    *reinterpret_cast<unsigned*>(maprow) = cls4;
}

// SCRATCH = false: the three whole-frame work arrays live in LDS (frames up to ~26,000 pixels).  SCRATCH = true: they live in
// a per-workgroup global scratch that stays in L2 (any frame size, e.g. config 5's 240x320); only the tables are in
// LDS.  Same code, same results; __syncthreads() orders the workgroup's global accesses between the phases.
template <bool SCRATCH>
__global__ __launch_bounds__(kEdgeBlock) void trs_preprocess_edge_kernel(const PreParams p)
{
    unsigned char* const work = SCRATCH ? p.scratch + (size_t)blockIdx.x * p.scratch_stride : smem;
    unsigned char* const simg = work;
    short* const mag = reinterpret_cast<short*>(work + p.off_mag);           // pixel (x, y) at mag[(y + 1) * MP + x + 4]: a group's 4 values are 8-byte aligned
    unsigned char* const map = work + p.off_map;
    int* const s_tab = reinterpret_cast<int*>(smem + p.off_tab);
    unsigned* const s_part = reinterpret_cast<unsigned*>(s_tab + 512);       // [2][3] channel sums of the brightness rows, by frame parity: the waves ADD their totals (LDS atomics;
                                                                             // round 4: the delta phase's 16-lane 64-bit shuffle reductions are gone; < 2^24 per channel)
    float* const s_delta = reinterpret_cast<float*>(s_part + 3 * (kEdgeBlock / 64));
    unsigned* const s_trim2 = reinterpret_cast<unsigned*>(s_delta + 4);       // [2][256] the trim of every byte value, by frame parity (the next frame's table is made during this frame's output phase)
    unsigned* const s_rng = s_trim2 + 512;                                   // [3][256] byte ch = 0xFF: value x of component c (h, s, v) lies inside the range of the filter that owns channel ch's mask (mask_pixel)
    const int tid = threadIdx.x, lane = tid & 63;
    // Every phase takes its thread index through `fresh`: an empty asm the compiler cannot see through, so that what a phase derives from
    // the index (row / column splits, addresses) is computed where it is used.  Left alone, hipcc hoisted those values of ALL phases in
    // front of the frame loop and kept them alive across it: 65 spilled registers, 240 bytes of scratch per lane = 63 MB written at
    // the start of a launch and re-read at every phase (the first frame's first phase took 40 k clocks against 3.7 k for the others).
    auto fresh = [](int v) -> int { asm volatile("" : "+v"(v)); return v; };
    const int H = p.H, W = p.W, MP = W + 8, npx = H * W;
    const size_t frame_bytes = (size_t)p.gpe * 12;
    const int chunk_groups = kEdgeBlock * kEdgeGpt, nchunks = (p.gpe + chunk_groups - 1) / chunk_groups;
    const bool one_chunk = nchunks == 1;
    auto fetch = [&](const __amdgpu_buffer_rsrc_t& r, int c, u3v (&R)[kEdgeGpt]) {
        const int t = fresh(tid);
#pragma unroll
        for (int k = 0; k < kEdgeGpt; ++k) R[k] = __builtin_amdgcn_raw_buffer_load_b96(r, (c * chunk_groups + k * kEdgeBlock + t) * 12, 0, 0);   // past the frame: zeros (buffer bounds)
    };
    u3v R[kEdgeGpt];                                                          // this thread's groups of the frame (see below)
    if (one_chunk && (int)blockIdx.x < p.n_img) {                            // the workgroup's FIRST frame is requested before anything else: its memory latency runs under the table set-up below
        const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.src) + (size_t)blockIdx.x * frame_bytes, 0, (int)frame_bytes, 0x00020000);
        fetch(r0, 0, R);
    }
    for (int i = tid; i < 512; i += kEdgeBlock) s_tab[i] = p.hsv_tab[i];
    unsigned sel = 0;                                                        // the channels that carry a mask (a later filter on a channel replaces an earlier one, :57-63)
    for (int i = tid; i < 768; i += kEdgeBlock) s_rng[i] = range_byte_entry(p.lo, p.hi, p.dst_ch, p.n_filters, i, nullptr);
    (void)range_byte_entry(p.lo, p.hi, p.dst_ch, p.n_filters, 0, &sel);
    // Sobel work items: (4-pixel column group, chunk of rows); the whole block works at once when the frame has <= 1024 / gpr chunks
    const int nchunk = max(1, kEdgeBlock / p.gpr), rows_per = (H + nchunk - 1) / nchunk;
#ifdef TRS_EDGE_STAMPS   /* diagnostic build: shader clocks per phase of workgroup 7, summed over its frames, printed at the end */
    unsigned long long ph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
#define EDGE_STAMP(k) do { if (blockIdx.x == 7 && tid == 0) { const unsigned long long tn = __builtin_amdgcn_s_memtime(); if ((k) > 0) ph[k] += tn - tprev; tprev = tn; } } while (0)
#else
#define EDGE_STAMP(k) do { } while (0)
#endif
    const int chunk_groups0 = kEdgeBlock * kEdgeGpt;
    auto chunk_sums = [&](const u3v (&R)[kEdgeGpt], int c, unsigned& sr, unsigned& sg, unsigned& sb) {   // this thread's groups of chunk c inside the brightness rows
        const int t = fresh(tid);
#pragma unroll
        for (int k = 0; k < kEdgeGpt; ++k) {
            const int g = c * chunk_groups0 + k * kEdgeBlock + t;
            if (g >= p.r0 * p.gpr && g < p.r1 * p.gpr) {
                const u3v w = R[k];
                sr = sum_bytes(w.x, 0xFF0000FFu, sr); sr = sum_bytes(w.y, 0x00FF0000u, sr); sr = sum_bytes(w.z, 0x0000FF00u, sr);
                sg = sum_bytes(w.x, 0x0000FF00u, sg); sg = sum_bytes(w.y, 0xFF0000FFu, sg); sg = sum_bytes(w.z, 0x00FF0000u, sg);
                sb = sum_bytes(w.x, 0x00FF0000u, sb); sb = sum_bytes(w.y, 0x0000FF00u, sb); sb = sum_bytes(w.z, 0xFF0000FFu, sb);
            }
        }
    };
    auto publish_sums = [&](unsigned sr, unsigned sg, unsigned sb, int par) {  // wave totals -> s_part[par] (read by the delta phase behind a barrier)
        sr = wave_sum_dpp(sr); sg = wave_sum_dpp(sg); sb = wave_sum_dpp(sb);   // (DPP: the wave's totals end in lane 63; the ds_bpermute shuffles were six dependent LDS round trips per frame)
        if (lane == 63) { atomicAdd(&s_part[par * 3], sr); atomicAdd(&s_part[par * 3 + 1], sg); atomicAdd(&s_part[par * 3 + 2], sb); }
    };
    auto make_trim_table = [&](int par_of_sums, unsigned* table) {           // one thread per byte value (tid < 256): delta from the frame's channel totals, then the trim
        const int t = fresh(tid);
        const double cnt = (double)(p.r1 - p.r0) * (double)W;
        double cur = 0.0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned tot = s_part[par_of_sums * 3 + ch];               // (a uniform LDS read: exact integer totals, any order of the adds)
            cur = cur + (cnt > 0 ? (double)tot / cnt : 0.0);
        }
        cur = cur + 0.0;
        const float deltaf = (float)((p.baseline - cur) / 3), off = p.offset, con = p.contrast;
        float x = (float)t;
        if (p.dynamic) x = x + deltaf;
        x = x - off; x = x * con; x = x + off;
        x = x < 0.0f ? 0.0f : (x > 255.0f ? 255.0f : x);
        table[t] = (unsigned)(int)x;
    };
    bool table_ready = false;                                                 // uniform: s_trim2[par] already holds this frame's table (made during the previous frame's output phase)
    if (tid < 6) s_part[tid] = 0u;                                            // (behind the first barrier below before anyone adds)
    int par = 0;                                                              // parity of the current frame of this workgroup
    bool sums_ready = false;                                                  // uniform: s_part already holds this frame's sums
    for (int img = blockIdx.x; img < p.n_img; img += gridDim.x) {
        EDGE_STAMP(0);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.src) + (size_t)img * frame_bytes, 0, (int)frame_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(p.dst + (size_t)img * frame_bytes, 0, (int)frame_bytes, 0x00020000);
        // magnitudes outside the image are 0: the rows above / below and the columns left / right of it (the interior is overwritten)
        for (int i = fresh(tid); i < 2 * MP + 2 * H; i += kEdgeBlock) {
            int idx;
            if (i < MP) idx = i;
            else if (i < 2 * MP) idx = (H + 1) * MP + (i - MP);
            else { const int k = i - 2 * MP, y = k >> 1; idx = (y + 1) * MP + ((k & 1) ? W + 4 : 3); }
            mag[idx] = 0;
        }
        // ---- the frame: kEdgeGpt groups per thread in registers, every load issued before the first is used (a thread that loaded and used
        // its groups one after the other paid one memory round trip per group: the two passes over the frame were 29 % of the kernel).
        // A frame of up to 1024 x kEdgeGpt groups (20,480 pixels: 120x160, not every frame whose work arrays fit LDS - 120x200 fits with
        // 6,000 groups) is read from memory ONCE — both passes work on the registers — and the next frame's loads are issued as soon as the
        // registers are free, in front of the Sobel phase.  Larger frames, in LDS or in the scratch, take the passes in chunks of
        // 1024 x kEdgeGpt groups (the second pass reads L2) and have no prefetch, no early sums and no early table. ----
        if (!one_chunk) fetch(rs, 0, R);                                    // (one-chunk frames: the first was requested at the kernel's start, the others during the previous frame)
        // ---- channel sums over the brightness rows -> delta (as trs_preprocess_kernel) ----
        // (one-chunk frames after the first: the sums were taken from the prefetched registers in the middle of the previous frame, see below -
        // this phase and its barrier were 12 % of the kernel, most of it waves waiting for each other right after the previous frame's last phase)
        if (!sums_ready) {
            unsigned sr = 0, sg = 0, sb = 0;
            for (int c = 0; c < nchunks; ++c) {
                if (c > 0) fetch(rs, c, R);
                chunk_sums(R, c, sr, sg, sb);
            }
            __syncthreads();                                                  // (the zeroing of s_part[par] is complete: kernel start, or the previous frame's delta phase)
            publish_sums(sr, sg, sb, par);
            __syncthreads();
        }
        EDGE_STAMP(1);
        // every thread of the table reads the three totals (the waves added theirs with LDS atomics: exact integers, any order) and evaluates the same
        // binary64 expression: no serial pass by one thread, no barrier for the delta, no reduction in this phase (round 3 reduced 16 partial sums per
        // channel here with 64-bit shuffles)
        unsigned* const s_trim = s_trim2 + par * 256;
        if (tid < 3) s_part[(par ^ 1) * 3 + tid] = 0u;                       // the NEXT frame's sums start from zero (their adders are behind the barriers below; that half was last read for the previous frame's table)
        if (!table_ready) {
            if (tid < 256) make_trim_table(par, s_trim);                     // this frame's trim of every byte value, in numpy's operation order (:92-99)
            __syncthreads();
        }
        EDGE_STAMP(2);
        // ---- trimmed frame -> LDS ----
        for (int c = 0, t = fresh(tid); c < nchunks; ++c) {
            if (!one_chunk) fetch(rs, c, R);
#pragma unroll
            for (int k = 0; k < kEdgeGpt; ++k) {
                const int g = c * chunk_groups + k * kEdgeBlock + t;
                if (g < p.gpe) {
                    const unsigned src[3] = {R[k].x, R[k].y, R[k].z};
                    unsigned out[3];
#pragma unroll
                    for (int k3 = 0; k3 < 3; ++k3) {
                        const unsigned v = src[k3];
                        out[k3] = s_trim[v & 255u] | (s_trim[(v >> 8) & 255u] << 8) | (s_trim[(v >> 16) & 255u] << 16) | (s_trim[v >> 24] << 24);
                    }
                    unsigned* d = reinterpret_cast<unsigned*>(simg + (size_t)g * 12);
                    d[0] = out[0]; d[1] = out[1]; d[2] = out[2];
                }
            }
        }
        if (one_chunk && img + (int)gridDim.x < p.n_img) {                 // the next frame of this workgroup: on its way during the phases below
            const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.src) + (size_t)(img + gridDim.x) * frame_bytes, 0, (int)frame_bytes, 0x00020000);
            fetch(rn, 0, R);
        }
        __syncthreads();
        EDGE_STAMP(3);
        // ---- Sobel per channel, the channel with the largest |dx| + |dy| wins (first on ties) ----
        // mag <- the winner's norm, map <- its gradient direction class for the non-maximum suppression (OpenCV's fixed-point
        // tangents: 0 = compare left / right, 1 = up / down, 2 / 3 = the two diagonals), so that the suppression needs no second Sobel
        for (int item = fresh(tid); item < (TRS_EDGE_ABLATE == 1 ? 0 : p.gpr * nchunk); item += kEdgeBlock) {
            const int rc = item / p.gpr, cg = item - rc * p.gpr, x0 = cg * 4;
            const int y0 = rc * rows_per, y1 = min(H, y0 + rows_per);
            if (y0 >= y1) continue;
            float ra[3][6], rb[3][6], rc3[3][6];                              // three rows in rotating roles: no register copies between output rows
            edge_row_f(simg, W, y0 > 0 ? y0 - 1 : 0, x0, ra);
            edge_row_f(simg, W, y0, x0, rb);
            for (int y = y0; y < y1; y += 3) {
                edge_row_f(simg, W, y + 1 < H ? y + 1 : H - 1, x0, rc3);
                edge_sobel_row(ra, rb, rc3, mag + (y + 1) * MP + x0 + 4, map + (size_t)y * W + x0);
                if (y + 1 < y1) {
                    edge_row_f(simg, W, y + 2 < H ? y + 2 : H - 1, x0, ra);
                    edge_sobel_row(rb, rc3, ra, mag + (y + 2) * MP + x0 + 4, map + (size_t)(y + 1) * W + x0);
                }
                if (y + 2 < y1) {
                    edge_row_f(simg, W, y + 3 < H ? y + 3 : H - 1, x0, rb);
                    edge_sobel_row(rc3, ra, rb, mag + (y + 3) * MP + x0 + 4, map + (size_t)(y + 2) * W + x0);
                }
            }
        }
        __syncthreads();
        EDGE_STAMP(4);
        // the NEXT frame's channel sums, from the registers its groups were prefetched into in front of the Sobel phase (they have arrived;
        // s_part is not read again in this frame): the next frame starts with its delta, no sums phase and no barrier for it
        sums_ready = false;
        if (one_chunk && img + (int)gridDim.x < p.n_img) {
            unsigned sr = 0, sg = 0, sb = 0;
            chunk_sums(R, 0, sr, sg, sb);
            publish_sums(sr, sg, sb, par ^ 1);
            sums_ready = true;
        }
        // ---- non-maximum suppression + double threshold: map <- 0 = weak / 1 = no / 2 = edge ----
        int weak_here = 0;                                                   // this thread wrote a weak pixel (0) in the phase below
        // Branch-free, two pixels per instruction (hipcc turned the per-pixel choice of neighbours into divergent branches with LDS reads
        // inside them: 133 instructions per pixel).  A comparison a < b of two magnitudes (0 .. 2040) is the sign bit of the 16-bit
        // difference a - b; the magnitudes arrive packed two per dword, so v_pk_sub_i16 compares a PAIR of pixels with their
        // neighbours, the four direction classes' tests are combined on those sign bits (bits 15 and 31; the others carry garbage
        // and are masked at the end) and the pixel's own class picks one with two bit-field selects.
        {
            typedef short s2v __attribute__((ext_vector_type(2)));
            auto sub2 = [](unsigned a, unsigned b) -> unsigned { return __builtin_bit_cast(unsigned, (s2v)(__builtin_bit_cast(s2v, a) - __builtin_bit_cast(s2v, b))); };
            auto bsel = [](unsigned mask, unsigned a, unsigned b) -> unsigned { return (mask & a) | (~mask & b); };   // v_bfi_b32
            const int lo_c = min(max(p.edge_low, -1), 32767), hi_c = min(max(p.edge_high, -1), 32767);   // magnitudes are <= 2040: any larger threshold behaves like 32767
            const unsigned low2 = (unsigned)(lo_c & 0xFFFF) * 0x10001u, high2 = (unsigned)(hi_c & 0xFFFF) * 0x10001u;
            // (row, column group) of this thread's groups without a division per group: g advances by 1024 = dy rows + dc column groups
            const int dy = kEdgeBlock / p.gpr, dc = kEdgeBlock - dy * p.gpr;
            int g = fresh(tid), y = g / p.gpr, cg = g - y * p.gpr;
            for (; g < p.gpe; g += kEdgeBlock, y += dy, cg += dc) {
                if (cg >= p.gpr) { cg -= p.gpr; ++y; }
                const int x0 = cg * 4;
                unsigned ctr[3][2], lft[3][2], rgt[3][2];                    // per row: the pair itself, its left and its right neighbours
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) {
                    const short* mr = mag + (y + rr) * MP + x0;              // shorts x0 .. x0 + 9 hold columns x0 - 4 .. x0 + 5
                    const uint2 a = *reinterpret_cast<const uint2*>(mr), b = *reinterpret_cast<const uint2*>(mr + 4);
                    const unsigned c = *reinterpret_cast<const unsigned*>(mr + 8);
                    ctr[rr][0] = b.x; ctr[rr][1] = b.y;                       // columns (x0, x0 + 1), (x0 + 2, x0 + 3)
                    lft[rr][0] = __builtin_amdgcn_alignbit(b.x, a.y, 16);     // (x0 - 1, x0)
                    lft[rr][1] = __builtin_amdgcn_alignbit(b.y, b.x, 16);     // (x0 + 1, x0 + 2)
                    rgt[rr][0] = lft[rr][1];
                    rgt[rr][1] = __builtin_amdgcn_alignbit(c, b.y, 16);       // (x0 + 3, x0 + 4)
                }
                const unsigned cls4 = *reinterpret_cast<const unsigned*>(map + (size_t)g * 4);
                unsigned out4 = 0u;
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    const unsigned M = ctr[1][pr];
                    const unsigned t0 = sub2(lft[1][pr], M) & ~sub2(M, rgt[1][pr]);     // class 0: m > left  && m >= right
                    const unsigned t1 = sub2(ctr[0][pr], M) & ~sub2(M, ctr[2][pr]);     // class 1: m > up    && m >= down
                    const unsigned t2 = sub2(lft[0][pr], M) & sub2(rgt[2][pr], M);      // class 2: m > up-left  && m > down-right
                    const unsigned t3 = sub2(rgt[0][pr], M) & sub2(lft[2][pr], M);      // class 3: m > up-right && m > down-left
                    const unsigned c2 = (cls4 >> (16 * pr)) & 0xFFFFu;                  // the pair's classes: byte 0, byte 1
                    const unsigned b0 = (c2 << 15) | (c2 << 23), b1 = (c2 << 14) | (c2 << 22);   // class bit 0 / bit 1 of the two pixels at bits 15 and 31
                    const unsigned sel = bsel(b1, bsel(b0, t3, t2), bsel(b0, t1, t0));
                    const unsigned ismax = TRS_EDGE_ABLATE == 6 ? 0u : (sel & sub2(low2, M));   // ... && m > low
                    const unsigned strong = ismax & sub2(high2, M);                              // ... && m > high
                    const unsigned h = ((~ismax >> 15) & 0x00010001u) | ((strong >> 14) & 0x00020002u);   // per half: 1 = no, 0 = weak, 2 = edge
                    out4 |= ((h & 0xFFu) | ((h >> 8) & 0xFF00u)) << (16 * pr);
                }
                *reinterpret_cast<unsigned*>(map + (size_t)g * 4) = out4;
                weak_here |= has_zero_byte(out4) ? 1 : 0;                    // (a group past the frame's end does not come here)
            }
        }
        // the barrier behind the suppression phase is a vote: a frame without a single weak pixel (0) has no hysteresis to run - no sweep, no barrier of its own
        const bool frame_has_weak = __syncthreads_or(weak_here) != 0;
        EDGE_STAMP(5);
        // ---- hysteresis: weak pixels 8-connected to an edge become edges.  A thread owns a contiguous run of pixels and walks it
        // forwards, then backwards: a chain along a row closes in one sweep instead of one pixel per sweep (the closure does not
        // depend on the order: only weak -> edge transitions); sweeps repeat until a block-wide OR reports no change ----
        {
            const int strip = 4 * ((p.gpe + kEdgeBlock - 1) / kEdgeBlock), s0 = fresh(tid) * strip, s1 = min(npx, s0 + strip);
            auto visit = [&](int px) -> int {
                const int y = px / W, x = px - y * W;
                bool hit = false;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int yy = y + dy, xx = x + dx;
                        if (yy >= 0 && yy < H && xx >= 0 && xx < W && map[yy * W + xx] == 2) hit = true;
                    }
                if (hit) map[px] = 2;
                return hit ? 1 : 0;
            };
            for (int iter = 0; iter < (TRS_EDGE_ABLATE == 3 || !frame_has_weak ? 0 : npx); ++iter) {
                int changed = 0;
                // A strip without a weak pixel (almost every strip) has nothing to do in either direction: its words are read TOGETHER first (one LDS
                // round trip) - the two walks below read them one after the other behind a branch each (ten dependent round trips per sweep).
                bool any_weak = false;
                for (int q = s0; q < s1; q += 4) any_weak |= has_zero_byte(*reinterpret_cast<const unsigned*>(map + q));
                if (any_weak) {
                    for (int q = s0; q < s1; q += 4) {
                        if (!has_zero_byte(*reinterpret_cast<const unsigned*>(map + q))) continue;
                        for (int k = 0; k < 4; ++k) if (map[q + k] == 0) changed |= visit(q + k);
                    }
                    for (int q = s1 - 4; q >= s0; q -= 4) {
                        if (!has_zero_byte(*reinterpret_cast<const unsigned*>(map + q))) continue;
                        for (int k = 3; k >= 0; --k) if (map[q + k] == 0) changed |= visit(q + k);
                    }
                }
                if (!__syncthreads_or(changed)) break;
            }
        }
        EDGE_STAMP(6);
        // ---- colour masks on the trimmed frame, merge, edge layer last (img_preprocessing.py:43-53) ----
        // (the switch p.color is tested once per group, not per pixel: four independent chains of dependent table lookups then
        // interleave instead of running one after the other)
        // The NEXT frame's trim table, by the first four waves (one per SIMD), while the other twelve keep the SIMDs busy with this phase: its channel
        // sums are complete (published in front of the suppression phase, three barriers ago).  Until late round 4 every frame began with this
        // table and a barrier - 256 threads in a chain of binary64 divisions, 768 waiting: 6 % of the kernel by the phase stamps.
        table_ready = sums_ready;
        if (table_ready && tid < 256) make_trim_table(par ^ 1, s_trim2 + (par ^ 1) * 256);
        for (int g = fresh(tid); g < (TRS_EDGE_ABLATE == 4 ? 0 : p.gpe); g += kEdgeBlock) {
            const unsigned* sw = reinterpret_cast<const unsigned*>(simg + (size_t)g * 12);
            const unsigned w0 = sw[0], w1 = sw[1], w2 = sw[2];              // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3, trimmed
            const unsigned e4 = *reinterpret_cast<const unsigned*>(map + (size_t)g * 4);
            unsigned P[4] = {w0, __builtin_amdgcn_alignbyte(w1, w0, 3), __builtin_amdgcn_alignbyte(w2, w1, 2), w2 >> 8};   // pixels as (r, g, b, x)
            if (p.color) {
#pragma unroll
                for (int q = 0; q < 4; ++q) P[q] = mask_pixel(P[q], s_tab, s_rng, sel);
            }
            if (p.edge_ch >= 0 && p.edge_ch <= 2) {                          // the edge layer last (:43-53): 255 where the map says edge (2), else 0
                const unsigned e1 = (e4 >> 1) & 0x01010101u, evb = (e1 << 8) - e1;   // per pixel byte: 0xFF / 0x00
                const unsigned em = 0xFFu << (8 * p.edge_ch);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned ev = (unsigned)__builtin_amdgcn_sbfe((int)evb, 8 * q, 8);   // all ones / zero
                    P[q] = (ev & em) | (P[q] & ~em);
                }
            }
            const u3v out = pack_rgb4(P[0], P[1], P[2], P[3]);
            __builtin_amdgcn_raw_buffer_store_b96(out, rd, g * 12, 0, 0);
        }
        __syncthreads();   // LDS is reused by the next frame of this workgroup
        par ^= 1;
        EDGE_STAMP(7);
    }
#ifdef TRS_EDGE_STAMPS
    if (blockIdx.x == 7 && tid == 0)
        printf("edge phases [clocks, workgroup 7, all its frames]: sums %llu | delta+table %llu | trim %llu | sobel %llu | nms %llu | hysteresis %llu | output %llu\n",
               ph[1], ph[2], ph[3], ph[4], ph[5], ph[6], ph[7]);
#endif
}

// float32(img) / 255 (keras_pilot.py:49-50): 4 bytes in, one 16-B store out per lane
__global__ __launch_bounds__(256) void trs_normalize_kernel(const uint32_t* src, float4* dst, size_t n4)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const uint32_t w = src[i];
        dst[i] = make_float4((float)(w & 255u) / 255.0f, (float)((w >> 8) & 255u) / 255.0f, (float)((w >> 16) & 255u) / 255.0f, (float)(w >> 24) / 255.0f);
    }
}

// ---- host side ----

// staging of the *_host entry points: room for `frames` frames in, out and as binary32
int ensure_tmp(trs_env* e, size_t frames)
{
    if (frames <= e->tmp_cap) return TRS_OK;
    HIPCHK(hipStreamSynchronize(e->sP));
    e->tmp_cap = 0;
    const size_t fb = (size_t)e->H * e->W * 3;
    HIPCHK(e->tmp_in.alloc(frames * fb));
    HIPCHK(e->tmp_out.alloc(frames * fb));
    HIPCHK(e->tmp_f.alloc(frames * fb * sizeof(float)));
    e->tmp_cap = frames;
    return TRS_OK;
}

}  // namespace

TRS_EXPORT void trs_default_pre_config(trs_pre_config* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->struct_size = (uint32_t)sizeof *c;
    c->brightness_baseline = 550.0; c->contrast_ratio = 1.0f; c->contrast_offset = 125.0f;
    c->n_filters = 2;                                       // core/config.py:23-24: white and yellow
    const uint8_t lo[2][3] = {{0, 0, 130}, {25, 180, 155}}, hi[2][3] = {{180, 64, 255}, {43, 255, 255}};
    std::memcpy(c->hsv_lo, lo, sizeof lo); std::memcpy(c->hsv_hi, hi, sizeof hi);
    c->dst_channel[0] = 0; c->dst_channel[1] = 1;
    c->edge_threshold_a = 60; c->edge_threshold_b = 100; c->edge_dst_channel = 2;
}

TRS_EXPORT int trs_preprocess(trs_env* e, const trs_pre_config* c, const uint8_t* d_src, uint8_t* d_dst, int n_images, const uint8_t** d_out)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    const char* why = nullptr;
    int rc = trsim::check_pre(c, &why);
    if (rc) return trs_internal_fail(rc, why);
    if (n_images < 0) return trs_internal_fail(TRS_ERR_ARG, "n_images < 0");
    HIPCHK(hipSetDevice(e->device));
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }
    if (!d_src) {
        if (!trs_internal_latest_frame(e) || n_images != e->n) return trs_internal_fail(TRS_ERR_ARG, "latest-frame source needs n_images == n_envs and a camera");
        d_src = trs_internal_latest_frame(e);
    }
    if (!d_dst) {
        if (n_images > e->n) return trs_internal_fail(TRS_ERR_ARG, "own buffer holds n_envs frames");
        HIPCHK(e->pre.reserve((size_t)e->n * e->H * e->W * 3));   // (allocated once: the size is fixed)
        d_dst = e->pre.get();
    }
    if (d_out) *d_out = d_dst;
    if (n_images == 0) return TRS_OK;
    rc = trsim::ensure_hsv_table(e);
    if (rc) return rc;
    PreParams p{};
    p.src = d_src; p.dst = d_dst; p.hsv_tab = e->hsv_tab.get();
    p.n_img = n_images; p.H = e->H; p.W = e->W; p.gpr = e->W / 4; p.gpe = p.gpr * e->H;
    p.r0 = std::min(40, e->H); p.r1 = std::min(119, e->H);                 // img[40:119] (img_preprocessing.py:88)
    p.dynamic = c->dynamic_brightness; p.color = c->color_filter_enabled; p.n_filters = c->n_filters;
    p.contrast = c->contrast_ratio; p.offset = c->contrast_offset; p.baseline = c->brightness_baseline;
    const trsim::FilterBounds fb = trsim::filter_bounds(*c);
    std::memcpy(p.lo, fb.lo, sizeof p.lo); std::memcpy(p.hi, fb.hi, sizeof p.hi); std::memcpy(p.dst_ch, fb.dst, sizeof p.dst_ch);
    if (c->edge_detection_enabled) {
        p.edge = 1; p.edge_ch = c->edge_dst_channel;
        p.edge_low = std::min(c->edge_threshold_a, c->edge_threshold_b);          // cv::Canny swaps the thresholds into order
        p.edge_high = std::max(c->edge_threshold_a, c->edge_threshold_b);
        const size_t npx = (size_t)e->H * e->W;
        p.off_mag = (int)trsim::align_up(npx * 3, 16);
        p.off_map = p.off_mag + (int)trsim::align_up((size_t)(e->H + 2) * (e->W + 8) * 2, 16);   // rows of W + 8 int16: a 4-pixel group's values are 8-byte aligned
        const size_t work = (size_t)p.off_map + trsim::align_up(npx, 16) + 16;
        const int tables = kEdgeTables;
        const int grid = std::min(n_images, e->cu_count);
        if (work + tables <= 160 * 1024) {                                    // whole frame in LDS
            p.off_tab = (int)work;
            const int lds = p.off_tab + tables;
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(trs_preprocess_edge_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            hipLaunchKernelGGL(trs_preprocess_edge_kernel<false>, dim3(grid), dim3(kEdgeBlock), lds, e->sP, p);
        } else {                                                              // work arrays in a global scratch (stays in L2), tables in LDS
            p.off_tab = 0;
            p.scratch_stride = trsim::align_up(work, 256);
            const size_t need = p.scratch_stride * (size_t)grid;
            if (e->edge_scratch.bytes() < need) {
                HIPCHK(hipStreamSynchronize(e->sP));
                HIPCHK(e->edge_scratch.reserve(need));
            }
            p.scratch = e->edge_scratch.get();
            hipLaunchKernelGGL(trs_preprocess_edge_kernel<true>, dim3(grid), dim3(kEdgeBlock), tables, e->sP, p);
        }
        HIPCHK(hipGetLastError());
        return TRS_OK;
    }
    const int block = p.gpe >= 8192 ? 1024 : 256;                          // large frames: more waves per frame (one workgroup per frame cannot fill the chip otherwise)
    const int grid = std::min(n_images, e->cu_count * (block == 256 ? 8 : 2));
    if (p.dynamic && (!p.color || block == 256)) hipLaunchKernelGGL(trs_preprocess_kernel<true>, dim3(grid), dim3(block), 0, e->sP, p);   // the frame held in registers between the sums and the trim (with the masks' arithmetic only on 256-thread workgroups: on 1024 threads the registers cost more occupancy than the second read)
    else hipLaunchKernelGGL(trs_preprocess_kernel<false>, dim3(grid), dim3(block), 0, e->sP, p);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

TRS_EXPORT int trs_preprocess_host(trs_env* e, const trs_pre_config* c, const uint8_t* h_src, uint8_t* h_dst, int n_images)
{
    if (!e || !h_src || !h_dst || n_images < 0) return trs_internal_fail(TRS_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(e->device));
    if (n_images == 0) return TRS_OK;
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }
    int rc = ensure_tmp(e, (size_t)n_images);
    if (rc) return rc;
    const size_t bytes = (size_t)n_images * e->H * e->W * 3;
    HIPCHK(hipMemcpyAsync(e->tmp_in.get(), h_src, bytes, hipMemcpyHostToDevice, e->sP));
    rc = trs_preprocess(e, c, e->tmp_in.get(), e->tmp_out.get(), n_images, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_dst, e->tmp_out.get(), bytes, hipMemcpyDeviceToHost, e->sP));
    e->d2h_bytes += bytes; e->h2d_bytes += bytes;
    HIPCHK(hipStreamSynchronize(e->sP));
    return TRS_OK;
}

TRS_EXPORT int trs_normalize(trs_env* e, const uint8_t* d_src, float* d_dst, int n_images)
{
    if (!e || !d_dst || n_images < 0) return trs_internal_fail(TRS_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(e->device));
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }
    if (!d_src) {
        if (!trs_internal_latest_frame(e) || n_images != e->n) return trs_internal_fail(TRS_ERR_ARG, "latest-frame source needs n_images == n_envs and a camera");
        d_src = trs_internal_latest_frame(e);
    }
    const size_t n4 = (size_t)n_images * e->H * e->W * 3 / 4;            // W % 4 == 0 -> whole dwords
    if (n4 == 0) return TRS_OK;
    const int grid = (int)std::min<size_t>((n4 + 255) / 256, (size_t)e->cu_count * 16);
    hipLaunchKernelGGL(trs_normalize_kernel, dim3(grid), dim3(256), 0, e->sP, reinterpret_cast<const uint32_t*>(d_src), reinterpret_cast<float4*>(d_dst), n4);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

TRS_EXPORT int trs_normalize_host(trs_env* e, const uint8_t* h_src, float* h_dst, int n_images)
{
    if (!e || !h_src || !h_dst || n_images < 0) return trs_internal_fail(TRS_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(e->device));
    if (n_images == 0) return TRS_OK;
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }
    int rc = ensure_tmp(e, (size_t)n_images);
    if (rc) return rc;
    const size_t bytes = (size_t)n_images * e->H * e->W * 3;
    HIPCHK(hipMemcpyAsync(e->tmp_in.get(), h_src, bytes, hipMemcpyHostToDevice, e->sP));
    rc = trs_normalize(e, e->tmp_in.get(), e->tmp_f.get(), n_images);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_dst, e->tmp_f.get(), bytes * sizeof(float), hipMemcpyDeviceToHost, e->sP));
    e->d2h_bytes += bytes * sizeof(float); e->h2d_bytes += bytes;
    HIPCHK(hipStreamSynchronize(e->sP));
    return TRS_OK;
}
