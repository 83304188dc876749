// trsim_train_conv.hip — training the pilot's last convolutions on the device (include/trsim_spec.h, "training the pilot's last convolutions"): conv4 .. conv7
// of a loaded 22-array pilot, all 3 x 3, stride 1, valid, 64 or 128 channels in and out, move by the session's Adam; conv1 .. conv3 stay as loaded.
// trs_pilot_train_step (trsim_train.hip) calls trs_train_conv_step after its own backward pass and before its Adam, with delta1 as binary16 q1 under the
// batch's scale 2^s.  The kernels, all on the handle's stream (x(l), q(l): binary16 [pixel][channel], the pixel index running over frame, row, column):
//   trs_train_g7_kernel       G7 = [x7 > 0] . 2^-s W1h q1 on the matrix cores from dense1's granules as the forward read them.  The reduction index (the
//                             output o) is the slow index of the granules, so a workgroup's 128 features x 128 outputs go to LDS as they lie and every
//                             weight fragment is two ds_read_b64_tr_b16 (tr_fragment), read once; q1's fragments come straight from memory.
//                             trs_train_g7_drop_kernel: the same body with dropout's s as one more factor, for a step that dropped x7
//   trs_train_cquant_kernel   G(l) -> q(l) = binary16(G(l) 2^s_l), s_l = train_scale_exponent of the integer maximum of |G(l)|'s bit patterns
//   trs_train_dgrad_kernel    G(l-1) = [x(l-1) > 0] . 2^-s_l sum_{kh,kw,co} q(l)[y-kh][x-kw][co] W(l)h[kh][kw][ci][co]: a wave owns 32 input pixels x all CIN,
//                             k runs over (kh, kw, co) in that order; both fragments are 16-byte loads (q(l) is [pixel][co]; the session's own binary16
//                             copy of the kernel is [kh][kw][ci][co]: co is the fast index of both)
//   trs_train_wgrad_kernel    the weight gradient's partial sums on the matrix cores: workgroup (slice, tap) stages 64 output pixels of q(l) and the 64
//                             input pixels of x(l-1) that tap reads, [pixel][channel] as they lie, and reads transposed fragments (the reduction index, the
//                             pixel, is the slow index of both): tr_gemm_chunks (trsim_train_dev.hpp), the loop of the tail's gW1 kernel, with this
//                             kernel's loaders; wave w owns a quarter of the CIN x COUT blocks of 32 x 32.  The workgroups of tap (0, 0)
//                             also add q(l)'s rows per channel from the staged tile: the bias gradient's partial sums (256 / COUT row classes per chunk,
//                             each a running sum in pixel order, added in order at the end)
//   trs_train_cadam_kernel    thread per kernel or bias value: the slices' partial sums in slice order, times 2^-s_l; Adam; the master, the session's
//                             binary16 copy, the packed copy ConvLayer::w at pack_layer's index, the bias where the kernels read it
//   trs_train_unpack_kernel   (once, at trs_pilot_train_convs) the session's [kh][kw][ci][co] binary16 copy from the packed one
// No floating-point atomics: the split of every reduction is a fixed function of (geometry, n, CU count): trsim_train_conv.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/trsim.h"
#include "trsim_train_session.hpp"

namespace {

using namespace trsim;
using namespace trsim_train_dev;      // the vector types, the GEMM's chunk loop, Adam's update and the small rules: shared with trsim_train.hip

// ---- G7: the gradient at conv7's output ---------------------------------------------------------------------------------------------
struct G7Params {
    const u4v* w1;             // dense1's granules [G][128 outputs] of 8 features each
    const u4v* q1;             // [n padded to 64][16] granules: delta1 quantised, 128 values per frame
    const unsigned short* x7;  // [n][F]
    float* G;                  // [n][F]
    const int* sexp1; unsigned* max_bits;
    int n; size_t F;
};

// DROP: x7 is the dropped x7' of "training the pilot's tail, dropout" (the gate carries the mask: a kept positive value stays positive) and the factor is
// s 2^-s1, one exact binary32 product
template <bool DROP>
__device__ __forceinline__ void g7_body(const G7Params p, float scale)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[128 * kGwPitch];      // [output][feature of the workgroup's 128]: 40 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = blockIdx.x * 16;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int e = tid + 256 * i, o = e & 127, gi = e >> 7;
        *reinterpret_cast<u4v*>(tile + o * kGwPitch + gi * 16) = p.w1[(size_t)(g0 + gi) * 128 + o];
    }
    __syncthreads();
    h16x8 bw[8];                                                                    // the wave's 32 features x all 128 outputs
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) bw[ks] = tr_fragment(tile, lane, 32 * wave, 16 * ks);
    const float back = DROP ? scale * pow2f(-*p.sexp1) : pow2f(-*p.sexp1);
    const int h = lane >> 5;
    const size_t k = (size_t)g0 * 8 + 32 * wave + (lane & 31);                      // the lane's feature
    unsigned mx = 0;
    for (int fb = blockIdx.y * 32; fb < p.n; fb += gridDim.y * 32) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const h16x8 a = __builtin_bit_cast(h16x8, p.q1[(size_t)(fb + (lane & 31)) * 16 + 2 * ks + h]);   // (frames up to the padding: zeros)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bw[ks], acc, 0, 0, 0);
        }
        // D[frame][feature]: lane = feature, register 4 q4 + j = frame fb + 8 q4 + 4 h + j
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int fr = fb + 8 * (r >> 2) + 4 * h + (r & 3);
            if (fr < p.n) gated_store(p.G, p.x7, (size_t)fr * p.F + k, acc[r], back, mx);
        }
    }
    wave_max_bits(mx, p.max_bits, lane);
}

__global__ __launch_bounds__(256) void trs_train_g7_kernel(const G7Params p) { g7_body<false>(p, 1.0f); }
__global__ __launch_bounds__(256) void trs_train_g7_drop_kernel(const G7Params p, const float scale) { g7_body<true>(p, scale); }

// ---- G(l) as binary16 under the layer's scale ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trs_train_cquant_kernel(const float* G, const unsigned* max_bits, unsigned short* q, int* sexp, size_t count)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;                  // count is a multiple of 64
    const int s = train_scale_exponent(*max_bits);
    if (i == 0) *sexp = s;
    if (i >= count) return;
    const float up = pow2f(s);
    const f4v g = *reinterpret_cast<const f4v*>(G + i);
    unsigned short h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = __builtin_bit_cast(unsigned short, (_Float16)(g[j] * up));          // exact scaling, then round to nearest even
    *reinterpret_cast<uint2*>(q + i) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
}

// ---- the data gradient --------------------------------------------------------------------------------------------------------------------
struct DgradParams {
    const unsigned short* q;   // delta(l): [n][OH][OW][COUT]
    const unsigned short* wt;  // W(l)h: [3][3][CIN][COUT]
    const unsigned short* xin; // x(l-1): [n][IH][IW][CIN]
    float* G;                  // G(l-1): [n][IH][IW][CIN]
    const int* sexp; unsigned* max_bits;
    int IH, IW, OH, OW; long M;                // M = n IH IW input pixels
};

template <int CIN, int COUT>
__global__ __launch_bounds__(256) void trs_train_dgrad_kernel(const DgradParams p)
{
    constexpr int CB = CIN / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const long p0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (p0 >= p.M) return;                                                          // whole waves
    const long pi = p0 + (lane & 31);
    const bool valid = pi < p.M;
    const long pc = valid ? pi : p.M - 1;
    const int f = (int)(pc / (p.IH * p.IW)), rem = (int)(pc - (long)f * (p.IH * p.IW)), y = rem / p.IW, x = rem - y * p.IW;
    f32x16 acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[cb][i] = 0.0f;
    for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - 3 * kh, oy = y - kh, ox = x - kw;
        const bool ok = valid && oy >= 0 && oy < p.OH && ox >= 0 && ox < p.OW;      // a term outside delta's extent is zero
        const unsigned short* const src = p.q + (ok ? (((size_t)f * p.OH + oy) * p.OW + ox) * COUT : 0) + 8 * h;
        const unsigned short* const wsrc = p.wt + ((size_t)tap * CIN + (lane & 31)) * COUT + 8 * h;
#pragma unroll 2
        for (int ks = 0; ks < COUT / 16; ++ks) {
            u4v av = *reinterpret_cast<const u4v*>(src + 16 * ks);
            if (!ok) av = u4v{0u, 0u, 0u, 0u};
            const h16x8 a = __builtin_bit_cast(h16x8, av);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const h16x8 b = __builtin_bit_cast(h16x8, *reinterpret_cast<const u4v*>(wsrc + (size_t)cb * 32 * COUT + 16 * ks));
                acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[cb], 0, 0, 0);
            }
        }
    }
    // D[pixel][ci]: lane = ci, register 4 q4 + j = pixel p0 + 8 q4 + 4 h + j
    const float back = pow2f(-*p.sexp);
    unsigned mx = 0;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long px = p0 + 8 * (r >> 2) + 4 * h + (r & 3);
            if (px < p.M) gated_store(p.G, p.xin, (size_t)px * CIN + cb * 32 + (lane & 31), acc[cb][r], back, mx);
        }
    wave_max_bits(mx, p.max_bits, lane);
}

// ---- the weight gradient's partial sums on the matrix cores -----------------------------------------------------------------------------------
struct WgradParams {
    const u4v* x;              // x(l-1): granules [n][IH][IW][CIN / 8]
    const u4v* q;              // delta(l): granules [P][COUT / 8]
    float* part;               // [slices][3][3][CIN][COUT]
    float* bpart;              // [slices][COUT]: the bias gradient's partial sums, by the workgroups of tap (0, 0)
    int IH, IW, OH, OW; long P; int per_slice;
};

template <int CIN, int COUT>
__global__ __launch_bounds__(256) void trs_train_wgrad_kernel(const WgradParams p)
{
    constexpr int XG = CIN / 8, QG = COUT / 8;                                      // granules per pixel: a quarter of them staged per thread and chunk
    constexpr int PER = (CIN / 32) * (COUT / 32) / 4;                               // 32 x 32 blocks per wave: 1, 2 or 4, all in one block row of ci
    static_assert(kConvChunk == kGwFrames, "the split's chunk is the loop's");
    __shared__ __attribute__((aligned(16))) unsigned char tiles[2 * kGwTile];       // x's tile, then q's: [pixel][channel], 40 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slice = blockIdx.x, tap = blockIdx.y, kh = tap / 3, kw = tap - 3 * kh;
    const long first = (long)slice * p.per_slice * kConvChunk, end = min(p.P, first + (long)p.per_slice * kConvChunk);
    const int b0 = wave * PER, cib = b0 / (COUT / 32), cob0 = b0 % (COUT / 32);
    // the bias gradient rides on tap (0, 0): thread (br, bco) adds q's rows br, br + BR, .. of every chunk as they lie in the tile
    constexpr int BR = 256 / COUT;
    const int bco = tid % COUT, br = tid / COUT;
    float bsum = 0.0f;
    f32x16 acc[PER];
#pragma unroll
    for (int b = 0; b < PER; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.0f;
    tr_gemm_chunks<CIN / 32, COUT / 32>(tiles, first, end, p.P, cib, cob0, acc,
        [&](long px, int gi) {
            u4v v = u4v{0u, 0u, 0u, 0u};
            if (px < p.P) {                                                         // a pixel past the batch: a zero row
                const int f = (int)(px / (p.OH * p.OW)), rem = (int)(px - (long)f * (p.OH * p.OW)), oy = rem / p.OW, ox = rem - oy * p.OW;
                v = p.x[(((size_t)f * p.IH + oy + kh) * p.IW + ox + kw) * XG + gi];
            }
            return v;
        },
        [&](long px, int gi) { return px < p.P ? p.q[(size_t)px * QG + gi] : u4v{0u, 0u, 0u, 0u}; },
        [&](int steps) {
            if (tap == 0)
                for (int r = br; r < 16 * steps; r += BR) bsum += (float)*reinterpret_cast<const _Float16*>(tiles + kGwTile + r * kGwPitch + bco * 2);
        });
    // D[co][ci]: lane = ci, registers 4 q4 .. + 3 = co 32 cob + 8 q4 + 4 h .. + 3: one 16-byte store each
    const int h = lane >> 5;
    float* const row = p.part + (((size_t)slice * 9 + tap) * CIN + 32 * cib + (lane & 31)) * COUT;
#pragma unroll
    for (int b = 0; b < PER; ++b)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
            *reinterpret_cast<f4v*>(row + 32 * (cob0 + b) + 8 * q4 + 4 * h) = f4v{acc[b][4 * q4], acc[b][4 * q4 + 1], acc[b][4 * q4 + 2], acc[b][4 * q4 + 3]};
    if (tap == 0) {                                                                 // (the whole workgroup: the barriers are uniform)
        float* const red = reinterpret_cast<float*>(tiles);
        __syncthreads();                                                            // the last chunk has been read
        red[br * COUT + bco] = bsum;
        __syncthreads();
        if (tid < COUT) {
            float sum = 0.0f;
            for (int r = 0; r < BR; ++r) sum += red[r * COUT + tid];                // the BR row classes in order
            p.bpart[(size_t)slice * COUT + tid] = sum;
        }
    }
}

// ---- the slices added in order, Adam, and every copy of the weight ---------------------------------------------------------------------------
struct ConvAdamParams {
    const float *part, *bpart; int slices; const int* sexp;
    float *g, *m, *v, *w;          // at the layer's kernel: the bias follows it (ConvTrainLayout)
    unsigned short *wt, *pack; float* bias;
    int CIN, COUT, KK;             // KK = 9 CIN COUT
};

__global__ __launch_bounds__(256) void trs_train_cadam_kernel(const ConvAdamParams p, const AdamK k)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.KK + p.COUT) return;
    const bool is_bias = e >= p.KK;
    const float* src = is_bias ? p.bpart + (e - p.KK) : p.part + e;
    const size_t stride = is_bias ? (size_t)p.COUT : (size_t)p.KK;
    float sum = 0.0f;
    for (int s = 0; s < p.slices; ++s) sum += src[(size_t)s * stride];              // slice order
    const float g = sum * pow2f(-*p.sexp);
    p.g[e] = g;
    float mm = p.m[e], vv = p.v[e];
    const float ww = adam(g, mm, vv, p.w[e], k);
    p.m[e] = mm; p.v[e] = vv; p.w[e] = ww;
    if (is_bias) { p.bias[e - p.KK] = ww; return; }
    const unsigned short hw = f2h_pack(ww);
    p.wt[e] = hw;
    p.pack[train_conv_packed_index(p.CIN, p.COUT, e)] = hw;
}

__global__ __launch_bounds__(256) void trs_train_unpack_kernel(const unsigned short* pack, unsigned short* wt, int CIN, int COUT)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 9 * CIN * COUT) return;
    wt[e] = pack[train_conv_packed_index(CIN, COUT, e)];
}

// ---- the session's conv part (ConvSession: trsim_train_session.hpp) ---------------------------------------------------------------------------
// the instance of a kernel for one of train_conv_geom's three channel shapes (trs_pilot_train_convs refuses a pilot with any other)
template <class P>
void launch3(const ConvGeom& g, void (*k64_64)(P), void (*k64_128)(P), void (*k128_128)(P), dim3 grid, hipStream_t st, const P& p)
{
    void (*const k)(P) = g.CIN == 128 ? k128_128 : (g.COUT == 128 ? k64_128 : k64_64);
    hipLaunchKernelGGL(k, grid, dim3(256), 0, st, p);
}

// enter_session, and the session's conv part
int enter_conv(trs_env* e, TrsEnvView* v, TrsPilotTail* t, TrainSession** ts, ConvSession** s)
{
    if (int rc = enter_session(e, v, t, ts)) return rc;
    *s = (*ts)->conv.get();
    if (!*s) return trs_internal_fail(TRS_ERR_STATE, "this session trains no convolution: trs_pilot_train_convs first");
    return TRS_OK;
}

}  // namespace

int trsim::trs_train_conv_step(ConvSession& conv, trs_env* e, const TrsEnvView& v, const TrsPilotTail& t, const unsigned short* q1, const int* sexp1, int n, const AdamK& k, float x7_scale)
{
    ConvSession* const s = &conv;
    TrsPilotConvs pc;
    if (int rc = trs_internal_pilot_convs(e, v, true, &pc)) return rc;                  // x4 .. x6 where the chain kept them in LDS
    hipStream_t st = v.stream;
    unsigned* const scal = s->scal.get();
    HIPCHK(hipMemsetAsync(scal, 0, 2 * kConvTrainLayers * sizeof(unsigned), st));
    {
        G7Params gp{};
        gp.w1 = reinterpret_cast<const u4v*>(t.w1_pack); gp.q1 = reinterpret_cast<const u4v*>(q1); gp.x7 = static_cast<const unsigned short*>(t.x7);
        gp.G = s->G.get(); gp.sexp1 = sexp1; gp.max_bits = scal + 2 * 3; gp.n = n; gp.F = t.F;
        const dim3 grid(t.G / 16, std::min(8, (n + 31) / 32));
        if (x7_scale != 0.0f) hipLaunchKernelGGL(trs_train_g7_drop_kernel, grid, dim3(256), 0, st, gp, x7_scale);
        else hipLaunchKernelGGL(trs_train_g7_kernel, grid, dim3(256), 0, st, gp);
    }
    for (int j = kConvTrainLayers - 1; j >= s->lowest; --j) {
        const ConvGeom& g = s->geo[j];
        const TrsPilotConvs::Layer& pl = pc.L[j];
        const size_t count = (size_t)g.out_pixels(n) * g.COUT;
        int* const sexp = reinterpret_cast<int*>(scal + 2 * j + 1);
        hipLaunchKernelGGL(trs_train_cquant_kernel, dim3((unsigned)((count / 4 + 255) / 256)), dim3(256), 0, st, s->G.get(), scal + 2 * j, s->q[j].get(), sexp, count);
        if (j > s->lowest) {                                                            // G(l-1), from the kernel's copy before Adam moves it
            DgradParams dp{};
            dp.q = s->q[j].get(); dp.wt = s->wt.get() + s->L.off[2 * j]; dp.xin = static_cast<const unsigned short*>(pl.in); dp.G = s->G.get();
            dp.sexp = sexp; dp.max_bits = scal + 2 * (j - 1);
            dp.IH = g.IH; dp.IW = g.IW; dp.OH = g.OH; dp.OW = g.OW; dp.M = g.in_pixels(n);
            launch3(g, trs_train_dgrad_kernel<64, 64>, trs_train_dgrad_kernel<64, 128>, trs_train_dgrad_kernel<128, 128>, dim3((unsigned)((dp.M + 127) / 128)), st, dp);
        }
        if (!s->trained(j)) continue;
        const ConvSplit sp = train_conv_split(g, n, s->cu_count);
        if ((size_t)sp.slices * (g.kernel_count() + g.COUT) * sizeof(float) > s->part.bytes())      // (never: train_conv_sizes holds the most slices any n has)
            return trs_internal_fail(TRS_ERR_LIMIT, "the partial sums of this batch size do not fit the session's buffer");
        float* const part = s->part.get();
        float* const bpart = part + (size_t)sp.slices * g.kernel_count();
        WgradParams wp{};
        wp.x = static_cast<const u4v*>(pl.in); wp.q = reinterpret_cast<const u4v*>(s->q[j].get()); wp.part = part; wp.bpart = bpart;
        wp.IH = g.IH; wp.IW = g.IW; wp.OH = g.OH; wp.OW = g.OW; wp.P = sp.P; wp.per_slice = sp.per_slice;
        launch3(g, trs_train_wgrad_kernel<64, 64>, trs_train_wgrad_kernel<64, 128>, trs_train_wgrad_kernel<128, 128>, dim3(sp.slices, 9), st, wp);
        ConvAdamParams ap{};
        const size_t o = s->L.off[2 * j];
        ap.part = part; ap.bpart = bpart; ap.slices = sp.slices; ap.sexp = sexp;
        ap.g = s->g.get() + o; ap.m = s->m.get() + o; ap.v = s->v.get() + o; ap.w = s->master.get() + o;
        ap.wt = s->wt.get() + o; ap.pack = pl.w; ap.bias = pl.bias;
        ap.CIN = g.CIN; ap.COUT = g.COUT; ap.KK = (int)g.kernel_count();
        hipLaunchKernelGGL(trs_train_cadam_kernel, dim3((ap.KK + g.COUT + 255) / 256), dim3(256), 0, st, ap, k);
    }
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_train_convs(trs_env* e, uint32_t conv_mask, const float* const* h_conv_arrays)
{
    TrsEnvView v; TrsPilotTail t; TrainSession* ts;
    if (int rc = enter_session(e, &v, &t, &ts)) return rc;
    if (ts->conv) return trs_internal_fail(TRS_ERR_STATE, "trs_pilot_train_convs was already called in this session");
    if (ts->t > 0) return trs_internal_fail(TRS_ERR_STATE, "trs_pilot_train_convs comes before the session's first step");
    if (const char* why = train_conv_mask_error(conv_mask, h_conv_arrays)) return trs_internal_fail(TRS_ERR_ARG, why);
    HIPCHK(hipSetDevice(v.device));
    TrsPilotConvs pc;
    if (int rc = trs_internal_pilot_convs(e, v, false, &pc)) return rc;
    std::unique_ptr<ConvSession> s(new ConvSession());
    s->mask = conv_mask; s->lowest = train_conv_lowest(conv_mask); s->n_cap = pc.n_cap; s->cu_count = pc.cu_count; s->L = ConvTrainLayout::of();
    for (int j = 0; j < kConvTrainLayers; ++j) {
        const TrsPilotConvs::Layer& l = pc.L[j];
        s->geo[j] = train_conv_geom(j, l.IH, l.IW);
        if (l.CIN != s->geo[j].CIN || l.COUT != s->geo[j].COUT || l.OH != s->geo[j].OH || l.OW != s->geo[j].OW || l.COUT_PAD != l.COUT || l.run_pad != 3 * l.CIN / 8)
            return trs_internal_fail(TRS_ERR_LIMIT, "conv4 .. conv7 of the loaded pilot are not the 3 x 3 layers of Keras_2D_CNN");
    }
    const ConvTrainSizes z = train_conv_sizes(pc.L[0].IH, pc.L[0].IW, pc.n_cap, pc.cu_count, s->lowest);
    const size_t total = s->L.off[kConvTrainArrays];
    HIPCHK(s->master.alloc(total * sizeof(float))); HIPCHK(s->m.alloc(total * sizeof(float))); HIPCHK(s->v.alloc(total * sizeof(float))); HIPCHK(s->g.alloc(total * sizeof(float)));
    HIPCHK(s->wt.alloc(total * sizeof(unsigned short)));
    HIPCHK(s->G.alloc(z.grad_floats * sizeof(float))); HIPCHK(s->part.alloc(z.part_floats * sizeof(float)));
    for (int j = s->lowest; j < kConvTrainLayers; ++j) HIPCHK(s->q[j].alloc(z.q_halfs[j] * sizeof(unsigned short)));
    HIPCHK(s->scal.alloc(2 * kConvTrainLayers * sizeof(unsigned)));
    HIPCHK(hipStreamSynchronize(v.stream));
    HIPCHK(hipMemset(s->master.get(), 0, total * sizeof(float)));
    for (int a = 0; a < kConvTrainArrays; ++a) {
        if (!h_conv_arrays[a]) continue;
        HIPCHK(hipMemcpy(s->master.get() + s->L.off[a], h_conv_arrays[a], s->L.count(a) * sizeof(float), hipMemcpyHostToDevice));
        trs_internal_count(e, 0, (uint64_t)(s->L.count(a) * sizeof(float)));
        s->held[a] = true;
    }
    HIPCHK(hipMemsetAsync(s->m.get(), 0, total * sizeof(float), v.stream));
    HIPCHK(hipMemsetAsync(s->v.get(), 0, total * sizeof(float), v.stream));
    HIPCHK(hipMemsetAsync(s->g.get(), 0, total * sizeof(float), v.stream));
    HIPCHK(hipMemsetAsync(s->wt.get(), 0, total * sizeof(unsigned short), v.stream));
    HIPCHK(hipMemsetAsync(s->scal.get(), 0, 2 * kConvTrainLayers * sizeof(unsigned), v.stream));
    for (int j = 0; j < kConvTrainLayers; ++j) {                                        // W(l)h: the binary16 values the forward kernels read
        const ConvGeom& g = s->geo[j];
        hipLaunchKernelGGL(trs_train_unpack_kernel, dim3((unsigned)((g.kernel_count() + 255) / 256)), dim3(256), 0, v.stream, pc.L[j].w, s->wt.get() + s->L.off[2 * j], g.CIN, g.COUT);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(v.stream));
    ts->conv = std::move(s);
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_train_get_convs(trs_env* e, float* const* h_out)
{
    TrsEnvView v; TrsPilotTail t; TrainSession* ts; ConvSession* s;
    if (int rc = enter_conv(e, &v, &t, &ts, &s)) return rc;
    if (!h_out) return trs_internal_fail(TRS_ERR_ARG, "h_out is NULL");
    HIPCHK(hipSetDevice(v.device));
    HIPCHK(hipStreamSynchronize(v.stream));
    for (int a = 0; a < kConvTrainArrays; ++a) {
        if (!h_out[a] || !s->held[a]) continue;
        HIPCHK(hipMemcpy(h_out[a], s->master.get() + s->L.off[a], s->L.count(a) * sizeof(float), hipMemcpyDeviceToHost));
        trs_internal_count(e, (uint64_t)(s->L.count(a) * sizeof(float)), 0);
    }
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_train_debug_conv(trs_env* e, int layer, int which, float* h_dst, size_t n_floats)
{
    TrsEnvView v; TrsPilotTail t; TrainSession* ts; ConvSession* s;
    if (int rc = enter_conv(e, &v, &t, &ts, &s)) return rc;
    if (!ts->last_n) return trs_internal_fail(TRS_ERR_STATE, "no training step yet");
    if (layer < 0 || layer >= kConvTrainLayers) return trs_internal_fail(TRS_ERR_ARG, "layer must be 0..3 (conv4 .. conv7)");
    const ConvGeom& g = s->geo[layer];
    const size_t want = train_conv_debug_floats(g, which, ts->last_n);
    if (!want || !h_dst) return trs_internal_fail(TRS_ERR_ARG, "unknown item (TRS_CONV_DBG_*) or NULL destination");
    if (n_floats != want) return trs_internal_fail(TRS_ERR_ARG, "size mismatch");
    if ((which == TRS_CONV_DBG_DELTA || which == TRS_CONV_DBG_SCALE_EXP) && layer < s->lowest)
        return trs_internal_fail(TRS_ERR_ARG, "back-propagation stops at the lowest trained layer: no delta below it");
    HIPCHK(hipSetDevice(v.device));
    HIPCHK(hipStreamSynchronize(v.stream));
    const size_t ok = s->L.off[2 * layer], ob = s->L.off[2 * layer + 1];
    const float* src = nullptr;
    switch (which) {
    case TRS_CONV_DBG_GW: src = s->g.get() + ok; break;
    case TRS_CONV_DBG_GB: src = s->g.get() + ob; break;
    case TRS_CONV_DBG_MW: src = s->m.get() + ok; break;
    case TRS_CONV_DBG_VW: src = s->v.get() + ok; break;
    case TRS_CONV_DBG_MB: src = s->m.get() + ob; break;
    case TRS_CONV_DBG_VB: src = s->v.get() + ob; break;
    default: break;
    }
    if (src) {
        HIPCHK(hipMemcpy(h_dst, src, want * sizeof(float), hipMemcpyDeviceToHost));
        return TRS_OK;
    }
    int sexp = 0;
    HIPCHK(hipMemcpy(&sexp, s->scal.get() + 2 * layer + 1, sizeof sexp, hipMemcpyDeviceToHost));
    if (which == TRS_CONV_DBG_SCALE_EXP) { h_dst[0] = (float)sexp; return TRS_OK; }
    if (which == TRS_CONV_DBG_DELTA) {
        std::vector<unsigned short> q(want);
        HIPCHK(hipMemcpy(q.data(), s->q[layer].get(), want * 2, hipMemcpyDeviceToHost));
        const float back = train_pow2(-sexp);
        for (size_t i = 0; i < want; ++i) h_dst[i] = widen_h(q[i]) * back;
        return TRS_OK;
    }
    // TRS_CONV_DBG_PACK: the granules the forward kernels read -> [3][3][CIN][COUT]
    TrsPilotConvs pc;
    if (int rc = trs_internal_pilot_convs(e, v, false, &pc)) return rc;
    std::vector<unsigned short> pack(want);
    HIPCHK(hipMemcpy(pack.data(), pc.L[layer].w, want * 2, hipMemcpyDeviceToHost));
    for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw)
            for (int ci = 0; ci < g.CIN; ++ci)
                for (int co = 0; co < g.COUT; ++co)
                    h_dst[((size_t)(kh * 3 + kw) * g.CIN + ci) * g.COUT + co] = widen_h(pack[train_conv_packed_index(g, kh, kw, ci, co)]);
    return TRS_OK;
}
