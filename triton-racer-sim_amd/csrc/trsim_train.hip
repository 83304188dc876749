// trsim_train.hip — training the pilot's tail on the device (include/trsim_spec.h, "training the pilot's tail"): dense1 -> dense2 -> dense3 -> output_layer
// of a loaded 22-array pilot move by Adam on 'mse', conv1 .. conv7 stay as loaded.  A step is the forward pass of trs_pilot_forward up to dense1's split-K
// slabs (trsim_pilot.hip runs it: the kernels that drive, unchanged) and six kernels of this file, all on the handle's stream:
//   trs_train_tail_kernel     one wave per frame: the slabs added in slice order, dense2 -> dense3 -> output as trs_pilot_tail_kernel computes them (restated:
//                             the same chains, so the same bits), delta4 .. delta1 in binary32, the integer maximum of |delta1|'s bit patterns
//   trs_train_small_kernel    one thread per small weight, bias and the loss: sums over the frames in ascending order (6,478 threads)
//   trs_train_quant_kernel    delta1 -> binary16 under the batch's power-of-two scale, [n padded to 64][128], zeros in the padding
//   trs_train_gw1_kernel      dense1's weight gradient on the matrix cores: gW1[k][o] = 2^-s sum_i x7_i[k] q_i[o].  The reduction index is the frame, the slow
//                             index of both operands as stored, so both tiles go to LDS as they lie in memory ([frame][value], 64 frames per chunk) and
//                             every MFMA fragment is two ds_read_b64_tr_b16.  A workgroup owns 128 features for the whole batch (wave w: features 32 w ..
//                             32 w + 31 x the four 32-output blocks: four accumulators), so the order of the sum is fixed.  Row pitch 320 B: rows q = 0..3
//                             of a transposed read start 16 banks apart, the two 16-lane groups of a half 8 apart, the four lanes of a row 2 apart —
//                             no two lanes of a 32-lane half on one bank.  The chunk loop is tr_gemm_chunks (trsim_train_dev.hpp), the one the
//                             convolutions' weight gradient runs.
//   trs_train_adam1_kernel    Adam over dense1's kernel: one thread per (granule, output) moves 8 masters and writes the binary16 granule the dense
//                             kernel reads; trs_train_adam_kernel: the other seven arrays, written to the master and where the tail kernels read them
// With trs_pilot_train_dropout (include/trsim_spec.h, "training the pilot's tail, dropout"; the draws: trsim_dropout.hpp) a site that drops takes
//   trs_train_drop7_kernel    site 0: conv7's activation masked and scaled where it lies, between conv7 and dense1 (trsim_pilot.hip calls it through a hook);
//                             the gW1 GEMM and G7's gate then read the dropped values
//   trs_train_tail_drop_kernel   sites 1 .. 3: the tail kernel's body with the forward scaling and the backward mask; it stores a'(l), which the small
//                             kernel reads where it read z(l) (relu(a') is a' bit for bit)
// and a site that does not keeps the kernels and the bits above.
// The session of a 28-array pilot, cnn_2d_speed_as_feature (include/trsim_spec.h, "training the pilot's tail, side branch"; trs_pilot_train_begin_ex,
// trs_pilot_train_step_ex), also trains the branch speed / 20 -> feature1 -> feature2 -> feature3 and dense1's 16 rows behind the flatten (W1Y).  It keeps the
// kernels above for everything they cover — the flatten rows of dense1 and arrays 1 .. 7, which its layout puts where those kernels are told — and adds
//   trs_train_tail_side_kernel, trs_train_tail_side_drop_kernel   the tail kernel's body with SIDE: the branch on 1 -> 4 -> 8 -> 16 lanes through LDS first,
//                             W1Y's rows added to z1 behind the slabs as trs_pilot_tail_ex_kernel adds them (the same chains, the same bits), delta-y3 ..
//                             delta-y1 behind delta1; stored per frame: fin, y1 .. y3, delta-y1 .. delta-y3 and the products fin delta-y1
//   trs_train_small_side_kernel   behind trs_train_small_kernel: 1,792 values (gW1Y 1,600; feature3 .. feature1: 128 + 32 + 4 weights, 16 + 8 + 4 biases), one
//                             thread each over the frames in ascending order, by the same grad_w and grad_b
//   trs_train_adam_side_kernel    the same Adam over those seven arrays, written to the master and to the slots of the tail's blob the ex tail reads
// A 22-array step launches none of them and its kernels are the code objects they were (scripts/kernel_diff.py).
// No floating-point atomics: two runs of a step agree bit for bit.  The rules that need no GPU (config, alpha_t, the scale's exponent, the buffers' layout)
// are trsim_train.hpp; the session, which trsim_train_conv.hip's entry points open as well, is trsim_train_session.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/trsim.h"
#include "trsim_train_session.hpp"

namespace {

using namespace trsim;
using namespace trsim_train_dev;      // the vector types, the GEMM's chunk loop, Adam's update and the small rules: shared with trsim_train_conv.hip

// ---- forward behind dense1's slabs, and backward through the three small layers: one wave per frame -------------------------------
struct TailTrainParams {
    const float* h1; int slices; size_t stride;          // dense1's slabs (bias in slice 0)
    const float *w2, *b2, *w3, *b3, *w4, *b4;            // Keras layouts [IN][OUT]
    const float* y; int n;
    float *out, *z1, *z2, *z3, *d1, *d2, *d3, *d4;
    unsigned* max_bits;                                  // zeroed before the launch
};

// Dropout at sites 1 .. 3 (include/trsim_spec.h, "training the pilot's tail, dropout"): the step's key Dt, the threshold and scale per site (a site that
// is off: T = 0, s = 1, which keep every unit and every bit) and where a'(l), what the next layer read, is kept for the small gradients
struct TailDropParams {
    uint64_t Dt; uint32_t T[3]; float s[3];
    float *a1, *a2, *a3;
};

// The side branch of a 28-array pilot (include/trsim_spec.h, "training the pilot's tail, side branch"): the feature, the branch's weights and dense1's rows
// behind the flatten where trs_pilot_tail_ex_kernel reads them, and where fin, y1 .. y3 and delta-y1 .. delta-y3 are kept for the small gradients
struct TailSideParams {
    const float* fin;                                    // [n][1]: speed / 20 as the loader delivers it
    const float *w1y, *f1w, *f1b, *f2w, *f2b, *f3w, *f3b;
    float *kfin, *y1, *y2, *y3, *dy1, *dy2, *dy3, *pf1;   // pf1 [n][4]: fin delta-y1, the terms of feature1's kernel gradient
};

// fin -> y1 -> y2 -> y3 on 1, 4, 8, 16 lanes of the frame's wave: each unit one fmaf chain from its bias, k ascending, then the ReLU, which is what dense_small
// (trsim_pilot_tail.hpp) computes for these widths.  Returns the wave's y1 | y2 | y3 in LDS (y3 at + 12).
__device__ __forceinline__ float* side_forward(const TailSideParams& sd, int i, int lane, int wv)
{
    __shared__ float sy[4][32];                          // y1 at 0, y2 at 4, y3 at 12, fin at 28
    float* const y = sy[wv];
    if (lane == 0) { const float f = sd.fin[i]; y[28] = f; sd.kfin[i] = f; }
    __builtin_amdgcn_wave_barrier();
    if (lane < 4) {
        float s = fmaf(y[28], sd.f1w[lane], sd.f1b[lane]);
        s = s > 0.f ? s : 0.f;
        y[lane] = s; sd.y1[(size_t)i * 4 + lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 8) {
        float s = sd.f2b[lane];
#pragma unroll
        for (int k = 0; k < 4; ++k) s = fmaf(y[k], sd.f2w[k * 8 + lane], s);
        s = s > 0.f ? s : 0.f;
        y[4 + lane] = s; sd.y2[(size_t)i * 8 + lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 16) {
        float s = sd.f3b[lane];
#pragma unroll
        for (int k = 0; k < 8; ++k) s = fmaf(y[4 + k], sd.f3w[k * 16 + lane], s);
        s = s > 0.f ? s : 0.f;
        y[12 + lane] = s; sd.y3[(size_t)i * 16 + lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    return y;
}

// delta-y3[k] = [y3[k] > 0] sum_o W1Y[k][o] delta1[o], then delta-y2 and delta-y1 through feature3 and feature2: lane k owns row k, one fmaf chain from 0, the
// output index ascending, as the tail's own deltas.  delta1 is (da, db) of the lanes; the weights of 25 terms are requested together.
__device__ __forceinline__ void side_backward(const TailSideParams& sd, const float* y, float da, float db, bool two, int i, int lane, int wv)
{
    __shared__ float e1[4][100], ey[4][24];              // delta1; delta-y3 at 0, delta-y2 at 16
    e1[wv][lane] = da;
    if (two) e1[wv][lane + 64] = db;
    __builtin_amdgcn_wave_barrier();
    if (lane < 16) {
        float s = 0.0f;
        for (int o0 = 0; o0 < 100; o0 += 25) {
            float w[25];
#pragma unroll
            for (int j = 0; j < 25; ++j) w[j] = sd.w1y[lane * 100 + o0 + j];
#pragma unroll
            for (int j = 0; j < 25; ++j) s = fmaf(w[j], e1[wv][o0 + j], s);
        }
        s = y[12 + lane] > 0.f ? s : 0.0f;
        sd.dy3[(size_t)i * 16 + lane] = s; ey[wv][lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 8) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s = fmaf(sd.f3w[lane * 16 + k], ey[wv][k], s);
        s = y[4 + lane] > 0.f ? s : 0.0f;
        sd.dy2[(size_t)i * 8 + lane] = s; ey[wv][16 + lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 4) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s = fmaf(sd.f2w[lane * 8 + k], ey[wv][16 + k], s);
        s = y[lane] > 0.f ? s : 0.0f;
        sd.dy1[(size_t)i * 4 + lane] = s; sd.pf1[(size_t)i * 4 + lane] = y[28] * s;
    }
}

// The four kernels share their body as text (trsim_train_tail_body.hpp says why); the LDS arrays are each kernel's own
__global__ __launch_bounds__(256) void trs_train_tail_kernel(const TailTrainParams p)
{
    __shared__ float s1[4][100], s2[4][50], s3[4][25], e4[4][2], e3[4][25], e2[4][50];
    constexpr bool DROP = false; const TailDropParams dp{};
    constexpr bool SIDE = false; const TailSideParams sd{};
#include "trsim_train_tail_body.hpp"
}
__global__ __launch_bounds__(256) void trs_train_tail_drop_kernel(const TailTrainParams p, const TailDropParams dp)
{
    __shared__ float s1[4][100], s2[4][50], s3[4][25], e4[4][2], e3[4][25], e2[4][50];
    constexpr bool DROP = true;
    constexpr bool SIDE = false; const TailSideParams sd{};
#include "trsim_train_tail_body.hpp"
}
__global__ __launch_bounds__(256) void trs_train_tail_side_kernel(const TailTrainParams p, const TailSideParams sd)
{
    __shared__ float s1[4][100], s2[4][50], s3[4][25], e4[4][2], e3[4][25], e2[4][50];
    constexpr bool DROP = false; const TailDropParams dp{};
    constexpr bool SIDE = true;
#include "trsim_train_tail_body.hpp"
}
__global__ __launch_bounds__(256) void trs_train_tail_side_drop_kernel(const TailTrainParams p, const TailDropParams dp, const TailSideParams sd)
{
    __shared__ float s1[4][100], s2[4][50], s3[4][25], e4[4][2], e3[4][25], e2[4][50];
    constexpr bool DROP = true;
    constexpr bool SIDE = true;
#include "trsim_train_tail_body.hpp"
}

// ---- dropout at site 0: conv7's activation masked and scaled in place, between conv7 and dense1 -------------------------------------
// x7'[f] = keep ? binary16_rn(min((float)x7[f] s, 65504)) : +0.  One lane per 16-byte unit of 8 features and one wave per workgroup: workgroup (x, y) owns
// units 64 x .. 64 x + 63 of frames y, y + gridDim.y, .., so a wave's loads and stores cover one contiguous run of 1 KB, the frame's key is the same for the
// whole wave (no lane divides a flat index by G) and a lane pays the two words of its unit (four fields each).  No LDS, no atomics.
__global__ __launch_bounds__(64) void trs_train_drop7_kernel(u4v* x7, int n, int G, uint64_t Dt, uint32_t T, float s)
{
    const int u = blockIdx.x * 64 + threadIdx.x;
    if (u >= G) return;
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const uint64_t key = dropout_frame_key(Dt, 0u, (uint32_t)i);
        const uint64_t w[2] = {dropout_word(key, 2u * (uint32_t)u), dropout_word(key, 2u * (uint32_t)u + 1u)};
        u4v* const at = x7 + (size_t)i * (size_t)G + u;
        const h16x8 x = __builtin_bit_cast(h16x8, *at);
        h16x8 y;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            y[j] = dropout_keep_field(w[j >> 2], (uint32_t)j, T) ? (_Float16)fminf((float)x[j] * s, 65504.0f) : (_Float16)0.0f;
        *at = __builtin_bit_cast(u4v, y);
    }
}

// ---- the small gradients and the loss: one thread per value, the frames in ascending order ----------------------------------------
struct SmallGradParams {
    const float *z1, *z2, *z3, *d1, *d2, *d3, *d4, *out, *y;
    float* g; size_t off[kTrainArrays + 1];              // the gradient buffer and its layout (TrainLayout)
    float *loss, *loss_user; int n;
};
constexpr int kSmallGradThreads = 100 + 5000 + 50 + 1250 + 25 + 50 + 2 + 1;   // gb1, gW2, gb2, gW3, gb3, gW4, gb4, the loss

// The loads of kGradAhead frames are requested together and the additions then run in frame order: the sum is the plain ascending one, but a load's round trip
// to L2 is paid once per kGradAhead frames and not once per frame (one frame at a time measured 364 us per step at 1024 frames: profiles/r31_train_tail.txt)
constexpr int kGradAhead = 32;
// KERNEL: one instance per kernel that calls them (0: trs_train_small_kernel, 1: trs_train_small_side_kernel).  The compiler propagates the widths its callers
// pass into a function before it inlines it; with one instance for both kernels the second kernel's widths changed the first one's code object.
template <int KERNEL = 0>
__device__ __forceinline__ float grad_w(const float* z, int nin, const float* d, int nout, int t, int n)
{
    const int k = t / nout, o = t - k * nout;
    const float *pz = z + k, *pd = d + o;
    float s = 0.0f;
    int i = 0;
    for (; i + kGradAhead <= n; i += kGradAhead) {
        float a[kGradAhead], b[kGradAhead];
#pragma unroll
        for (int j = 0; j < kGradAhead; ++j) { a[j] = pz[(size_t)(i + j) * nin]; b[j] = pd[(size_t)(i + j) * nout]; }
#pragma unroll
        for (int j = 0; j < kGradAhead; ++j) s = fmaf(a[j] > 0.f ? a[j] : 0.f, b[j], s);
    }
    for (; i < n; ++i) { const float a = pz[(size_t)i * nin]; s = fmaf(a > 0.f ? a : 0.f, pd[(size_t)i * nout], s); }
    return s;
}
template <int KERNEL = 0>
__device__ __forceinline__ float grad_b(const float* d, int nout, int o, int n)
{
    const float* pd = d + o;
    float s = 0.0f;
    int i = 0;
    for (; i + kGradAhead <= n; i += kGradAhead) {
        float b[kGradAhead];
#pragma unroll
        for (int j = 0; j < kGradAhead; ++j) b[j] = pd[(size_t)(i + j) * nout];
#pragma unroll
        for (int j = 0; j < kGradAhead; ++j) s += b[j];
    }
    for (; i < n; ++i) s += pd[(size_t)i * nout];
    return s;
}

__global__ __launch_bounds__(64) void trs_train_small_kernel(const SmallGradParams p)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 100) { p.g[p.off[1] + t] = grad_b(p.d1, 100, t, p.n); return; }
    t -= 100;
    if (t < 5000) { p.g[p.off[2] + t] = grad_w(p.z1, 100, p.d2, 50, t, p.n); return; }
    t -= 5000;
    if (t < 50) { p.g[p.off[3] + t] = grad_b(p.d2, 50, t, p.n); return; }
    t -= 50;
    if (t < 1250) { p.g[p.off[4] + t] = grad_w(p.z2, 50, p.d3, 25, t, p.n); return; }
    t -= 1250;
    if (t < 25) { p.g[p.off[5] + t] = grad_b(p.d3, 25, t, p.n); return; }
    t -= 25;
    if (t < 50) { p.g[p.off[6] + t] = grad_w(p.z3, 25, p.d4, 2, t, p.n); return; }
    t -= 50;
    if (t < 2) { p.g[p.off[7] + t] = grad_b(p.d4, 2, t, p.n); return; }
    t -= 2;
    if (t == 0) {                                        // loss = sum_i sum_j (out - y)^2 / (2 n)
        float s = 0.0f;
        int i = 0;
        for (; i + kGradAhead <= 2 * p.n; i += kGradAhead) {
            float a[kGradAhead], b[kGradAhead];
#pragma unroll
            for (int j = 0; j < kGradAhead; ++j) { a[j] = p.out[i + j]; b[j] = p.y[i + j]; }
#pragma unroll
            for (int j = 0; j < kGradAhead; ++j) { const float e = a[j] - b[j]; s = fmaf(e, e, s); }
        }
        for (; i < 2 * p.n; ++i) { const float e = p.out[i] - p.y[i]; s = fmaf(e, e, s); }
        s = s / (float)(2 * p.n);
        *p.loss = s;
        if (p.loss_user) *p.loss_user = s;
    }
}

// The side branch's small gradients (a 28-array session), launched behind trs_train_small_kernel: gW1Y[k][o] = sum_i y3_i[k] delta1_i[o] (rows F .. F + 15 of
// dense1's kernel, which the GEMM over x7 does not reach), kernel and bias of feature1 .. feature3.  One thread per value, the frames in ascending order, by
// grad_w and grad_b.  feature1's input is the feature itself, which may be negative, and grad_w gates its first operand: the tail kernel stores the products
// fin_i delta-y1_i[j], each rounded once, and grad_b adds them.
struct SmallSideParams {
    const float *pf1, *y1, *y2, *y3, *d1, *dy1, *dy2, *dy3;   // pf1: the products fin delta-y1 [n][4]
    float* g; size_t at[7];                              // the gradient buffer and where the seven side arrays lie in it (TrainSession::side_array)
    int n;
};
__global__ __launch_bounds__(64) void trs_train_small_side_kernel(const SmallSideParams p)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < kSideRows * 100) { p.g[p.at[0] + t] = grad_w<1>(p.y3, kSideRows, p.d1, 100, t, p.n); return; }
    t -= kSideRows * 100;
    if (t < 4) { p.g[p.at[1] + t] = grad_b<1>(p.pf1, 4, t, p.n); return; }
    t -= 4;
    if (t < 4) { p.g[p.at[2] + t] = grad_b<1>(p.dy1, 4, t, p.n); return; }
    t -= 4;
    if (t < 32) { p.g[p.at[3] + t] = grad_w<1>(p.y1, 4, p.dy2, 8, t, p.n); return; }
    t -= 32;
    if (t < 8) { p.g[p.at[4] + t] = grad_b<1>(p.dy2, 8, t, p.n); return; }
    t -= 8;
    if (t < 128) { p.g[p.at[5] + t] = grad_w<1>(p.y2, 8, p.dy3, 16, t, p.n); return; }
    t -= 128;
    if (t < 16) p.g[p.at[6] + t] = grad_b<1>(p.dy3, 16, t, p.n);
}

// ---- delta1 as binary16 under the batch's scale ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void trs_train_quant_kernel(const float* d1, const unsigned* max_bits, unsigned short* q, int* sexp, int n)
{
    const int i = blockIdx.x, o = threadIdx.x;           // grid: n padded to 64 frames
    const int s = train_scale_exponent(*max_bits);
    if (i == 0 && o == 0) *sexp = s;
    _Float16 h = (_Float16)0.0f;
    if (i < n && o < 100) h = (_Float16)(d1[(size_t)i * 100 + o] * pow2f(s));   // exact scaling, then round to nearest even
    q[(size_t)i * 128 + o] = __builtin_bit_cast(unsigned short, h);
}

// ---- dense1's weight gradient on the matrix cores ---------------------------------------------------------------------------------------
struct Gw1Params {
    const u4v* x7;             // conv7's activation: binary16 [n][G] granules
    const u4v* q;              // [n_pad][16] granules: delta1 quantised, 128 values per frame
    float* gw1;                // [F][100]
    const int* sexp;
    int n, n_pad, G;
};
// (the LDS chunk of 64 frames, its row pitch of 320 B, the transposed fragment read and the chunk loop tr_gemm_chunks: trsim_train_dev.hpp)
__global__ __launch_bounds__(256) void trs_train_gw1_kernel(const Gw1Params p)
{
    __shared__ __attribute__((aligned(16))) unsigned char tiles[2 * kGwTile];   // x7's tile, then q's: 40 KB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = blockIdx.x * 16;                                         // the tile's first granule: features 128 blockIdx.x ..
    // 16 granules per frame of both operands: four staged granules per thread; wave w owns features 32 w .. against the four 32-output blocks
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.0f;
    tr_gemm_chunks<4, 4>(tiles, 0, p.n_pad, p.n, wave, 0, acc,
        [&](int fr, int gi) {
            u4v v = p.x7[(size_t)min(fr, p.n - 1) * p.G + g0 + gi];          // a frame past the batch: a valid address, a zero fragment
            if (fr >= p.n) v = u4v{0u, 0u, 0u, 0u};
            return v;
        },
        [&](int fr, int gi) { return p.q[(size_t)fr * 16 + gi]; },           // (padded with zeros up to n_pad)
        [](int) {});
    // D[output][feature]: lane = feature, registers 4 q4 .. + 3 = outputs 32 b + 8 q4 + 4 h .. + 3: one 16-byte store each, scaled back by 2^-s (exact)
    const float back = pow2f(-*p.sexp);
    const int h = lane >> 5;
    float* const row = p.gw1 + ((size_t)g0 * 8 + 32 * wave + (lane & 31)) * 100;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int o = 32 * b + 8 * q4 + 4 * h;
            if (o < 100) *reinterpret_cast<f4v*>(row + o) = f4v{acc[b][4 * q4] * back, acc[b][4 * q4 + 1] * back, acc[b][4 * q4 + 2] * back, acc[b][4 * q4 + 3] * back};
        }
}

// ---- Adam in Keras's form -----------------------------------------------------------------------------------------------------------------
// (AdamK, the update `adam` and the packed rounding f2h_pack: trsim_train_dev.hpp)
// dense1's kernel: thread (granule, output) owns master rows 8 granule .. + 7 of column `output` and the granule [granule][output][8] of the pack
__global__ __launch_bounds__(256) void trs_train_adam1_kernel(const float* g, float* m, float* v, float* w, unsigned short* pack, int G, const AdamK k)
{
    const int gid = blockIdx.x * 256 + threadIdx.x, gr = gid >> 7, co = gid & 127;
    if (gr >= G || co >= 100) return;                    // columns 100 .. 127 of the pack stay zero
    unsigned short h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const size_t e = ((size_t)gr * 8 + j) * 100 + co;
        float mm = m[e], vv = v[e];
        const float ww = adam(g[e], mm, vv, w[e], k);
        m[e] = mm; v[e] = vv; w[e] = ww;
        h[j] = f2h_pack(ww);
    }
    const u4v out = {h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16)};
    *reinterpret_cast<u4v*>(pack + ((size_t)gr * 128 + co) * 8) = out;
}

// arrays 1 .. 7 (dense1's bias, then the small layers): thread per value; the new weight goes to the master and to where the tail kernels read it
struct AdamSmallParams { size_t off[kTrainArrays + 1]; float* live[kTrainArrays]; unsigned mask; };
__global__ __launch_bounds__(256) void trs_train_adam_kernel(const float* g, float* m, float* v, float* w, const AdamSmallParams p, const AdamK k)
{
    const size_t e = p.off[1] + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= p.off[kTrainArrays]) return;
    int a = 1;
    while (e >= p.off[a + 1]) ++a;
    if (!((p.mask >> (a >> 1)) & 1u)) return;
    float mm = m[e], vv = v[e];
    const float ww = adam(g[e], mm, vv, w[e], k);
    m[e] = mm; v[e] = vv; w[e] = ww;
    p.live[a][e - p.off[a]] = ww;
}

// the seven side arrays of a 28-array session (W1Y, then kernel and bias of feature1 .. feature3): thread per value, the same rule; the new weight goes to the
// master and to the slot of the tail's blob that trs_pilot_tail_ex_kernel and the side tail kernels read.  bit[j]: the train mask's bit that moves array j.
struct AdamSideParams { size_t at[7]; int first[8]; float* live[7]; int bit[7]; unsigned mask; };
__global__ __launch_bounds__(256) void trs_train_adam_side_kernel(const float* g, float* m, float* v, float* w, const AdamSideParams p, const AdamK k)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.first[7]) return;
    int j = 0;
    while (t >= p.first[j + 1]) ++j;
    if (!((p.mask >> p.bit[j]) & 1u)) return;
    const size_t e = p.at[j] + (size_t)(t - p.first[j]);
    float mm = m[e], vv = v[e];
    const float ww = adam(g[e], mm, vv, w[e], k);
    m[e] = mm; v[e] = vv; w[e] = ww;
    p.live[j][t - p.first[j]] = ww;
}

// ---- the session (trsim_train_session.hpp) ------------------------------------------------------------------------------------------------
// where the tail kernels read arrays 1 .. 7; dense1's kernel, array 0, is read as the pack
void tail_live(const TrsPilotTail& t, float* (&live)[kTrainArrays])
{
    float* const at[kTrainArrays] = {nullptr, t.b1, t.w2, t.b2, t.w3, t.b3, t.w4, t.b4};
    std::memcpy(live, at, sizeof at);
}

}  // namespace

void trs_train_free(void* session) { delete static_cast<TrainSession*>(session); }

TRS_EXPORT void trs_default_train_config(trs_train_config* cfg)
{
    if (cfg) trsim::train_defaults(cfg);
}

namespace {

// trs_pilot_train_begin (ex false: 8 arrays, 22-array pilots alone) and trs_pilot_train_begin_ex: the session of the loaded pilot over n_arrays trained arrays
int begin_session(trs_env* e, const trs_train_config* cfg_or_null, const float* const* h_arrays, int n_arrays, bool ex)
{
    if (n_arrays != kTrainArrays && n_arrays != kTrainSideArrays) return trs_internal_fail(TRS_ERR_ARG, "n_arrays must be 8 (a 22-array pilot) or 14 (a 28-array pilot)");
    trs_train_config cfg;
    trsim::train_defaults(&cfg);
    if (n_arrays == kTrainSideArrays) cfg.train_mask = kTrainMaskAllSide;
    if (cfg_or_null) {
        if (const char* why = trsim::train_config_error_ex(cfg_or_null, n_arrays)) return trs_internal_fail(TRS_ERR_ARG, why);
        cfg = *cfg_or_null;
    }
    if (!h_arrays || !h_arrays[0]) return trs_internal_fail(TRS_ERR_ARG, "h_tail_arrays[0], dense1's kernel as trs_pilot_load got it, is NULL");
    TrsEnvView v; TrsPilotTail t;
    if (int rc = trs_internal_pilot_tail(e, &v, &t)) return rc;
    if (!ex && t.arch != TRS_PILOT_SPD_CTL)
        return trs_internal_fail(TRS_ERR_LIMIT, "the tail of a 28- or 42-array pilot (cnn_2d_speed_as_feature, cnn_2d_full_house) is not trained by this call: 22 arrays only "
                                                "(trs_pilot_train_begin_ex opens the session of a 28-array pilot)");
    bool limit = false;
    if (const char* why = trsim::train_count_error(t.arch == TRS_PILOT_SPD_CTL ? 22 : (t.arch == TRS_PILOT_SPD_FTR ? 28 : 42), n_arrays, &limit))
        return trs_internal_fail(limit ? TRS_ERR_LIMIT : TRS_ERR_ARG, why);
    if (*t.train) return trs_internal_fail(TRS_ERR_STATE, "a training session is already open on this pilot: trs_pilot_train_end first");
    HIPCHK(hipSetDevice(v.device));
    std::unique_ptr<TrainSession> s(new TrainSession());
    s->cfg = cfg; s->F = t.F; s->n_cap = t.n_cap; s->L = TrainLayout::of(t.F); s->n_arrays = n_arrays;
    if (s->has_side()) {
        s->SL = TrainSideLayout::of(t.F); s->L = s->SL.tail();
        HIPCHK(s->side.alloc((size_t)t.n_cap * side_frame_floats() * sizeof(float)));
    }
    const size_t total = s->total() * sizeof(float), n_pad = trsim::align_up((size_t)t.n_cap, kGwFrames);
    HIPCHK(s->master.alloc(total)); HIPCHK(s->m.alloc(total)); HIPCHK(s->v.alloc(total)); HIPCHK(s->g.alloc(total));
    HIPCHK(s->fwd.alloc((size_t)t.n_cap * train_frame_floats() * sizeof(float)));
    HIPCHK(s->q.alloc(n_pad * 128 * sizeof(unsigned short)));
    HIPCHK(s->scal.alloc(4 * sizeof(unsigned)));
    HIPCHK(hipStreamSynchronize(v.stream));
    HIPCHK(hipMemcpy(s->master.get(), h_arrays[0], s->L.count(0) * sizeof(float), hipMemcpyHostToDevice));
    trs_internal_count(e, 0, (uint64_t)(s->L.count(0) * sizeof(float)));
    float* live[kTrainArrays];
    tail_live(t, live);
    for (int a = 1; a < kTrainArrays; ++a)
        HIPCHK(hipMemcpyAsync(s->master.get() + s->L.off[a], live[a], s->L.count(a) * sizeof(float), hipMemcpyDeviceToDevice, v.stream));
    for (int j = 1; s->has_side() && j < 7; ++j)                               // feature1 .. feature3 (W1Y came with dense1's kernel)
        HIPCHK(hipMemcpyAsync(s->master.get() + s->side_array(j), t.side[j], kSideArrayCount[j] * sizeof(float), hipMemcpyDeviceToDevice, v.stream));
    HIPCHK(hipMemsetAsync(s->m.get(), 0, total, v.stream));
    HIPCHK(hipMemsetAsync(s->v.get(), 0, total, v.stream));
    HIPCHK(hipMemsetAsync(s->g.get(), 0, total, v.stream));
    if (s->has_side()) HIPCHK(hipMemsetAsync(s->side.get(), 0, s->side.bytes(), v.stream));
    HIPCHK(hipMemsetAsync(s->scal.get(), 0, 4 * sizeof(unsigned), v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    *t.train = s.release();
    return TRS_OK;
}

// trs_pilot_train_step (ex false: no features, 22-array sessions alone) and trs_pilot_train_step_ex
int train_step(trs_env* e, const uint8_t* d_frames, const float* d_features, const float* d_labels, int n, float* d_loss_or_null, bool ex)
{
    TrsEnvView v; TrsPilotTail t; TrainSession* s;
    if (int rc = enter_session(e, &v, &t, &s)) return rc;
    if (!ex && s->has_side()) return trs_internal_fail(TRS_ERR_ARG, "a 28-array session also reads the feature: use trs_pilot_train_step_ex");
    if (n < 1 || n > s->n_cap) return trs_internal_fail(TRS_ERR_ARG, "n must be in [1, n_envs]");
    if (!d_frames || !d_labels) return trs_internal_fail(TRS_ERR_ARG, "d_frames or d_labels is NULL");
    if (s->has_side() && !d_features) return trs_internal_fail(TRS_ERR_ARG, "d_features is NULL: a 28-array session reads float[n][1], speed / 20 per frame");
    HIPCHK(hipSetDevice(v.device));
    const DropSession& dr = s->drop;
    const uint64_t Dt = dropout_step_key(dr.seed, (uint64_t)(s->t + 1));                  // (read only where a site is on)
    struct Drop7 { hipStream_t st; int G; uint64_t Dt; uint32_t T; float s; } d7{v.stream, t.G, Dt, dr.T, dr.s};
    const TrsPilotX7Hook hook{[](void* arg, void* x7, int frames) -> int {
        const Drop7& d = *static_cast<const Drop7*>(arg);
        hipLaunchKernelGGL(trs_train_drop7_kernel, dim3((d.G + 63) / 64, std::min(frames, 65535)), dim3(64), 0, d.st, static_cast<u4v*>(x7), frames, d.G, d.Dt, d.T, d.s);
        return TRS_OK;
    }, &d7};
    // conv1 .. conv7 and dense1, by the kernels that drive; with site 0 on, x7 is masked where it lies before dense1 reads it
    if (int rc = trs_internal_pilot_dense_forward(e, v, d_frames, n, &t, dr.site(0) ? &hook : nullptr)) return rc;
    hipStream_t st = v.stream;
    unsigned* const scal = s->scal.get();
    HIPCHK(hipMemsetAsync(scal, 0, sizeof(unsigned), st));
    TailTrainParams tp{};
    tp.h1 = t.slab; tp.slices = t.slices; tp.stride = t.slab_stride;
    tp.w2 = t.w2; tp.b2 = t.b2; tp.w3 = t.w3; tp.b3 = t.b3; tp.w4 = t.w4; tp.b4 = t.b4;
    tp.y = d_labels; tp.n = n;
    tp.out = s->item(TRS_TRAIN_DBG_OUT); tp.z1 = s->item(TRS_TRAIN_DBG_Z1); tp.z2 = s->item(TRS_TRAIN_DBG_Z2); tp.z3 = s->item(TRS_TRAIN_DBG_Z3);
    tp.d1 = s->item(TRS_TRAIN_DBG_DELTA1); tp.d2 = s->item(TRS_TRAIN_DBG_DELTA2); tp.d3 = s->item(TRS_TRAIN_DBG_DELTA3); tp.d4 = s->item(TRS_TRAIN_DBG_DELTA4);
    tp.max_bits = scal;
    SmallGradParams sp{};
    sp.z1 = tp.z1; sp.z2 = tp.z2; sp.z3 = tp.z3;
    TailSideParams sd{};
    if (s->has_side()) {
        sd.fin = d_features;
        sd.w1y = t.side[0]; sd.f1w = t.side[1]; sd.f1b = t.side[2]; sd.f2w = t.side[3]; sd.f2b = t.side[4]; sd.f3w = t.side[5]; sd.f3b = t.side[6];
        sd.kfin = s->side_item(TRS_TRAIN_SIDE_FIN); sd.y1 = s->side_item(TRS_TRAIN_SIDE_Y1); sd.y2 = s->side_item(TRS_TRAIN_SIDE_Y2); sd.y3 = s->side_item(TRS_TRAIN_SIDE_Y3);
        sd.dy1 = s->side_item(TRS_TRAIN_SIDE_DY1); sd.dy2 = s->side_item(TRS_TRAIN_SIDE_DY2); sd.dy3 = s->side_item(TRS_TRAIN_SIDE_DY3); sd.pf1 = s->side_item(TRS_TRAIN_SIDE_DY3 + 1);
    }
    if (dr.tail()) {
        TailDropParams dp{};
        dp.Dt = Dt;
        for (int l = 1; l <= 3; ++l) { dp.T[l - 1] = dr.site(l) ? dr.T : 0u; dp.s[l - 1] = dr.site(l) ? dr.s : 1.0f; }
        dp.a1 = s->dropped(1); dp.a2 = s->dropped(2); dp.a3 = s->dropped(3);
        if (s->has_side()) hipLaunchKernelGGL(trs_train_tail_side_drop_kernel, dim3((n + 3) / 4), dim3(256), 0, st, tp, dp, sd);
        else
        hipLaunchKernelGGL(trs_train_tail_drop_kernel, dim3((n + 3) / 4), dim3(256), 0, st, tp, dp);
        // the small kernel takes relu of what it reads, and relu(a') is a' bit for bit (a' is +0 or a non-negative product): it reads a'(l) where it read z(l)
        sp.z1 = dp.a1; sp.z2 = dp.a2; sp.z3 = dp.a3;
    } else if (s->has_side()) {
        hipLaunchKernelGGL(trs_train_tail_side_kernel, dim3((n + 3) / 4), dim3(256), 0, st, tp, sd);
    } else {
        hipLaunchKernelGGL(trs_train_tail_kernel, dim3((n + 3) / 4), dim3(256), 0, st, tp);
    }
    sp.d1 = tp.d1; sp.d2 = tp.d2; sp.d3 = tp.d3; sp.d4 = tp.d4; sp.out = tp.out; sp.y = d_labels;
    sp.g = s->g.get(); std::memcpy(sp.off, s->L.off, sizeof sp.off);
    sp.loss = reinterpret_cast<float*>(scal + 2); sp.loss_user = d_loss_or_null; sp.n = n;
    hipLaunchKernelGGL(trs_train_small_kernel, dim3((kSmallGradThreads + 63) / 64), dim3(64), 0, st, sp);
    if (s->has_side()) {
        SmallSideParams ssp{};
        ssp.pf1 = sd.pf1; ssp.y1 = sd.y1; ssp.y2 = sd.y2; ssp.y3 = sd.y3; ssp.d1 = tp.d1; ssp.dy1 = sd.dy1; ssp.dy2 = sd.dy2; ssp.dy3 = sd.dy3;
        ssp.g = s->g.get(); ssp.n = n;
        for (int j = 0; j < 7; ++j) ssp.at[j] = s->side_array(j);
        hipLaunchKernelGGL(trs_train_small_side_kernel, dim3((kSideValues + 63) / 64), dim3(64), 0, st, ssp);
    }
    const int n_pad = (int)trsim::align_up((size_t)n, kGwFrames);
    hipLaunchKernelGGL(trs_train_quant_kernel, dim3(n_pad), dim3(128), 0, st, tp.d1, scal, s->q.get(), reinterpret_cast<int*>(scal + 1), n);
    Gw1Params gp{};
    gp.x7 = static_cast<const u4v*>(t.x7); gp.q = reinterpret_cast<const u4v*>(s->q.get()); gp.gw1 = s->g.get(); gp.sexp = reinterpret_cast<const int*>(scal + 1);
    gp.n = n; gp.n_pad = n_pad; gp.G = t.G;
    hipLaunchKernelGGL(trs_train_gw1_kernel, dim3(t.G / 16), dim3(256), 0, st, gp);
    const trs_train_config& c = s->cfg;
    const AdamK k{c.beta1, trsim::train_one_minus(c.beta1), c.beta2, trsim::train_one_minus(c.beta2), c.eps, trsim::train_alpha(c, s->t + 1)};
    if (s->conv)                                                            // conv4 .. conv7 from delta1 and the dense1 copy the forward used: before Adam rewrites it
        if (int rc = trs_train_conv_step(*s->conv, e, v, t, s->q.get(), reinterpret_cast<const int*>(scal + 1), n, k, dr.site(0) ? dr.s : 0.0f)) return rc;
    if (c.train_mask & 1u)
        hipLaunchKernelGGL(trs_train_adam1_kernel, dim3((t.G * 128 + 255) / 256), dim3(256), 0, st, s->g.get(), s->m.get(), s->v.get(), s->master.get(), t.w1_pack, t.G, k);
    AdamSmallParams ap{};
    std::memcpy(ap.off, s->L.off, sizeof ap.off);
    tail_live(t, ap.live);
    ap.mask = c.train_mask;
    const size_t small = s->L.off[kTrainArrays] - s->L.off[1];
    hipLaunchKernelGGL(trs_train_adam_kernel, dim3((unsigned)((small + 255) / 256)), dim3(256), 0, st, s->g.get(), s->m.get(), s->v.get(), s->master.get(), ap, k);
    if (s->has_side()) {
        AdamSideParams asp{};
        for (int j = 0; j < 7; ++j) {
            asp.at[j] = s->side_array(j); asp.first[j + 1] = asp.first[j] + (int)kSideArrayCount[j]; asp.live[j] = t.side[j];
            asp.bit[j] = j == 0 ? 0 : train_mask_bit(kTrainArrays + j - 1);
        }
        asp.mask = c.train_mask;
        hipLaunchKernelGGL(trs_train_adam_side_kernel, dim3((kSideValues + 255) / 256), dim3(256), 0, st, s->g.get(), s->m.get(), s->v.get(), s->master.get(), asp, k);
    }
    HIPCHK(hipGetLastError());
    s->t += 1; s->last_n = n;
    return TRS_OK;
}

// trs_pilot_train_get (n_arrays 0: eight arrays, 22-array sessions alone) and trs_pilot_train_get_ex
int get_masters(trs_env* e, float* const* h_out, int n_arrays, int* t_out_or_null)
{
    TrsEnvView v; TrsPilotTail t; TrainSession* s;
    if (int rc = enter_session(e, &v, &t, &s)) return rc;
    if (!h_out) return trs_internal_fail(TRS_ERR_ARG, "h_tail_arrays_out is NULL");
    if (!n_arrays && s->has_side()) return trs_internal_fail(TRS_ERR_ARG, "a 28-array session holds 14 arrays: use trs_pilot_train_get_ex");
    if (n_arrays && n_arrays != s->n_arrays) return trs_internal_fail(TRS_ERR_ARG, "n_arrays does not match the session: 8 for a 22-array pilot, 14 for a 28-array one");
    HIPCHK(hipSetDevice(v.device));
    HIPCHK(hipStreamSynchronize(v.stream));
    for (int a = 0; a < s->n_arrays; ++a) {
        if (!h_out[a]) continue;
        const size_t at = a < kTrainArrays ? s->L.off[a] : s->SL.off[a], count = a < kTrainArrays ? s->L.count(a) : s->SL.count(a);
        HIPCHK(hipMemcpy(h_out[a], s->master.get() + at, count * sizeof(float), hipMemcpyDeviceToHost));
        trs_internal_count(e, (uint64_t)(count * sizeof(float)), 0);
    }
    if (t_out_or_null) *t_out_or_null = (int)s->t;
    return TRS_OK;
}

}  // namespace

TRS_EXPORT int trs_pilot_train_begin(trs_env* e, const trs_train_config* cfg_or_null, const float* const* h_tail_arrays)
{
    return begin_session(e, cfg_or_null, h_tail_arrays, kTrainArrays, false);
}

TRS_EXPORT int trs_pilot_train_begin_ex(trs_env* e, const trs_train_config* cfg_or_null, const float* const* h_arrays, int n_arrays)
{
    return begin_session(e, cfg_or_null, h_arrays, n_arrays, true);
}

TRS_EXPORT int trs_pilot_train_step(trs_env* e, const uint8_t* d_frames, const float* d_labels, int n, float* d_loss_or_null)
{
    return train_step(e, d_frames, nullptr, d_labels, n, d_loss_or_null, false);
}

TRS_EXPORT int trs_pilot_train_step_ex(trs_env* e, const uint8_t* d_frames, const float* d_features, const float* d_labels, int n, float* d_loss_or_null)
{
    return train_step(e, d_frames, d_features, d_labels, n, d_loss_or_null, true);
}

// ---- dropout behind conv7 (trsim_dropout.hpp) -------------------------------------------------------------------------------------------
TRS_EXPORT void trs_default_dropout_config(trs_dropout_config* cfg)
{
    if (cfg) trsim::dropout_defaults(cfg);
}

TRS_EXPORT int trs_train_dropout_keep(const trs_dropout_config* cfg_or_null, int64_t t, int site, int n, int64_t width, uint8_t* h_keep)
{
    trs_dropout_config cfg;
    trsim::dropout_defaults(&cfg);
    if (cfg_or_null) {
        if (const char* why = trsim::dropout_config_error(cfg_or_null)) return trs_internal_fail(TRS_ERR_ARG, why);
        cfg = *cfg_or_null;
    }
    if (const char* why = trsim::dropout_keep_error(t, site, n, width, h_keep)) return trs_internal_fail(TRS_ERR_ARG, why);
    trsim::dropout_keep_host(cfg, t, site, n, width, h_keep);
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_train_dropout(trs_env* e, const trs_dropout_config* cfg_or_null)
{
    trs_dropout_config cfg;
    trsim::dropout_defaults(&cfg);
    if (cfg_or_null) {
        if (const char* why = trsim::dropout_config_error(cfg_or_null)) return trs_internal_fail(TRS_ERR_ARG, why);
        cfg = *cfg_or_null;
    }
    TrsEnvView v; TrsPilotTail t; TrainSession* s;
    if (int rc = enter_session(e, &v, &t, &s)) return rc;
    if (s->drop.called) return trs_internal_fail(TRS_ERR_STATE, "trs_pilot_train_dropout was already called in this session");
    if (s->t > 0) return trs_internal_fail(TRS_ERR_STATE, "trs_pilot_train_dropout comes before the session's first step");
    DropSession& d = s->drop;
    d.T = trsim::dropout_threshold(cfg.rate);
    d.s = trsim::dropout_scale(d.T);
    d.seed = cfg.seed;
    d.on = d.T ? cfg.sites : 0u;                                            // rate 0: every site keeps its kernels and its bits
    if (d.tail()) {
        HIPCHK(hipSetDevice(v.device));
        HIPCHK(d.act.alloc((size_t)s->n_cap * (100 + 50 + 25) * sizeof(float)));
    }
    d.called = true;
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_train_get(trs_env* e, float* const* h_tail_arrays_out, int* t_out_or_null)
{
    return get_masters(e, h_tail_arrays_out, 0, t_out_or_null);
}

TRS_EXPORT int trs_pilot_train_get_ex(trs_env* e, float* const* h_arrays_out, int n_arrays, int* t_out_or_null)
{
    if (n_arrays != kTrainArrays && n_arrays != kTrainSideArrays) return trs_internal_fail(TRS_ERR_ARG, "n_arrays must be 8 (a 22-array pilot) or 14 (a 28-array pilot)");
    return get_masters(e, h_arrays_out, n_arrays, t_out_or_null);
}

TRS_EXPORT int trs_pilot_train_debug_side(trs_env* e, int which, float* h_dst, size_t n_floats)
{
    TrsEnvView v; TrsPilotTail t; TrainSession* s;
    if (int rc = enter_session(e, &v, &t, &s)) return rc;
    if (!s->has_side()) return trs_internal_fail(TRS_ERR_STATE, "the session has no side branch: a 28-array pilot's alone has (trs_pilot_train_begin_ex)");
    if (!s->last_n) return trs_internal_fail(TRS_ERR_STATE, "no training step yet");
    const size_t want = trsim::train_side_debug_floats(which, s->last_n);
    if (!want || !h_dst) return trs_internal_fail(TRS_ERR_ARG, "unknown item (TRS_TRAIN_SIDE_*) or NULL destination");
    if (n_floats != want) return trs_internal_fail(TRS_ERR_ARG, "size mismatch");
    HIPCHK(hipSetDevice(v.device));
    HIPCHK(hipStreamSynchronize(v.stream));
    const float* src;
    if (which <= TRS_TRAIN_SIDE_DY3) src = s->side_item(which);
    else if (which < TRS_TRAIN_SIDE_M) src = s->g.get() + s->side_array(which - TRS_TRAIN_SIDE_G);
    else if (which < TRS_TRAIN_SIDE_V) src = s->m.get() + s->side_array(which - TRS_TRAIN_SIDE_M);
    else src = s->v.get() + s->side_array(which - TRS_TRAIN_SIDE_V);
    HIPCHK(hipMemcpy(h_dst, src, want * sizeof(float), hipMemcpyDeviceToHost));
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_train_debug(trs_env* e, int which, float* h_dst, size_t n_floats)
{
    TrsEnvView v; TrsPilotTail t; TrainSession* s;
    if (int rc = enter_session(e, &v, &t, &s)) return rc;
    if (!s->last_n) return trs_internal_fail(TRS_ERR_STATE, "no training step yet");
    const size_t want = trsim::train_debug_floats(which, s->last_n, s->F);
    if (!want || !h_dst) return trs_internal_fail(TRS_ERR_ARG, "unknown item (TRS_TRAIN_DBG_*) or NULL destination");
    if (n_floats != want) return trs_internal_fail(TRS_ERR_ARG, "size mismatch");
    HIPCHK(hipSetDevice(v.device));
    HIPCHK(hipStreamSynchronize(v.stream));
    const float* src = nullptr;
    if (which <= TRS_TRAIN_DBG_DELTA4) src = s->item(which);
    else if (which <= TRS_TRAIN_DBG_GW4) src = s->g.get() + s->L.off[2 * (which - TRS_TRAIN_DBG_GW1)];
    else if (which <= TRS_TRAIN_DBG_GB4) src = s->g.get() + s->L.off[2 * (which - TRS_TRAIN_DBG_GB1) + 1];
    else if (which < TRS_TRAIN_DBG_V) src = s->m.get() + s->L.off[which - TRS_TRAIN_DBG_M];
    else if (which < TRS_TRAIN_DBG_SCALE_EXP) src = s->v.get() + s->L.off[which - TRS_TRAIN_DBG_V];
    else if (which == TRS_TRAIN_DBG_LOSS) src = reinterpret_cast<const float*>(s->scal.get() + 2);
    if (src) {
        HIPCHK(hipMemcpy(h_dst, src, want * sizeof(float), hipMemcpyDeviceToHost));
        return TRS_OK;
    }
    if (which >= TRS_TRAIN_DBG_A1 && which <= TRS_TRAIN_DBG_A3) {       // what the next layer read: a'(l) of a step with dropout, else relu(z(l))
        const int l = which - TRS_TRAIN_DBG_A1 + 1;
        if (s->drop.tail()) {
            HIPCHK(hipMemcpy(h_dst, s->dropped(l), want * sizeof(float), hipMemcpyDeviceToHost));
            return TRS_OK;
        }
        HIPCHK(hipMemcpy(h_dst, s->item(TRS_TRAIN_DBG_Z1 + l - 1), want * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < want; ++i) h_dst[i] = h_dst[i] > 0.0f ? h_dst[i] : 0.0f;
        return TRS_OK;
    }
    if (which == TRS_TRAIN_DBG_SCALE_EXP) {
        int sexp = 0;
        HIPCHK(hipMemcpy(&sexp, s->scal.get() + 1, sizeof sexp, hipMemcpyDeviceToHost));
        h_dst[0] = (float)sexp;
        return TRS_OK;
    }
    // TRS_TRAIN_DBG_PACK1: granules [G][128][8] -> [F][100]
    std::vector<unsigned short> pack((size_t)t.G * 128 * 8);
    HIPCHK(hipMemcpy(pack.data(), t.w1_pack, pack.size() * 2, hipMemcpyDeviceToHost));
    for (size_t g = 0; g < (size_t)t.G; ++g)
        for (int j = 0; j < 8; ++j)
            for (int co = 0; co < 100; ++co) h_dst[(g * 8 + j) * 100 + co] = widen_h(pack[(g * 128 + co) * 8 + j]);
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_train_end(trs_env* e)
{
    TrsEnvView v; TrsPilotTail t; TrainSession* s;
    if (int rc = enter_session(e, &v, &t, &s)) return rc;
    HIPCHK(hipSetDevice(v.device));
    HIPCHK(hipStreamSynchronize(v.stream));
    delete s;
    *t.train = nullptr;
    return TRS_OK;
}
