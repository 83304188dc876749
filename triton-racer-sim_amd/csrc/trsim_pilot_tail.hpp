// trsim_pilot_tail.hpp — everything of the pilot behind conv7 (included by trsim_pilot.hip inside its anonymous namespace, like trsim_pilot_layers.hpp):
//   trs_pilot_dense_kernel      dense1 (and dense4) on the matrix cores: split-K slabs of fp32 partial sums
//   trs_pilot_tail_kernel       cnn_2d_speed_control / cnn_2d: the slabs added, dense2 -> dense3 -> output in fp32, KerasPilot.step
//   trs_pilot_tail_ex_kernel    cnn_2d_speed_as_feature / cnn_2d_full_house: the small input branches and the second head as well
//   pilot_step                  KerasPilot.step itself, the ONE copy both tails end with, on the one block (StepIo) both parameter structs embed
//   trs_pilot_count_sat_kernel, trs_zero_controls_kernel
// The two tails add their slabs and run their small dense layers differently on purpose (one wave per frame in both; the first holds a lane's 175 weights
// in registers, the second serves two architectures' widths from one blob): the comments in each say what was measured.  The slots of that blob (XO_*)
// and the branch widths are trsim_pilot_plan.hpp's, which also packs it.
#pragma once

// Where KerasPilot.step's inputs and outputs live and the pilot's configuration: what the two tails share (filled by step_io in trsim_pilot.hip)
struct StepIo {
    float* raw_out;            // [n][2] or nullptr
    const float* speed;        // 'gym/speed' (read by the rule only where act is set; trs_pilot_tail_ex_kernel also feeds it to the model)
    const uint8_t* mode;       // 'usr/mode' per car (TRS_MODE_*) or nullptr: a car outside AI / AI_STEERING gets (0, 0, 0) (keras_pilot.py:139)
    float *steer, *thr, *brk;  // next controls
    int n, act;                // act = 0: raw outputs only
    float threshold, rev_mult, brk_mult, smooth_thr;
    int use_break, smooth, capped;   // capped: ModelType.CNN_2D and CNN_2D_SPD_FTR (the outputs are steering and throttle)
};

// raw outputs -> KerasPilot.step's controls for car i (keras_pilot.py:56-118: the speed controller of CNN_2D_SPD_CTL / CNN_2D_FULL_HOUSE :78-95, :97-118; __cap of
// both outputs for CNN_2D / CNN_2D_SPD_FTR :56-76; the mode mask :139; smooth steering :147-153; calcThrottle / calcBreak of utils/mapping.py:23-35)
__device__ __forceinline__ void pilot_step(const StepIo& p, int i, float out0, float out1)
{
    if (p.raw_out) { p.raw_out[2 * i] = out0; p.raw_out[2 * i + 1] = out1; }
    if (!p.act) return;
    if (p.mode && p.mode[i] != TRS_MODE_AI && p.mode[i] != TRS_MODE_AI_STEERING) { p.steer[i] = 0.0f; p.thr[i] = 0.0f; p.brk[i] = 0.0f; return; }
    float steering = out0 < -1.0f ? -1.0f : (out0 > 1.0f ? 1.0f : out0);           // __cap (keras_pilot.py:142-145)
    float throttle, breaking = 0.0f;
    if (p.capped) throttle = out1 < -1.0f ? -1.0f : (out1 > 1.0f ? 1.0f : out1);    // __cap of both outputs, breaking 0 (:60, :74)
    else {
        const float predicted = out1 * 20.0f;                                       // :83
        const float real = p.speed[i];
        const float kHalfPi = 1.57079632679489661923f;
        const float delta = predicted * p.threshold - real;                         // calcThrottle (mapping.py:23-28)
        throttle = p.rev_mult * atanf(delta * 2.0f) / kHalfPi;
        if (throttle > -0.2f && throttle < 0.0f) throttle = 0.0f;
        if (p.use_break) {                                                          // keras_pilot.py:88-90, mapping.py:30-35
            throttle = (predicted - real > 0.0f) ? 1.0f : 0.0f;
            breaking = -1.0f * p.brk_mult * atanf(delta * 1.0f) / kHalfPi;
            if (breaking < 0.4f) breaking = 0.0f;
        }
    }
    if (p.smooth) {                                                                 // keras_pilot.py:147-153
        if (steering > p.smooth_thr) steering = 1.0f;
        else if (steering < -p.smooth_thr) steering = -1.0f;
    }
    p.steer[i] = steering; p.thr[i] = throttle; p.brk[i] = breaking;
}

// dense2 -> dense3 -> output in fp32 (keras_train.py:161-168), then KerasPilot.step
struct TailParams {
    const float* h1;           // dense1 output before ReLU, fp32: h1_slices slabs of [n][100] (split-K partial sums, added here in slice order)
    int h1_slices; size_t h1_stride;
    const float *w2, *b2, *w3, *b3, *w4, *b4;    // Keras layouts [IN][OUT]
    StepIo io;
};

__global__ __launch_bounds__(256) void trs_pilot_tail_kernel(const TailParams p)
{
    // one wave per frame: lane o owns output neuron o of the current layer; activations travel through LDS
    __shared__ float s1[4][100], s2[4][50], s3[4][25], s4[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    if (i >= p.io.n) return;
    // The three small layers are latency chains (100 + 50 + 25 dependent FMAs per lane); what made them slow was a global weight
    // load in front of every FMA.  All of a lane's weights — column `lane` of each matrix — are requested up front (175 independent
    // loads, coalesced across lanes) and land while the slab sums run; the FMAs then read registers and LDS only.
    float wc2[100], wc3[50], wc4[25];
    {
        const int o2 = min(lane, 49), o3 = min(lane, 24), o4 = min(lane, 1);
#pragma unroll
        for (int k = 0; k < 100; ++k) wc2[k] = p.w2[k * 50 + o2];
#pragma unroll
        for (int k = 0; k < 50; ++k) wc3[k] = p.w3[k * 25 + o3];
#pragma unroll
        for (int k = 0; k < 25; ++k) wc4[k] = p.w4[k * 2 + o4];
    }
    const float bias2 = p.b2[min(lane, 49)], bias3 = p.b3[min(lane, 24)], bias4 = p.b4[min(lane, 1)];
    {   // dense1's 100 outputs of this frame = the K-slice slabs added in slice order (fixed order: run-to-run identical).  A lane
        // owns outputs `lane` and `lane + 64`; the phase is pure load latency, so 16 slices x 2 outputs are requested together.
        const bool two = lane + 64 < 100;
        const float* src0 = p.h1 + (size_t)i * 100 + lane;
        const float* src1 = src0 + (two ? 64 : 0);
        float x0 = 0.0f, x1 = 0.0f;
        // groups of 16 slices, the last one padded: a slice past the end is read at the last slice's address and added as 0.0f (x + 0.0f == x for
        // every x that can reach the ReLU's test).  31 slices (240x320) are two load round trips; the ragged tail used to go 4 + 4 + 4 + 1 + 1 + 1
        // slices at a time: seven dependent round trips, the whole difference between this kernel's 6.0 us at 120x160 and 8.8 us at 240x320.
        auto add_groups = [&](auto gc) {
            constexpr int G = decltype(gc)::value;
            for (int sl = 0; sl < p.h1_slices; sl += G) {
                float v0[G], v1[G];
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const int sq = min(sl + q, p.h1_slices - 1);
                    v0[q] = src0[(size_t)sq * p.h1_stride]; v1[q] = src1[(size_t)sq * p.h1_stride];
                }
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const bool in = sl + q < p.h1_slices;
                    x0 += in ? v0[q] : 0.0f; x1 += in ? v1[q] : 0.0f;
                }
            }
        };
        if (p.h1_slices <= 8) add_groups(std::integral_constant<int, 8>{});      // (120x160: 8 slices - no padded loads)
        else add_groups(std::integral_constant<int, 16>{});
        s1[wv][lane] = x0 > 0.f ? x0 : 0.f;                                 // dense1's ReLU
        if (two) s1[wv][lane + 64] = x1 > 0.f ? x1 : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 50) {
        float s = bias2;
#pragma unroll
        for (int k = 0; k < 100; ++k) s = fmaf(s1[wv][k], wc2[k], s);
        s2[wv][lane] = s > 0.f ? s : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 25) {
        float s = bias3;
#pragma unroll
        for (int k = 0; k < 50; ++k) s = fmaf(s2[wv][k], wc3[k], s);
        s3[wv][lane] = s > 0.f ? s : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 2) {
        float s = bias4;
#pragma unroll
        for (int k = 0; k < 25; ++k) s = fmaf(s3[wv][k], wc4[k], s);
        s4[wv][lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane != 0) return;
    pilot_step(p.io, i, s4[wv][0], s4[wv][1]);
}

// ---- dense1 as its own kernel (round 2) -------------------------------------------------------------------------------------
// dense1 (4,608 -> 100 at 120x160, 70,528 -> 100 at 240x320) is 0.8 % of the network's arithmetic but, as a 1x1 convolution on
// the chunked kernel, it and the tail were 23 of 267 us: 36 K slices of partial sums written and read back (19 MB against 9.4 MB
// of activations).  Here a workgroup takes 32 frames x one K slice (8 slices fill the chip at 1024 frames):
//   * the slice's activations go through LDS (coalesced 16-byte loads of each frame's contiguous run, chunks of 72 granules,
//     double buffered; row pitch 73 granules = conflict-free ds_read_b128 fragments);
//   * wave w owns channels 32 w .. 32 w + 31: all 36 k-steps of a chunk on one accumulator, its weight fragments ALL in flight (a
//     register ring of 36 granules straight from L2, each refilled for the next chunk right behind the MFMA that read it);
//   * workgroups are numbered so that one XCD works on one K slice: its 1/8 of the weights stays in that XCD's L2;
//   * the slice's partial sums go to slab [slice][frame][100]; the tail kernel adds the slabs in slice order.
// 15.5 -> 7.3 us (and the tail 7.5 -> 5.8 with 8 slabs instead of 36); 47 -> 36 us at 512 x 240x320.  Measured and NOT kept
// (profiles/r02_pilot_dense.txt): the tail in the same launch, run by the last K slice of a frame group to arrive — the hand-over
// between XCDs costs a write-through drain (2.2 us) and an sc1 read (4 us) and leaves 32 workgroups to do what 256 do in the
// tail kernel: 17 us in one launch against 7.3 + 5.8 in two.  (DenseParams: trsim_pilot_pass.hpp)
#ifndef TRS_DENSE_ABLATE
#define TRS_DENSE_ABLATE 0   /* timing-only diagnostic builds (scripts/r04_dense_ablate.sh), never shipped */
#endif
constexpr int kDenseSteps = kDenseChunk / 2;
constexpr int kDenseStage = 9;             // granules a thread stages per chunk and per 32 frames (32 x 72 / 256)

// NF = frame blocks of 32 per workgroup.  NF = 2 (round 4, long K: 240x320): every weight fragment feeds TWO MFMAs (frames 0..31 and 32..63), so the
// weight stream — per-lane 16-byte loads straight from L2, 1.18 MB per workgroup at 512 x 240x320, measured as 15 of the kernel's 37 us by a
// timing-only build (profiles/r04_pilot_dense.txt) — is halved for the same arithmetic; 150 KB of LDS, one workgroup per CU.
template <int NF>
__global__ __launch_bounds__(256) void trs_pilot_dense_kernel(const DenseParams p)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int group = idx % p.groups, slice = xcd + 8 * (idx / p.groups);
    if (slice >= p.KS) return;                                              // the grid is padded to whole rounds of 8 slices
    u4v* const st = reinterpret_cast<u4v*>(psmem);                          // [2][32 NF][73] granules
    const int gs = slice * p.gps, ge = min(p.G, gs + p.gps);
    const int f0 = group * 32 * NF;
    constexpr int kStage = kDenseStage * NF, kBuf = 32 * NF * kDensePitch;

    // staging: thread t moves granules e = t + 256 i (i < 9 NF) of a chunk: frame e / 72, granule e % 72
    int sbase[kStage], sdst[kStage];
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
        const int e = tid + 256 * i, f = e / kDenseChunk, gi = e - f * kDenseChunk;
        sbase[i] = min(f0 + f, p.n - 1) * p.G;
        sdst[i] = f * kDensePitch + gi;
    }
    u4v pf[kStage];
    auto stage_load = [&](int c0) {
#pragma unroll
        for (int i = 0; i < kStage; ++i) {
            const int e = tid + 256 * i, f = e / kDenseChunk, gi = e - f * kDenseChunk;
#if TRS_DENSE_ABLATE == 2   /* timing-only: every chunk re-reads the slice's first chunk (cache hits instead of the HBM stream) */
            pf[i] = p.act[sbase[i] + min(gs + gi, p.G - 1)]; (void)c0;
#else
            pf[i] = p.act[sbase[i] + min(c0 + gi, p.G - 1)];
#endif
        }
    };
    auto stage_write = [&](int buf) {
        u4v* const sn = st + buf * kBuf;
#pragma unroll
        for (int i = 0; i < kStage; ++i) sn[sdst[i]] = pf[i];
    };
    // weight ring: granule 2 j + h of the chunk for k-step j, this wave's 32 channels
    u4v wr[kDenseSteps];
    const u4v* const wlane = p.w + wave * 32 + r;
    auto ring_load = [&](int j, int c0) { wr[j] = wlane[(size_t)min(c0 + 2 * j + h, p.G - 1) * 128]; };
    stage_load(gs);
#pragma unroll
    for (int j = 0; j < kDenseSteps; ++j) ring_load(j, gs);

    f32x16 acc[NF];
#pragma unroll
    for (int b = 0; b < NF; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = slice == 0 ? p.bias[wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h] : 0.0f;
    stage_write(0);
    __syncthreads();

    auto chunk = [&](int c0, int buf, auto prefetch) {
        const u4v* const sb = st + buf * kBuf + r * kDensePitch + h;
#pragma unroll
        for (int j = 0; j < kDenseSteps; ++j) {
            const bool past = c0 + 2 * j >= ge;                             // ragged last chunk: a zero fragment instead of a branch
#pragma unroll
            for (int b = 0; b < NF; ++b) {
                u4v a = sb[b * 32 * kDensePitch + 2 * j];
                if (past) a = u4v{0u, 0u, 0u, 0u};
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, wr[j]), __builtin_bit_cast(h16x8, a), acc[b], 0, 0, 0);
            }
#if TRS_DENSE_ABLATE != 1   /* 1: timing-only, the weights of the first chunk serve every chunk (no weight stream) */
            if constexpr (decltype(prefetch)::value) ring_load(j, c0 + kDenseChunk);
#endif
        }
    };
    int c0 = gs, buf = 0;
    for (; c0 + kDenseChunk < ge; c0 += kDenseChunk, buf ^= 1) {            // every chunk but the last: the next one's operands are requested underneath
        stage_load(c0 + kDenseChunk);
        chunk(c0, buf, std::true_type{});
        stage_write(buf ^ 1);
        __syncthreads();
    }
    chunk(c0, buf, std::false_type{});

    {   // D[cout][frame]: lane = frame r, registers 4 q4 .. + 3 = channels 32 wave + 8 q4 + 4 h .. + 3: one 16-byte store each
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(p.slab, 0, (int)((size_t)p.KS * p.n * 400), 0x00020000);
#pragma unroll
        for (int b = 0; b < NF; ++b) {
            const int fr = f0 + 32 * b + r;
            const int row = ((slice * p.n + fr) * 100) * 4;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int c = wave * 32 + 8 * q4 + 4 * h;
                if (c < 100 && fr < p.n) {
                    const u4v v = {__float_as_uint(acc[b][4 * q4]), __float_as_uint(acc[b][4 * q4 + 1]), __float_as_uint(acc[b][4 * q4 + 2]), __float_as_uint(acc[b][4 * q4 + 3])};
                    __builtin_amdgcn_raw_buffer_store_b128(v, rs, row + c * 4, 0, 0);
                }
            }
        }
    }
}

// The tail of the model types with extra inputs (components/keras_train.py): cnn_2d_speed_as_feature =
// Keras_2D_CNN.get_model(num_feature_vectors = 1) (:127-174: speed / 20 -> Dense 4 -> 8 -> 16, concatenated behind the flatten in
// front of dense1) and cnn_2d_full_house = Keras_2D_FULL_HOUSE.get_model (:184-245: 'loc/segment' -> 16 -> 32 -> 64 joins the
// flatten for the speed head dense1..3 -> output_speed; speed / 20 -> 16 -> 32 -> 64 joins both for the steering head
// dense4..6 -> out_steering; output = [steering, speed]).  The rows of dense1 / dense4 that multiply the flatten ran on the
// matrix cores (split-K slabs, added here in slice order); the rows of the small branches and everything behind are fp32, one
// wave per frame, a fixed summation order (k ascending) so that two runs agree bit for bit.
struct TailExParams {
    const float* h1; int h1_slices; size_t h1_stride;       // dense1: slabs of [n][100]
    const float* h4; int h4_slices; size_t h4_stride;       // dense4 (full house) or nullptr
    const float* blob; int xo[32];                           // the small fp32 weights and their offsets by XO_* (pack_tail_blob, trsim_pilot_plan.hpp)
    int arch, f1, f2, f3;                                    // widths of the small branches (4, 8, 16 or 16, 32, 64)
    const float* segment; const int32_t* seg_idx; int np;    // 'loc/segment' given, or from the env's index
    StepIo io;                                               // io.speed ('gym/speed') is a model input here: never null
};

__device__ __forceinline__ void dense_small(const float* in, int nin, const float* w, const float* b, int nout, float* out, int lane, bool relu)
{   // out[o] = act(b[o] + sum_k in[k] * w[k][o]), lanes over o (nout <= 128).  One FMA chain per output, k ascending; the weights of 16 k
    // are requested together (a load in front of every FMA made this the slowest kernel of the full-house loop: one L2 round trip per k)
    for (int o = lane; o < nout; o += 64) {
        float s = b[o];
        int k = 0;
        for (; k + 16 <= nin; k += 16) {
            float wv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) wv[j] = w[(k + j) * nout + o];
#pragma unroll
            for (int j = 0; j < 16; ++j) s = fmaf(in[k + j], wv[j], s);
        }
        for (; k + 4 <= nin; k += 4) {
            float wv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wv[j] = w[(k + j) * nout + o];
#pragma unroll
            for (int j = 0; j < 4; ++j) s = fmaf(in[k + j], wv[j], s);
        }
        for (; k < nin; ++k) s = fmaf(in[k], w[k * nout + o], s);
        out[o] = relu ? (s > 0.f ? s : 0.f) : s;
    }
}

__global__ __launch_bounds__(256) void trs_pilot_tail_ex_kernel(const TailExParams p)
{
    __shared__ float sy[4][3][64], ss[4][3][64], sh[4][2][100], sa[4][2][50], sb[4][2][25], so[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    if (i >= p.io.n) return;
    const float* B = p.blob;
    const float real = p.io.speed[i];
    // the small branches
    float fin = real / 20.0f;                                                      // keras_pilot.py:68,100: speed / 20
    if (p.arch == TRS_PILOT_FULL_HOUSE)                                            // 'loc/segment' (track_data_process.py:106-107: idx / len * 10, binary64)
        fin = p.segment ? p.segment[i] : (float)((double)p.seg_idx[i] / (double)p.np * 10.0);
    if (lane == 0) sy[wv][2][63] = fin;
    __builtin_amdgcn_wave_barrier();
    dense_small(&sy[wv][2][63], 1, B + p.xo[XO_F1W], B + p.xo[XO_F1B], p.f1, sy[wv][0], lane, true);
    __builtin_amdgcn_wave_barrier();
    dense_small(sy[wv][0], p.f1, B + p.xo[XO_F2W], B + p.xo[XO_F2B], p.f2, sy[wv][1], lane, true);
    __builtin_amdgcn_wave_barrier();
    dense_small(sy[wv][1], p.f2, B + p.xo[XO_F3W], B + p.xo[XO_F3B], p.f3, sy[wv][2], lane, true);
    if (p.arch == TRS_PILOT_FULL_HOUSE) {
        if (lane == 0) ss[wv][2][63] = real / 20.0f;
        __builtin_amdgcn_wave_barrier();
        dense_small(&ss[wv][2][63], 1, B + p.xo[XO_C1W], B + p.xo[XO_C1B], p.f1, ss[wv][0], lane, true);
        __builtin_amdgcn_wave_barrier();
        dense_small(ss[wv][0], p.f1, B + p.xo[XO_C2W], B + p.xo[XO_C2B], p.f2, ss[wv][1], lane, true);
        __builtin_amdgcn_wave_barrier();
        dense_small(ss[wv][1], p.f2, B + p.xo[XO_C3W], B + p.xo[XO_C3B], p.f3, ss[wv][2], lane, true);
    }
    __builtin_amdgcn_wave_barrier();
    // dense1 (and dense4): slabs in slice order, then the rows of the small branches, then ReLU
    for (int head = 0; head < (p.arch == TRS_PILOT_FULL_HOUSE ? 2 : 1); ++head) {
        const float* slab = head ? p.h4 : p.h1;
        const int slices = head ? p.h4_slices : p.h1_slices;
        const size_t stride = head ? p.h4_stride : p.h1_stride;
        const float* wy = B + p.xo[head ? XO_W4Y : XO_W1Y];
        for (int o = lane; o < 100; o += 64) {
            float x = 0.0f;
            {   // the K-slice slabs in slice order, eight loads in flight
                int sl = 0;
                for (; sl + 8 <= slices; sl += 8) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = slab[(size_t)(sl + j) * stride + (size_t)i * 100 + o];
#pragma unroll
                    for (int j = 0; j < 8; ++j) x += v[j];
                }
                for (; sl < slices; ++sl) x += slab[(size_t)sl * stride + (size_t)i * 100 + o];
            }
            for (int k = 0; k < p.f3; k += 4) {                             // f3 is 16 or 64
                float w4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) w4[j] = wy[(k + j) * 100 + o];
#pragma unroll
                for (int j = 0; j < 4; ++j) x = fmaf(sy[wv][2][k + j], w4[j], x);
            }
            if (head) for (int k = 0; k < p.f3; k += 4) {
                float w4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) w4[j] = wy[(p.f3 + k + j) * 100 + o];
#pragma unroll
                for (int j = 0; j < 4; ++j) x = fmaf(ss[wv][2][k + j], w4[j], x);
            }
            sh[wv][head][o] = x > 0.f ? x : 0.f;
        }
    }
    __builtin_amdgcn_wave_barrier();
    const int nz = p.arch == TRS_PILOT_FULL_HOUSE ? 1 : 2;                         // outputs of the first head
    dense_small(sh[wv][0], 100, B + p.xo[XO_W2], B + p.xo[XO_B2], 50, sa[wv][0], lane, true);
    if (p.arch == TRS_PILOT_FULL_HOUSE) dense_small(sh[wv][1], 100, B + p.xo[XO_W5], B + p.xo[XO_B5], 50, sa[wv][1], lane, true);
    __builtin_amdgcn_wave_barrier();
    dense_small(sa[wv][0], 50, B + p.xo[XO_W3], B + p.xo[XO_B3], 25, sb[wv][0], lane, true);
    if (p.arch == TRS_PILOT_FULL_HOUSE) dense_small(sa[wv][1], 50, B + p.xo[XO_W6], B + p.xo[XO_B6], 25, sb[wv][1], lane, true);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        auto lin = [&](const float* in, const float* w, const float* b, int nout, int o) {
            float s = b[o];
            for (int k = 0; k < 25; ++k) s = fmaf(in[k], w[k * nout + o], s);
            return s;
        };
        if (p.arch == TRS_PILOT_FULL_HOUSE) {                                      // [out_steering, out_speed] (keras_train.py:240)
            so[wv][0] = lin(sb[wv][1], B + p.xo[XO_W7], B + p.xo[XO_B7], 1, 0);
            so[wv][1] = lin(sb[wv][0], B + p.xo[XO_W4], B + p.xo[XO_B4], nz, 0);
        } else {
            so[wv][0] = lin(sb[wv][0], B + p.xo[XO_W4], B + p.xo[XO_B4], nz, 0);
            so[wv][1] = lin(sb[wv][0], B + p.xo[XO_W4], B + p.xo[XO_B4], nz, 1);
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane != 0) return;
    pilot_step(p.io, i, so[wv][0], so[wv][1]);
}

// fp16 range check (trs_pilot_range_check): activations are stored as binary16 and SATURATE at 65504 (v_pk_min_i16 in every epilogue; the
// reference computes in fp32, components/keras_pilot.py:49-59).  A stored value of exactly 0x7BFF is a saturated one (a sum that lands on
// 65504 by itself is not a practical case): counted per layer into `per_layer` and into the handle's TRS_F_STATS slot.
__global__ __launch_bounds__(256) void trs_pilot_count_sat_kernel(const unsigned short* act, size_t n, unsigned long long* per_layer, unsigned long long* total)
{
    unsigned cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) cnt += act[i] == 0x7BFFu ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((threadIdx.x & 63) == 0 && cnt) { atomicAdd(per_layer, (unsigned long long)cnt); atomicAdd(total, (unsigned long long)cnt); }
}

__global__ void trs_zero_controls_kernel(float* a, float* b, float* c, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { a[i] = 0.f; b[i] = 0.f; c[i] = 0.f; }
}
