// trsim_pilot.hip — cnn_2d_speed_control in the loop (BASELINE config 5).
//
// Model: Keras_2D_CNN.get_model(input_shape, num_outputs=2) of the reference
// (TritonRacerSim/components/keras_train.py:127-174, chosen for cnn_2d_speed_control at :393-395): conv 5x5/2 x3
// (24, 32, 64), conv 3x3/1 x4 (64, 64, 128, 128), all 'valid' + ReLU, flatten (NHWC order), dense 100/50/25 + ReLU,
// linear output 2.  Dropout is identity at inference.  57.8 M MAC per 120x160 frame.
//
// Convolutions are implicit GEMMs on the matrix cores, one kernel for every layer:
//   C[pixel][cout] = sum_k A[pixel][k] * B[k][cout],  k = (kh, kw, cin) cut into granules of 8 input channels
//   v_mfma_f32_32x32x16_f16: a wave owns 32 output pixels x all (padded) output channels; per 16-deep k-step the
//   lane (row r = lane & 31, half h = lane >> 5) needs A[r][8h .. 8h+7] = ONE granule = one 16-byte load straight
//   from the NHWC fp16 activation in global memory (no im2col buffer, no LDS for A); B granules [g][cout][8] are
//   staged per workgroup in LDS in exactly the fragment order, so a B fragment is one ds_read_b128.
//   conv1 reads the uint8 frame directly: a k-step is one kernel row = 15 contiguous bytes (5 px x RGB) + 1 pad,
//   fetched with 3 aligned dwords + v_alignbyte, converted exactly to binary16; the 1/255 of the pilot's normalisation
//   (components/keras_pilot.py:49-50) is folded into conv1's weights as 256/255, with 2^-8 in its epilogue (kConv1Scale).
//   dense1 (4608 -> 100) is the same kernel as a 1x1 convolution over "pixels" = frames.
// The fp32 tail (dense2, dense3, output) and KerasPilot's post-processing (keras_pilot.py:78-95; calcThrottle /
// calcBreak of utils/mapping.py:23-35) run in one small kernel that writes the env's next controls.
//
// This file: the host side (the context, the launches of a pass, the C entry points).  Beside it:
//   trsim_pilot_plan.hpp    host-only: which kernel serves which layer, the packing of the weights, the layout of the tail's fp32 blob
//   trsim_pilot_pass.hpp    host-only: the kernels' parameter blocks with every integer filled from the plan, and a pass as data: which launch computes which layers,
//                           from which buffer into which, on what grid (pilot_pass, pilot_materialise)
//   trsim_pilot_mma.hpp     the fragment-level pieces every convolution kernel is made of: vector types, fp16 conversions and the packed ReLU, the epilogue
//                           block (block_groups), the bias start (acc_from_bias), the ONE K loop over a weight ring (ring_k_loop), the 3x3 item and the
//                           staging that the frame kernel and the chain share (conv3x3_item, stage_run)
//   trsim_pilot_layers.hpp  the single-layer convolution kernels
//   trsim_pilot_fused.hpp   the fused convolution kernels: a 3x3 layer with its frames in LDS, conv4 .. conv7 in one launch, conv3 with its frames in LDS, conv1 -> conv2
//   trsim_pilot_tail.hpp    everything behind conv7: dense1's kernel, the two tail kernels and the one KerasPilot.step rule they share
//
// Numerics: binary16 (fp16) operands, fp32 accumulate, activations stored as binary16 (saturating at 65504) — checked against a
// PyTorch fp32 reference with the same fp16-rounded weights (tests/test_pilot.py, tolerance stated there).  Until round 2 the
// 16-bit format was bfloat16: the same MFMA rate, but 8 significant bits instead of 11 — measured max |output - fp32| 5.0e-4 against
// 4.4e-5 (profiles/r03_pilot_precision.txt); the reference's arithmetic is fp32 (keras_pilot.py:49-55).  Bound: MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <memory>
#include <vector>

#include "../../include/trsim.h"
#include "trsim_internal.hpp"
#include "trsim_mem.hpp"
#include "trsim_pilot_pass.hpp"   // host-only: the kernels' parameter blocks and the schedule of a pass; through it trsim_pilot_plan.hpp: the plan, the constants shared with
                                  // the kernels, the weight packing

namespace {

#include "trsim_pilot_mma.hpp"      // the fragment-level pieces: vector types, fp16 conversions, the epilogue block, the bias start, the K loop, the shared 3x3 item and its staging

using namespace trsim;   // (trsim_pilot_pass.hpp, trsim_pilot_plan.hpp, trsim_mem.hpp)
constexpr int kLayers = 11;               // conv1..7, dense1..3, output
#ifndef TRS_CONV_ABLATE
#define TRS_CONV_ABLATE 0   /* diagnostic builds of trs_conv_lt_kernel, never shipped: 1 = no steady-state global loads, 2 = no LDS transpose, 3 = no MFMA, 4 = no stores */
#endif
constexpr int kConvPrefetch = 4;           // trips (pairs of k-steps) of pixel fragments in flight per wave

extern __shared__ __attribute__((aligned(16))) unsigned char psmem[];

#include "trsim_pilot_layers.hpp"   // the single-layer kernels: conv1 as its own layer, the span kernel (conv2 unfused, conv3 at 240x320), the quad-load fallback
#include "trsim_pilot_fused.hpp"    // the fused kernels: the frame kernel (3x3 layers), the chain (conv4 .. conv7), frame5 (conv3) and the band head (conv1 -> conv2)

#include "trsim_pilot_tail.hpp"   // everything behind conv7: dense1's kernel, the two tails and KerasPilot.step's one rule, the range check's counter, the zeroed controls

// ---- the host side: the device buffers, and a pass launched as trsim_pilot_pass.hpp schedules it: its blocks get their pointers here ----
struct ConvLayer { trsim::DevBuf<u4v> w; trsim::DevBuf<float> bias; trsim::DevBuf<int> goff; };

struct PilotCtx {
    PilotPlan plan;                       // what trs_pilot_load decided for this frame size, batch capacity, device and tuning
    ConvLayer L[9];                       // conv1..7 + dense1 (1x1 "conv" over frames) [+ dense4: the second head of cnn_2d_full_house]
    trsim::DevBuf<void> act[9];           // outputs of L[i] for n_cap frames (fp16; act[7], act[8] float)
    trsim::DevBuf<float> xblob; TailLayout tail;   // the small fp32 weights the tail kernel reads, and where each lies (pack_tail_blob)
    trsim::DevBuf<void> slab2; int last_slices2 = 1;   // dense4 partial sums
    trsim::DevBuf<float> raw;             // [n_cap][2]
    trsim::DevBuf<uint8_t> tmp_frames; size_t tmp_cap = 0;   // room for tmp_cap bytes of frames and side inputs (+ the callers' padding)
    int last_n = 0, last_slices = 1;
    Fuse12Params fuse{};                  // conv1 -> conv2 in one kernel, band form (plan.head): all but the per-call fields
    const uint8_t* last_frames = nullptr; bool act0_valid = false;           // conv1's activation is only materialised on demand (debug getter)
    trsim::DevBuf<void> slab;             // dense1 partial sums [slices][n][100] fp32
    ChainParams chain{};                  // conv(plan.chain.first + 1) .. conv7 in one launch (trs_conv_chain_kernel): all but the per-call field
    bool chain_mid_valid = true;          // act[chain.first .. 5] hold the last pass (the chain never writes them; the debug getter runs the single layers on demand)
    trsim::DevBuf<u4v> w2_parity;         // conv2's granules in the band kernel's order (conv2_parity_order)
    void* train = nullptr;                // trsim_train.hip's session between trs_pilot_train_begin and _end (released by trs_train_free)
};

template <typename D, typename T>
int upload(trsim::DevBuf<D>& dst, const std::vector<T>& v)
{
    HIPCHK(dst.alloc(v.size() * sizeof(T)));
    HIPCHK(hipMemcpy(dst.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return TRS_OK;
}

// one launch of a schedule with dynamic LDS: the kernel may use up to a.lds_max, this launch gets a.lds
template <typename P>
int launch_lds(void (*kernel)(P), const PilotLaunch& a, hipStream_t s, const P& p)
{
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_max));
    hipLaunchKernelGGL(kernel, dim3(a.grid_x, a.grid_y), dim3(a.block), a.lds, s, p);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

using ConvKernel = void (*)(ConvParams);
ConvKernel single_kernel(PilotLaunchKind k)
{
    switch (k) {
    case kLaunchU8: return trs_conv_u8_kernel;
    case kLaunchSpan1: return trs_conv_span_kernel<1, false>;
    case kLaunchSpan2: return trs_conv_span_kernel<2, true>;
    case kLaunchLt1: return trs_conv_lt_kernel<1>;
    default: return trs_conv_lt_kernel<2>;
    }
}

// launch a of a schedule over n frames: its block (trsim_pilot_pass.hpp), the pointers, the kernel of its kind
int launch(PilotCtx* c, const PilotPass& pass, const PilotLaunch& a, const uint8_t* frames, int n, hipStream_t s)
{
    const PilotLayer& l = c->plan.L[a.first];
    const ConvLayer& cl = c->L[a.first];
    const void* const in = a.src == kBufFrames ? frames : c->act[a.src].get();
    void* const out = c->act[a.dst].get();
    auto in_w_bias_out = [&](auto& q) { q.in = static_cast<const u4v*>(in); q.w = cl.w.get(); q.bias = cl.bias.get(); q.out = static_cast<unsigned short*>(out); };
    switch (a.kind) {
    case kLaunchHeadWhole: case kLaunchHeadSplit: {
        Fuse12Params q = fuse12_call(c->fuse, c->plan, n, pass.head);
        q.frames = frames; q.c2.out = out;
        return launch_lds(a.kind == kLaunchHeadSplit ? trs_conv12_band_kernel<true> : trs_conv12_band_kernel<false>, a, s, q);
    }
    case kLaunchFrame5: {                                                   // one persistent 8-wave workgroup per CU: a unit (frame or row band) computed from one LDS buffer, the next staged into the other
        Frame5Params q = frame5_params(l, n);
        in_w_bias_out(q);
        return launch_lds(trs_conv_frame5_kernel<2, TRS_F5_NB, TRS_F5_R, kFrame5Block, TRS_F5_COMPUTE>, a, s, q);
    }
    case kLaunchFrame8: case kLaunchFrame16: {                              // one persistent workgroup per CU
        FrameConvParams q = frame_params(l, n);
        in_w_bias_out(q);
        return launch_lds(a.kind == kLaunchFrame8 ? trs_conv_frame_kernel<2, 2, 4, TRS_FRAME_R, 8, TRS_FRAME_LOADERS> : trs_conv_frame_kernel<2, 2, 8, TRS_FRAME_R, 8, TRS_FRAME_LOADERS>, a, s, q);
    }
    case kLaunchChain: {
        ChainParams q = chain_call(c->chain, n);
        q.in = static_cast<const u4v*>(in); q.out = static_cast<unsigned short*>(out);
        return launch_lds(trs_conv_chain_kernel<kChainBlock>, a, s, q);
    }
    case kLaunchDense1: case kLaunchDense2: {                               // one fp32 slab per K slice, added in order by the tail kernel
        trsim::DevBuf<void>& slab = a.dst == 7 ? c->slab : c->slab2;
        const size_t need = (size_t)pass.dense.KS * n * l.act_elems() * sizeof(float);
        if (slab.bytes() < need) {
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(slab.reserve(need));
        }
        DenseParams q = dense_params(l, pass.dense, n);
        q.act = static_cast<const u4v*>(in); q.w = cl.w.get(); q.bias = cl.bias.get(); q.slab = static_cast<float*>(slab.get());
        return launch_lds(a.kind == kLaunchDense2 ? trs_pilot_dense_kernel<2> : trs_pilot_dense_kernel<1>, a, s, q);
    }
    default: {
        ConvParams p = conv_params(l, n);
        p.in = in; p.w = cl.w.get(); p.bias = cl.bias.get(); p.goff = cl.goff.get(); p.out = out;
        return launch_lds(single_kernel(a.kind), a, s, p);
    }
    }
}

// a schedule over n frames launched in order, or refused whole; between: see forward
int run_schedule(PilotCtx* c, const PilotPass& pass, const TrsEnvView& v, const uint8_t* frames, int n, const TrsPilotX7Hook* between = nullptr)
{
    if (pass.err) return trs_internal_fail(pass.err, pass.err_text);
    for (int k = 0; k < pass.count; ++k) {
        if (int rc = launch(c, pass, pass.at[k], frames, n, v.stream)) return rc;
        if (between && pass.at[k].last == 6) { if (int rc = between->fn(between->arg, c->act[6].get(), n)) return rc; }
    }
    c->act0_valid = pass.act0_valid; c->chain_mid_valid = pass.chain_mid_valid;
    return TRS_OK;
}

// between: what a training step runs on conv7's activation before dense1 reads it (TrsPilotX7Hook, trsim_internal.hpp); nullptr everywhere else
int forward(PilotCtx* c, const TrsEnvView& v, const uint8_t* d_frames, int n, const TrsPilotX7Hook* between = nullptr)
{
    const PilotPass pass = pilot_pass(c->plan, n);
    if (int rc = run_schedule(c, pass, v, d_frames, n, between)) return rc;
    c->last_frames = d_frames; c->last_n = n;
    c->last_slices = pass.dense.KS;
    if (c->plan.arch == TRS_PILOT_FULL_HOUSE) c->last_slices2 = pass.dense.KS;   // dense4 has dense1's shape: one plan for both
    return TRS_OK;
}

// materialise what the fused kernels of the last forward pass kept in LDS, as far as layers lo..hi need it: conv1 behind the fused head (layer 0),
// the chain's interior layers
int materialise_layers(PilotCtx* c, const TrsEnvView& v, int lo, int hi)
{
    return run_schedule(c, pilot_materialise(c->plan, c->last_n, lo, hi, c->act0_valid, c->chain_mid_valid), v, c->last_frames, c->last_n);
}

struct ActIo { const float* speed; const float* segment; const uint8_t* mode; float *steer, *thr, *brk; };   // where KerasPilot.step's inputs / outputs live (device)

// the model type a caller asks for must be one the loaded weights can serve
int check_model_type(const PilotCtx* c, const trs_pilot_config* cfg)
{
    const int mt = cfg->model_type;
    const bool ok = c->plan.arch == TRS_PILOT_SPD_CTL ? (mt == TRS_PILOT_SPD_CTL || mt == TRS_PILOT_CNN_2D) : mt == c->plan.arch;
    if (!ok) return trs_internal_fail(TRS_ERR_ARG, "trs_pilot_config.model_type does not match the loaded weights (22 arrays: cnn_2d_speed_control / cnn_2d; 28: cnn_2d_speed_as_feature; 42: cnn_2d_full_house)");
    return TRS_OK;
}

// the block both tails share, from the view (a delayed one under an observation latency), the caller's arrays (io; nullptr: the env's own), cfg and act
StepIo step_io(const PilotCtx* c, const TrsEnvView& v, int n, float* raw_out, const trs_pilot_config* cfg, bool act, const ActIo* io)
{
    StepIo t{};
    t.raw_out = raw_out; t.n = n; t.act = act ? 1 : 0;
    t.speed = (io && io->speed) ? io->speed : v.speed;
    if (!act) return t;
    t.steer = v.ctl_steer; t.thr = v.ctl_thr; t.brk = v.ctl_brk;
    if (io) { t.mode = io->mode; t.steer = io->steer; t.thr = io->thr; t.brk = io->brk; }
    t.threshold = cfg->spd_ctl_threshold; t.rev_mult = cfg->spd_ctl_reverse_multiplier; t.brk_mult = cfg->spd_ctl_break_multiplier;
    t.use_break = cfg->spd_ctl_break; t.smooth = cfg->smooth_steering_enabled; t.smooth_thr = cfg->smooth_steering_threshold;
    t.capped = cfg->model_type == TRS_PILOT_CNN_2D || c->plan.arch == TRS_PILOT_SPD_FTR;
    return t;
}

int run_tail(PilotCtx* c, const TrsEnvView& v, int n, float* raw_out, const trs_pilot_config* cfg, bool act, const ActIo* io)
{
    const PilotPlan& P = c->plan;
    const float* const h1 = static_cast<const float*>(c->slab.get());
    const float* const B = c->xblob.get(); const int* const xo = c->tail.xo;
    const size_t h1_stride = (size_t)n * P.L[7].act_elems();
    const StepIo s = step_io(c, v, n, raw_out, cfg, act, io);
    if (P.arch == TRS_PILOT_SPD_CTL) {
        const TailParams t{h1, c->last_slices, h1_stride, B + xo[XO_W2], B + xo[XO_B2], B + xo[XO_W3], B + xo[XO_B3], B + xo[XO_W4], B + xo[XO_B4], s};
        hipLaunchKernelGGL(trs_pilot_tail_kernel, dim3((n + 3) / 4), dim3(256), 0, v.stream, t);
    } else {
        TailExParams t{};
        t.h1 = h1; t.h1_slices = c->last_slices; t.h1_stride = h1_stride;
        t.h4 = static_cast<const float*>(c->slab2.get()); t.h4_slices = c->last_slices2; t.h4_stride = (size_t)n * P.L[8].act_elems();
        t.blob = B; std::memcpy(t.xo, xo, sizeof t.xo);
        t.arch = P.arch; t.f1 = c->tail.f1; t.f2 = c->tail.f2; t.f3 = c->tail.f3;
        t.segment = io ? io->segment : nullptr; t.seg_idx = v.seg_idx; t.np = v.n_points > 0 ? v.n_points : 1;
        t.io = s;
        hipLaunchKernelGGL(trs_pilot_tail_ex_kernel, dim3((n + 3) / 4), dim3(256), 0, v.stream, t);
    }
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

// the whole pilot: convolutions, dense1 and the tail (raw_out = nullptr: the context's own buffer)
int forward_and_tail(PilotCtx* c, const TrsEnvView& v, const uint8_t* d_frames, int n, float* raw_out, const trs_pilot_config* cfg, bool act, const ActIo* io = nullptr)
{
    int rc = forward(c, v, d_frames, n);
    if (rc) return rc;
    return run_tail(c, v, n, raw_out ? raw_out : c->raw.get(), cfg, act, io);
}

// args[0] is None -> (0.0, 0.0, 0.0) (keras_pilot.py:46-47)
int zero_controls(const TrsEnvView& v, float* steer, float* thr, float* brk, int n)
{
    hipLaunchKernelGGL(trs_zero_controls_kernel, dim3((n + 255) / 256), dim3(256), 0, v.stream, steer, thr, brk, n);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

// how every entry point behind trs_pilot_load begins: the handle's view and its loaded pilot (need_pass: one that has run a forward pass)
int enter(trs_env* e, TrsEnvView* v, PilotCtx** c, bool need_pass = false)
{
    if (!trs_internal_view(e, v)) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    *c = static_cast<PilotCtx*>(*trs_internal_pilot_slot(e));
    if (!*c || (need_pass && !(*c)->last_n)) return trs_internal_fail(TRS_ERR_STATE, need_pass ? "no forward pass yet" : "no pilot loaded");
    return TRS_OK;
}

// the frames a call reads: the caller's, or the env's latest ones for a call over all its envs; may_be_none: before the first rendered step the answer is nullptr,
// not a refusal.  `text` is the entry point's own refusal.
int frames_or_latest(const TrsEnvView& v, const uint8_t** d_frames, int n, bool may_be_none, const char* text)
{
    if (*d_frames) return TRS_OK;
    if ((!may_be_none && !v.latest_frame) || n != v.n) return trs_internal_fail(TRS_ERR_ARG, text);
    *d_frames = v.latest_frame;
    return TRS_OK;
}
const char* const kLatestNeeds = "latest-frame source needs a rendered step and n_images == n_envs";

// what the two host variants share behind their checks: frames and the side inputs given are staged in the temporary buffer, the pass runs by the rule of the
// device entry point (with side inputs trs_pilot_forward_ex's; without, and for cnn_2d_speed_control always, trs_pilot_forward's: the env's own speed,
// n_images == n_envs for the other model types), the outputs are read back
int forward_staged(trs_env* e, PilotCtx* c, const TrsEnvView& v, const uint8_t* h_frames, const float* h_speed, const float* h_segment, int n, float* h_out)
{
    HIPCHK(hipSetDevice(v.device));
    const size_t bytes = (size_t)n * c->plan.H * c->plan.W * 3, extra = (size_t)n * 8;
    if (bytes + extra > c->tmp_cap) {
        HIPCHK(hipStreamSynchronize(v.stream));
        c->tmp_cap = 0;
        HIPCHK(c->tmp_frames.alloc(bytes + extra + 128));
        c->tmp_cap = bytes + extra;
    }
    uint8_t* const d_frames = c->tmp_frames.get();
    float* const d_spd = reinterpret_cast<float*>(d_frames + ((bytes + 63) & ~(size_t)63));
    float* const d_seg = d_spd + n;
    HIPCHK(hipMemcpyAsync(d_frames, h_frames, bytes, hipMemcpyHostToDevice, v.stream));
    if (h_speed) HIPCHK(hipMemcpyAsync(d_spd, h_speed, (size_t)n * 4, hipMemcpyHostToDevice, v.stream));
    if (h_segment) HIPCHK(hipMemcpyAsync(d_seg, h_segment, (size_t)n * 4, hipMemcpyHostToDevice, v.stream));
    int rc = (h_speed && c->plan.arch != TRS_PILOT_SPD_CTL) ? trs_pilot_forward_ex(e, d_frames, d_spd, h_segment ? d_seg : nullptr, n, nullptr)
                                                            : trs_pilot_forward(e, d_frames, n, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_out, c->raw.get(), (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, v.stream));
    trs_internal_count(e, (uint64_t)n * 2 * sizeof(float), (uint64_t)bytes);
    HIPCHK(hipStreamSynchronize(v.stream));
    return TRS_OK;
}

}  // namespace

void trs_pilot_free(void* ctx)
{
    PilotCtx* const c = static_cast<PilotCtx*>(ctx);
    if (c) trs_train_free(c->train);
    delete c;
}

// ---- what trsim_train.hip needs of the loaded pilot (trsim_internal.hpp) ----
namespace {
void fill_tail(PilotCtx* c, TrsPilotTail* t)
{
    const PilotPlan& P = c->plan;
    float* const B = c->xblob.get(); const int* const xo = c->tail.xo;
    t->arch = P.arch; t->n_cap = P.n_cap; t->F = (size_t)P.L[7].CIN; t->G = P.L[7].G;
    t->x7 = c->act[6].get();
    t->slab = static_cast<const float*>(c->slab.get()); t->slices = c->last_slices; t->slab_stride = (size_t)c->last_n * P.L[7].act_elems();
    t->w1_pack = reinterpret_cast<unsigned short*>(c->L[7].w.get()); t->b1 = c->L[7].bias.get();
    t->w2 = B + xo[XO_W2]; t->b2 = B + xo[XO_B2]; t->w3 = B + xo[XO_W3]; t->b3 = B + xo[XO_B3]; t->w4 = B + xo[XO_W4]; t->b4 = B + xo[XO_B4];
    const int side[7] = {XO_W1Y, XO_F1W, XO_F1B, XO_F2W, XO_F2B, XO_F3W, XO_F3B};
    for (int j = 0; j < 7; ++j) t->side[j] = P.arch == TRS_PILOT_SPD_CTL ? nullptr : B + xo[side[j]];
    t->train = &c->train;
}
}  // namespace

int trs_internal_pilot_tail(trs_env* e, TrsEnvView* v, TrsPilotTail* t)
{
    PilotCtx* c;
    if (int rc = enter(e, v, &c)) return rc;
    fill_tail(c, t);
    return TRS_OK;
}

int trs_internal_pilot_dense_forward(trs_env* e, const TrsEnvView& v, const uint8_t* d_frames, int n, TrsPilotTail* t, const TrsPilotX7Hook* between)
{
    PilotCtx* const c = static_cast<PilotCtx*>(*trs_internal_pilot_slot(e));
    if (int rc = forward(c, v, d_frames, n, between)) return rc;
    fill_tail(c, t);
    return TRS_OK;
}

int trs_internal_pilot_convs(trs_env* e, const TrsEnvView& v, bool materialise, TrsPilotConvs* out)
{
    PilotCtx* const c = static_cast<PilotCtx*>(*trs_internal_pilot_slot(e));
    if (!c) return trs_internal_fail(TRS_ERR_STATE, "no pilot loaded");
    if (materialise) { if (int rc = materialise_layers(c, v, 3, 5)) return rc; }
    const PilotPlan& P = c->plan;
    out->n_cap = P.n_cap; out->cu_count = P.cu_count;
    for (int j = 0; j < 4; ++j) {
        const PilotLayer& l = P.L[3 + j];
        out->L[j] = TrsPilotConvs::Layer{l.IH, l.IW, l.OH, l.OW, l.CIN, l.COUT, l.COUT_PAD, l.run_pad, c->act[2 + j].get(), c->act[3 + j].get(),
                                         reinterpret_cast<unsigned short*>(c->L[3 + j].w.get()), c->L[3 + j].bias.get()};
    }
    return TRS_OK;
}

TRS_EXPORT void trs_default_pilot_config(trs_pilot_config* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->struct_size = (uint32_t)sizeof *c;
    c->spd_ctl_threshold = 1.1f; c->spd_ctl_break = 0; c->spd_ctl_reverse_multiplier = 1.0f; c->spd_ctl_break_multiplier = 1.0f;
    c->smooth_steering_enabled = 0; c->smooth_steering_threshold = 0.9f;
}

TRS_EXPORT void trs_default_pilot_tuning(trs_pilot_tuning* t) { if (t) *t = pilot_default_tuning(); }

TRS_EXPORT int trs_pilot_set_tuning(trs_env* e, const trs_pilot_tuning* t)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (t && t->struct_size != sizeof(trs_pilot_tuning)) return trs_internal_fail(TRS_ERR_ARG, "trs_pilot_tuning.struct_size does not match this library (start from trs_default_pilot_tuning)");
    if (const PilotCtx* c = static_cast<const PilotCtx*>(*trs_internal_pilot_slot(e)); c && c->train)
        return trs_internal_fail(TRS_ERR_STATE, "a training session is open on this pilot: trs_pilot_train_end first");
    trs_internal_set_pilot_tuning(e, t);
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_load(trs_env* e, const float* const* arr, int n_arrays)
{
    TrsEnvView v;
    if (!trs_internal_view(e, &v)) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (!arr || (n_arrays != 2 * kLayers && n_arrays != 28 && n_arrays != 42))
        return trs_internal_fail(TRS_ERR_ARG, "expected 22 arrays: kernel and bias of conv1..conv7, dense1..dense3, output_layer (28 with feature1..3 for cnn_2d_speed_as_feature; "
                                              "42 for cnn_2d_full_house: ..., output_speed, feature1..3, current_spd_1..3, dense4..6, out_steering)");
    for (int i = 0; i < n_arrays; ++i) if (!arr[i]) return trs_internal_fail(TRS_ERR_ARG, "null weight array");
    void** slot = trs_internal_pilot_slot(e);
    if (*slot && static_cast<PilotCtx*>(*slot)->train)
        return trs_internal_fail(TRS_ERR_STATE, "a training session is open on this pilot: trs_pilot_train_end first");
    HIPCHK(hipSetDevice(v.device));
    if (*slot) { HIPCHK(hipStreamSynchronize(v.stream)); delete static_cast<PilotCtx*>(*slot); *slot = nullptr; }
    // the context under construction is freed on EVERY early return below (HIPCHK included); released into the handle at the end
    std::unique_ptr<PilotCtx> guard(new PilotCtx());
    PilotCtx* const c = guard.get();
    // ---- plan: which kernel serves which layer, every LDS layout (trsim_pilot_plan.hpp) ----
    const trs_pilot_tuning* const user = trs_internal_pilot_tuning(e);
    int cu_count = 256;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, v.device) == hipSuccess && prop.multiProcessorCount > 0) cu_count = prop.multiProcessorCount; }
    c->plan = pilot_plan(v.H, v.W, v.n, cu_count, n_arrays, user ? *user : pilot_default_tuning());
    const PilotPlan& P = c->plan;
    if (P.err) return trs_internal_fail(P.err, P.err_text);
    // ---- pack the Keras arrays, allocate and upload ----
    for (int i = 0; i < P.n_layers; ++i) {
        const PilotLayer& l = P.L[i];
        ConvLayer& cl = c->L[i];
        const int ai = i == 8 ? 34 : 2 * i;                               // dense4 of the full-house model
        const PackedLayer pk = pack_layer(l, arr[ai], arr[ai + 1]);
        int rc = upload(cl.w, pk.w); if (!rc) rc = upload(cl.bias, pk.bias); if (!rc) rc = upload(cl.goff, pk.goff);
        if (!rc && i == 1 && P.head.on) rc = upload(c->w2_parity, conv2_parity_order(l, pk.w));
        if (rc) return rc;
        HIPCHK(c->act[i].alloc((size_t)P.n_cap * l.act_elems() * (l.out_f32 ? 4 : 2) + 64));
    }
    {   // the small fp32 weights behind dense1: one blob, offsets by XO_*
        const TailBlob blob = pack_tail_blob(P, arr);
        int rc = upload(c->xblob, blob.data); if (rc) return rc;
        c->tail = blob;
    }
    // ---- the parameter blocks of the two fused kernels, all but their per-call fields (trsim_pilot_pass.hpp), and their pointers ----
    if (P.head.on) {
        Fuse12Params& q = c->fuse = fuse12_params(P, conv1_bounded(P.L[0], arr[0], arr[1]));
        q.w1 = c->L[0].w.get(); q.b1 = c->L[0].bias.get(); q.w2 = c->w2_parity.get(); q.c2.bias = c->L[1].bias.get();
    }
    if (P.chain.first >= 0) {
        c->chain = chain_params(P);
        for (int j = 0; j < P.chain.nl; ++j) { c->chain.L[j].w = c->L[P.chain.first + j].w.get(); c->chain.L[j].bias = c->L[P.chain.first + j].bias.get(); }
    }
    HIPCHK(c->raw.alloc((size_t)P.n_cap * 2 * sizeof(float)));
    *slot = guard.release();
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_forward(trs_env* e, const uint8_t* d_frames, int n_images, float* d_out)
{
    TrsEnvView v; PilotCtx* c;
    if (int rc = enter(e, &v, &c)) return rc;
    if (n_images < 1 || n_images > c->plan.n_cap) return trs_internal_fail(TRS_ERR_ARG, "n_images must be in [1, n_envs]");
    HIPCHK(hipSetDevice(v.device));
    if (int rc = frames_or_latest(v, &d_frames, n_images, false, kLatestNeeds)) return rc;
    if (c->plan.arch != TRS_PILOT_SPD_CTL && n_images != v.n)
        return trs_internal_fail(TRS_ERR_ARG, "this model type also reads speed (and segment): use trs_pilot_forward_ex, or n_images == n_envs for the env's own");
    return forward_and_tail(c, v, d_frames, n_images, d_out, nullptr, false);
}

TRS_EXPORT int trs_pilot_forward_ex(trs_env* e, const uint8_t* d_frames, const float* d_speed, const float* d_segment, int n_images, float* d_out)
{
    TrsEnvView v; PilotCtx* c;
    if (int rc = enter(e, &v, &c)) return rc;
    if (n_images < 1 || n_images > c->plan.n_cap) return trs_internal_fail(TRS_ERR_ARG, "n_images must be in [1, n_envs]");
    if ((!d_speed || (c->plan.arch == TRS_PILOT_FULL_HOUSE && !d_segment)) && n_images != v.n) return trs_internal_fail(TRS_ERR_ARG, "the env's own speed / segment need n_images == n_envs");
    HIPCHK(hipSetDevice(v.device));
    if (int rc = frames_or_latest(v, &d_frames, n_images, false, kLatestNeeds)) return rc;
    const ActIo io{d_speed, d_segment, nullptr, nullptr, nullptr, nullptr};
    return forward_and_tail(c, v, d_frames, n_images, d_out, nullptr, false, &io);
}

TRS_EXPORT int trs_pilot_forward_host_ex(trs_env* e, const uint8_t* h_frames, const float* h_speed, const float* h_segment, int n_images, float* h_out)
{
    TrsEnvView v; PilotCtx* c;
    if (int rc = enter(e, &v, &c)) return rc;
    if (!h_frames || !h_out || n_images < 1 || n_images > c->plan.n_cap) return trs_internal_fail(TRS_ERR_ARG, "bad argument (n_images must be in [1, n_envs])");
    if (c->plan.arch != TRS_PILOT_SPD_CTL && (!h_speed || (c->plan.arch == TRS_PILOT_FULL_HOUSE && !h_segment))) return trs_internal_fail(TRS_ERR_ARG, "this model type needs speed (and segment) arrays");
    return forward_staged(e, c, v, h_frames, h_speed, h_segment, n_images, h_out);
}

TRS_EXPORT int trs_pilot_forward_host(trs_env* e, const uint8_t* h_frames, int n_images, float* h_out)
{
    TrsEnvView v; PilotCtx* c;
    if (int rc = enter(e, &v, &c)) return rc;
    if (!h_frames || !h_out || n_images < 1 || n_images > c->plan.n_cap) return trs_internal_fail(TRS_ERR_ARG, "bad argument (n_images must be in [1, n_envs])");
    return forward_staged(e, c, v, h_frames, nullptr, nullptr, n_images, h_out);
}

TRS_EXPORT int trs_pilot_debug_layer(trs_env* e, int layer, float* h_dst, size_t n_floats)
{
    TrsEnvView v; PilotCtx* c;
    if (int rc = enter(e, &v, &c, true)) return rc;
    if (layer < 0 || layer > 7 || !h_dst) return trs_internal_fail(TRS_ERR_ARG, "bad layer");
    const size_t total = (size_t)c->last_n * c->plan.L[layer].act_elems();
    if (n_floats != total) return trs_internal_fail(TRS_ERR_ARG, "size mismatch");
    HIPCHK(hipSetDevice(v.device));
    { int rc = materialise_layers(c, v, layer, layer); if (rc) return rc; }   // what the fused kernels kept in LDS: only what this layer needs
    HIPCHK(hipStreamSynchronize(v.stream));
    if (c->plan.L[layer].out_f32) {                                              // dense1: add the K-slice slabs in slice order, then the ReLU (both live in the tail kernel)
        std::vector<float> part(total);
        for (size_t i = 0; i < total; ++i) h_dst[i] = 0.0f;
        for (int sl = 0; sl < c->last_slices; ++sl) {
            HIPCHK(hipMemcpy(part.data(), static_cast<const float*>(c->slab.get()) + (size_t)sl * total, total * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < total; ++i) h_dst[i] += part[i];
        }
        for (size_t i = 0; i < total; ++i) h_dst[i] = h_dst[i] > 0.0f ? h_dst[i] : 0.0f;
        return TRS_OK;
    }
    std::vector<unsigned short> tmp(total);
    HIPCHK(hipMemcpy(tmp.data(), c->act[layer].get(), total * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < total; ++i) h_dst[i] = host_h2f(tmp[i]);
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_range_check(trs_env* e, uint64_t h_out[8])
{
    TrsEnvView v; PilotCtx* c;
    if (int rc = enter(e, &v, &c, true)) return rc;
    if (!h_out) return trs_internal_fail(TRS_ERR_ARG, "null output");
    HIPCHK(hipSetDevice(v.device));
    { int rc = materialise_layers(c, v, 0, 6); if (rc) return rc; }
    unsigned long long* const scratch = v.stats + 24;                       // stats[24..30]: this call's per-layer counts; stats[3]: running total
    HIPCHK(hipMemsetAsync(scratch, 0, 8 * sizeof(unsigned long long), v.stream));
    for (int i = 0; i < 7; ++i) {
        const size_t n = (size_t)c->last_n * c->plan.L[i].act_elems();
        const int grid = (int)std::min<size_t>(4096, (n + 255) / 256);
        hipLaunchKernelGGL(trs_pilot_count_sat_kernel, dim3(grid), dim3(256), 0, v.stream, static_cast<const unsigned short*>(c->act[i].get()), n, scratch + i, v.stats + 3);
    }
    HIPCHK(hipGetLastError());
    unsigned long long host[8] = {};
    HIPCHK(hipMemcpyAsync(host, scratch, sizeof host, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    host[7] = 0;
    for (int i = 0; i < 7; ++i) { h_out[i] = host[i]; host[7] += host[i]; }
    h_out[7] = host[7];
    return TRS_OK;
}

TRS_EXPORT int trs_pilot_act(trs_env* e, const trs_pilot_config* cfg, const uint8_t* d_frames, const float* d_speed, const float* d_segment,
                             const uint8_t* d_mode, float* d_steer, float* d_thr, float* d_brk, int n)
{
    TrsEnvView v; PilotCtx* c;
    if (int rc = enter(e, &v, &c)) return rc;
    if (!cfg || cfg->struct_size != sizeof(trs_pilot_config)) return trs_internal_fail(TRS_ERR_ARG, "trs_pilot_config.struct_size mismatch");
    { int rm = check_model_type(c, cfg); if (rm) return rm; }
    if (!d_steer || !d_thr || !d_brk || n < 0 || n > c->plan.n_cap) return trs_internal_fail(TRS_ERR_ARG, "null output or n out of range (n <= n_envs)");
    if ((!d_speed || (c->plan.arch == TRS_PILOT_FULL_HOUSE && !d_segment)) && n != v.n) return trs_internal_fail(TRS_ERR_ARG, "the env's own speed / segment need n == n_envs");
    HIPCHK(hipSetDevice(v.device));
    if (n == 0) return TRS_OK;
    if (int rc = frames_or_latest(v, &d_frames, n, true, "latest-frame source needs n == n_envs")) return rc;
    if (!d_frames) return zero_controls(v, d_steer, d_thr, d_brk, n);       // no frame rendered yet
    const ActIo io{d_speed, d_segment, d_mode, d_steer, d_thr, d_brk};
    return forward_and_tail(c, v, d_frames, n, nullptr, cfg, true, &io);
}

int trs_internal_pilot_loop_check(trs_env* e, const trs_pilot_config* cfg, int n_steps)
{
    TrsEnvView v; PilotCtx* c;
    if (int rc = enter(e, &v, &c)) return rc;
    if (!cfg || cfg->struct_size != sizeof(trs_pilot_config)) return trs_internal_fail(TRS_ERR_ARG, "trs_pilot_config.struct_size mismatch");
    if (n_steps < 1) return trs_internal_fail(TRS_ERR_ARG, "n_steps < 1");
    { int rm = check_model_type(c, cfg); if (rm) return rm; }
    if (!v.render) return trs_internal_fail(TRS_ERR_STATE, "the pilot needs a camera (render = 1)");
    HIPCHK(hipSetDevice(v.device));
    return TRS_OK;
}

int trs_internal_pilot_tick(trs_env* e, const trs_pilot_config* cfg, TrsEnvView* view, const uint8_t** fed)
{
    TrsEnvView& v = *view;
    PilotCtx* const c = static_cast<PilotCtx*>(*trs_internal_pilot_slot(e));
    if (int rc = trs_internal_tick_view(e, &v)) return rc;
    const uint8_t* seen = v.obs_on ? v.obs_frame : v.latest_frame;      // the frame the pilot reads today (nullptr: none yet)
    if (seen && v.codec_quality) {              // a camera codec is set: the pilot reads codec(that frame), as the reference's pilot reads decoded JPEGs
        int rc = trs_internal_camera_codec(e, seen, &seen);
        if (rc) return rc;
    }
    // KerasPilot.step on the frame of the previous tick and the env's own speed and segment.  With an observation latency: on what each car has been told
    // (frame, speed, segment), and (0, 0, 0) for the cars nothing has reached yet (keras_pilot.py:46-47) through the rule's mode mask
    TrsEnvView o = v;
    ActIo io{nullptr, nullptr, nullptr, v.ctl_steer, v.ctl_thr, v.ctl_brk};
    if (v.obs_on) { o.speed = v.obs_speed; o.seg_idx = v.obs_seg_idx; io.mode = v.obs_mode; }
    *fed = seen;
    return seen ? forward_and_tail(c, o, seen, v.n, nullptr, cfg, true, &io) : zero_controls(v, v.ctl_steer, v.ctl_thr, v.ctl_brk, v.n);
}

TRS_EXPORT int trs_step_pilot(trs_env* e, const trs_pilot_config* cfg, int n_steps)
{
    if (int rc = trs_internal_pilot_loop_check(e, cfg, n_steps)) return rc;
    struct Ops : TrsLoopOps {
        const trs_pilot_config* cfg;
        int observe(const uint8_t** fed) { return trs_internal_pilot_tick(e, cfg, &v, fed); }
        int label(int) { return TRS_OK; }                   // the pilot's controls are the applied ones
    } ops{{e, nullptr, {}}, cfg};
    return trsim::closed_loop(ops, n_steps, nullptr, nullptr, nullptr);   // no driver, no capture
}
