// trsim_pilot_pass.hpp — what a pass of the pilot launches, as data a host compiler builds without the GPU's headers: the parameter block of every kernel
// of the pass with every integer filled from the plan (trsim_pilot_plan.hpp), and the schedule itself — which launch computes which layers, from which
// buffer into which, on what grid (pilot_pass: a forward pass of n frames; pilot_materialise: what the debug getter and the training units ask for afterwards).
// trsim_pilot.hip walks a schedule, adds the device pointers and launches; tests/pilot_plan_driver.cpp prints it on the CPU.
#pragma once
#include "trsim_pilot_plan.hpp"

namespace trsim {

// a 16-byte granule of 8 fp16 values in device memory.  The blocks only point at it: a host compiler without the vector extension sees an incomplete type
#if defined(__clang__)
typedef unsigned u4v __attribute__((ext_vector_type(4)));
#else
struct u4v;
#endif

constexpr float kConv1Scale = 1.0f / 256.0f;   // conv1's weights carry 256 / 255 (the pilot's / 255 of keras_pilot.py:49-50 x 2^8, so that small weights stay normal
                                               // binary16 numbers); its epilogues multiply the sum by 2^-8 inside the bias FMA: exact, no extra instruction

// ---- the parameter blocks: members, order and types are the kernels' argument layout ----------------------------------------------
struct ConvParams {            // the single-layer kernels (trsim_pilot_layers.hpp)
    const void* in;            // fp16 NHWC [N][IH][IW][CIN]   (conv1: uint8 [N][IH][IW][3])
    const u4v* w;              // [G_pad][COUT_PAD] granules of 8 fp16
    const float* bias;         // [COUT_PAD]
    const int* goff;           // [G_pad] byte offset of granule g relative to the output pixel's input base
    void* out;                 // fp16 NHWC [N][OH][OW][COUT]
    int in_bytes;              // size of `in` (buffer-load bounds)
    int N, IH, IW, CIN, OH, OW, COUT, COUT_PAD, S;
    int G, G_pad, M;           // granules (even-padded), GEMM rows = N*OH*OW
    int in_px_bytes;           // bytes per input pixel (CIN*2, conv1: 3)
    int nt_out;                // non-temporal activation stores (outputs far larger than L2; measured: conv1 86 -> 80 us, small layers lose)
    int KH, KW, run_pad, cg, span_nl;   // span kernel: kernel rows, granules per kernel row (padded), granules per pixel, load instructions per kernel row
    float oscale;              // the sums are multiplied by this power of two inside the bias FMA: 2^-8 for conv1 (kConv1Scale), 1 elsewhere
};
struct FrameConvParams {       // trs_conv_frame_kernel
    const u4v* in;             // fp16 NHWC [N][IH][IW][CIN] as 16-B granules
    const u4v* w;              // [KH*KW*cg][COUT_PAD] granules (kernel-row major, then tap, then channel granule)
    const float* bias;
    unsigned short* out;       // fp16 NHWC [N][OH][OW][COUT]
    int N, IH, IW, OH, OW, COUT, COUT_PAD, KH, KW;
    int F, cg, cgs;            // units (frames, or row bands of frames) per workgroup; granules per pixel (8 / 16) and log2 of it
    int bands, ohb, ihb;       // a frame whose activation does not fit LDS is cut into `bands` bands of ohb output rows = ohb + KH - 1 input rows
                               // (neighbouring bands re-stage KH - 1 rows); bands == 1: ohb = OH, ihb = IH
    unsigned magic_uout, magic_ow, magic_bands;   // floor(p / d) = umulhi(p, ceil(2^32 / d)), exact for p < 2^32 / d: d = ohb x OW, OW, bands (an item's set-up without divisions)
};
struct ChainLayer {            // a layer of trs_conv_chain_kernel
    const u4v* w; const float* bias;
    int IH, IW, OH, OW, COUT, cg, cgs;     // COUT == COUT_PAD (64 / 128); cg = input granules per pixel (8 / 16), cgs = log2
    int nt, nb;                            // a wave item = nt x 32 pixels x nb x 32 channels (nt 2 / 3, nb 1 / 2): the choice that leaves the busiest SIMD the fewest MFMAs
    unsigned magic_uout, magic_ow;         // floor(p / (OH x OW)) = umulhi(p, magic_uout), floor(p / OW) = umulhi(p, magic_ow) for p < 65536 (an item's set-up: four divisions
                                           // per tile cost ~100 vector instructions per item — a K loop is 36 k-steps of ~25)
};
struct ChainParams {
    const u4v* in;             // the first layer's input activation, fp16 NHWC
    unsigned short* out;       // the last layer's output activation
    int N, F, nl, split_first; // frames, frames per workgroup, layers (3 = conv5..7, 4 = conv4..7), first layer in two passes of F / 2 frames
    int offA, offB, off_bias;  // LDS byte offsets
    ChainLayer L[4];           // every layer but the last reads 64 channels (HALF = 4), the last 128 (HALF = 8)
};
struct Frame5Params {          // trs_conv_frame5_kernel
    const u4v* in;             // fp16 NHWC [N][IH][IW][32]
    const u4v* w;              // [KH*KW*4][64] granules: row (kh, kw, c8), 2 k + h = granule of k-step k, half h
    const float* bias;
    unsigned short* out;       // fp16 NHWC [N][OH][OW][64]
    int N, IH, IW, OH, OW, F, ev, COUT;   // ev = even columns per row = (IW + 1) / 2
    int bands, ohb, ihb;                  // a frame that does not fit LDS is cut into `bands` bands of ohb output rows = ihb = 2 ohb + 3 input rows (bands == 1: ohb = OH, ihb = IH)
    unsigned magic_ow;                    // floor(p / OW) = umulhi(p, magic_ow)
};
struct Fuse12Params {          // trs_conv12_band_kernel
    const uint8_t* frames; int frames_bytes;
    const u4v* w1; const float* b1;                        // conv1: [12][32] granules, [32]
    const u4v* w2;                                          // conv2: [80][32] granules (kernel rows padded 15 -> 16)
    ConvParams c2;                                          // conv2's output side (out, M, bias)
    int N, IH, IW, OH1, OW1, OH2, OW2, R2, bands;
    int off_w2, off_b, off_tile;                            // LDS layout
    int tile_bytes;
    int off_band, band_bytes;                               // band kernel: the frame rows under the conv1 tile as fp16 [rows][IW * 3]
    int wsplit, w2p, cpr;                                   // band kernel cut in width: parts per band, conv2 columns per part, 16-byte chunks per staged row
    int roll;                                               // band kernel: a workgroup walks the bands of a (frame, part) top to bottom and keeps the 3 shared conv1 rows (see the kernel)
    int c1_bounded;                                         // conv1's sums provably stay inside binary16 (|bias| + sum |w| < 65504, pixels / 256 <= 1): its epilogue skips the saturation
    unsigned magic_full, magic_cpr;                         // floor(p / w1) = umulhi(p, magic_full) for a part's conv1 width 2 w2p + 3; the same for / cpr
};
struct DenseParams {           // trs_pilot_dense_kernel
    const u4v* act;            // conv7's output: fp16 [n][G] granules (the NHWC flatten)
    const u4v* w;              // [G][128] granules
    const float* bias;         // [128]
    float* slab;               // [KS][n][100] fp32
    int n, G, gps, KS, groups;
};

// ---- every block with all its integers, from the plan: the pointers come back null ----------------------------------------------------
inline int granule_shift(int cg) { return cg == 8 ? 3 : 4; }                // log2 of the granules per pixel (8 / 16)

inline ConvParams conv_params(const PilotLayer& l, int n)
{
    ConvParams p{};
    p.N = n; p.IH = l.IH; p.IW = l.IW; p.CIN = l.CIN; p.OH = l.OH; p.OW = l.OW; p.COUT = l.COUT; p.COUT_PAD = l.COUT_PAD; p.S = l.S;
    p.G = l.G; p.G_pad = l.G_pad; p.M = n * l.OH * l.OW;
    p.in_px_bytes = l.u8in ? 3 : l.CIN * 2;
    p.in_bytes = (int)((size_t)n * l.IH * l.IW * p.in_px_bytes);           // (pilot_pass refuses a batch whose input does not fit an int)
    p.oscale = l.u8in ? kConv1Scale : 1.0f;
    // outputs above 128 MB leave non-temporally (measured: conv1's 222 MB -> conv1 88 -> 81 us, conv2 85 -> 82; at 48 MB conv3 loses)
    p.nt_out = (!l.out_f32 && (size_t)p.M * l.COUT * 2 > ((size_t)128 << 20)) ? 1 : 0;
    p.KH = l.KH; p.KW = l.KW; p.run_pad = l.run_pad; p.cg = l.u8in ? 0 : l.CIN / 8; p.span_nl = l.span_nl;
    return p;
}
// (wave items of 2 x 32 pixels x 64 channels: the plan cuts the frames into bands so that a group has about 8 of them — items of 3 tiles need
// more than the 168 registers that 12 waves leave each)
inline FrameConvParams frame_params(const PilotLayer& l, int n)
{
    FrameConvParams q{};
    q.N = n; q.IH = l.IH; q.IW = l.IW; q.OH = l.OH; q.OW = l.OW; q.COUT = l.COUT; q.COUT_PAD = l.COUT_PAD; q.KH = l.KH; q.KW = l.KW;
    q.F = l.frame_f; q.cg = l.CIN / 8; q.cgs = granule_shift(q.cg);
    q.bands = l.frame_bands; q.ohb = l.frame_ohb; q.ihb = l.frame_ohb + l.KH - 1;
    q.magic_uout = pilot_magic(q.ohb * q.OW); q.magic_ow = pilot_magic(q.OW); q.magic_bands = q.bands == 1 ? 0u : pilot_magic(q.bands);
    return q;
}
inline Frame5Params frame5_params(const PilotLayer& l, int n)
{
    Frame5Params q{};
    q.N = n; q.IH = l.IH; q.IW = l.IW; q.OH = l.OH; q.OW = l.OW; q.F = 1; q.ev = (l.IW + 1) / 2; q.COUT = l.COUT;
    q.bands = l.frame5_bands; q.ohb = l.frame5_ohb; q.ihb = l.frame5_bands == 1 ? l.IH : 2 * l.frame5_ohb + 3; q.magic_ow = pilot_magic(l.OW);
    return q;
}
// all but the per-call field N (chain_call)
inline ChainParams chain_params(const PilotPlan& P)
{
    const PilotChain& h = P.chain;
    ChainParams q{};
    q.F = h.F; q.nl = h.nl; q.split_first = h.split_first; q.offA = h.offA; q.offB = h.offB; q.off_bias = h.off_bias;
    for (int j = 0; j < h.nl; ++j) {
        const PilotLayer& l = P.L[h.first + j];
        q.L[j] = ChainLayer{nullptr, nullptr, l.IH, l.IW, l.OH, l.OW, l.COUT, l.CIN / 8, granule_shift(l.CIN / 8), h.nt[j], h.nb[j], h.magic_uout[j], h.magic_ow[j]};
    }
    return q;
}
inline ChainParams chain_call(ChainParams q, int n) { q.N = n; return q; }
// all but the per-call fields (fuse12_call); c1_bounded: conv1_bounded of the loaded weights
inline Fuse12Params fuse12_params(const PilotPlan& P, int c1_bounded)
{
    const PilotLayer& l0 = P.L[0]; const PilotLayer& l1 = P.L[1]; const PilotHead& h = P.head;
    Fuse12Params q{};
    q.c2.COUT = l1.COUT; q.c2.COUT_PAD = l1.COUT_PAD; q.c2.oscale = 1.0f;
    q.IH = l0.IH; q.IW = l0.IW; q.OH1 = l0.OH; q.OW1 = l0.OW; q.OH2 = l1.OH; q.OW2 = l1.OW;
    q.R2 = h.R2; q.bands = h.bands; q.wsplit = h.wsplit; q.w2p = h.w2p; q.cpr = h.cpr; q.magic_full = h.magic_full; q.magic_cpr = h.magic_cpr;
    q.off_w2 = h.off_w2; q.off_b = h.off_b; q.off_tile = h.off_tile; q.tile_bytes = h.tile_bytes; q.off_band = h.off_band; q.band_bytes = h.band_bytes;
    q.c1_bounded = c1_bounded;
    return q;
}
inline Fuse12Params fuse12_call(Fuse12Params q, const PilotPlan& P, int n, const HeadCall& hc)
{
    q.frames_bytes = (int)((size_t)n * P.H * P.W * 3); q.N = n;            // (pilot_pass refuses frames that do not fit an int)
    q.c2.M = n * P.L[1].OH * P.L[1].OW; q.c2.nt_out = 0;
    q.roll = hc.roll;
    return q;
}
inline DenseParams dense_params(const PilotLayer& l, const DenseCall& d, int n)
{
    DenseParams q{};
    q.n = n; q.G = l.G; q.gps = d.gps; q.KS = d.KS; q.groups = d.groups;
    return q;
}

// ---- a pass as data ---------------------------------------------------------------------------------------------------------------------
// The kernel (and template instance) of a launch.  The head takes conv1 and conv2, the chain conv(first + 1)..conv7, every other kind one layer
enum PilotLaunchKind { kLaunchHeadWhole, kLaunchHeadSplit, kLaunchU8, kLaunchSpan1, kLaunchSpan2, kLaunchLt1, kLaunchLt2, kLaunchFrame8, kLaunchFrame16, kLaunchFrame5,
                       kLaunchChain, kLaunchDense1, kLaunchDense2 };         // Frame8 / 16: granules per input pixel; Dense1 / 2: blocks of 32 frames per workgroup (NF)
inline const char* pilot_launch_name(PilotLaunchKind k)
{
    static const char* const names[] = {"band<whole>", "band<split>", "u8", "span<1>", "span<2>", "lt<1>", "lt<2>", "frame", "frame", "frame5", "chain", "dense", "dense"};
    return names[k];
}
constexpr int kBufFrames = -1;             // PilotLaunch::src: the caller's frames
struct PilotLaunch {
    PilotLaunchKind kind;
    int first, last;                       // the layers it computes, 0-based (7: dense1, 8: dense4)
    int src, dst;                          // kBufFrames, else the activation of that layer (act[]); dst 7 / 8: the fp32 slab of dense1 / dense4's K slices
    size_t in_bytes;                       // of src for this batch
    int grid_x, grid_y, block, lds, lds_max;   // lds_max: what the kernel is allowed (hipFuncAttributeMaxDynamicSharedMemorySize), lds: what this launch asks for
};
struct PilotPass {
    int err = TRS_OK; const char* err_text = nullptr;     // a refusal: nothing is launched
    int count = 0; PilotLaunch at[10];
    DenseCall dense{}; HeadCall head{};                    // what the batch adds to dense1 / dense4 and to the fused head (pilot_pass only)
    // What the activations the fused kernels keep in LDS are worth once the schedule has run.  act0_valid: act[0] holds conv1 of the last pass's frames
    // (after a pass: conv1 ran as its own layer; after a materialisation: that, or it was materialised).  chain_mid_valid: act[chain.first .. 5] hold
    // the last pass (after a pass: there is no chain; after a materialisation: that, or the interior was materialised).
    bool act0_valid = false, chain_mid_valid = false;
};
// bytes of buffer `buf` for n frames: the uint8 RGB frames, or an fp16 activation
inline size_t pilot_buffer_bytes(const PilotPlan& P, int buf, int n) { return buf == kBufFrames ? (size_t)n * P.H * P.W * 3 : (size_t)n * P.L[buf].act_elems() * 2; }

// conv(i + 1) launched by itself on n frames: one persistent workgroup per CU for the kernels that keep frames in LDS, grid (x, res_ysplit) for the others
inline PilotLaunch layer_launch(const PilotPlan& P, int i, int n)
{
    const PilotLayer& l = P.L[i];
    PilotLaunch a{};
    a.first = a.last = a.dst = i; a.src = i - 1; a.in_bytes = pilot_buffer_bytes(P, a.src, n); a.grid_y = 1;
    const PilotKernel k = pilot_kernel_of(l);
    if (k == kKernFrame5) { a.kind = kLaunchFrame5; a.grid_x = frame5_grid(l, n, P.cu_count); a.block = kFrame5Block; a.lds = l.frame5_lds; a.lds_max = kPilotLds; }
    else if (k == kKernFrame) { a.kind = l.CIN / 8 == 8 ? kLaunchFrame8 : kLaunchFrame16; a.grid_x = frame_grid(l, n, P.cu_count); a.block = kFrameBlock; a.lds = l.frame_lds; a.lds_max = kPilotLds; }
    else {
        a.kind = k == kKernU8 ? kLaunchU8 : k == kKernSpan1 ? kLaunchSpan1 : k == kKernSpan2 ? kLaunchSpan2 : k == kKernLt1 ? kLaunchLt1 : kLaunchLt2;
        a.grid_x = single_grid_x(l, n, P.cu_count); a.grid_y = l.res_ysplit; a.block = l.res_block; a.lds = a.lds_max = l.res_lds;
    }
    return a;
}
// a launch joins the schedule; a single layer's buffer-load bounds are 32-bit
inline bool pass_add(PilotPass& s, const PilotLaunch& a, const char* too_large)
{
    if (too_large && a.in_bytes >= 0x80000000ull) { s.err = TRS_ERR_LIMIT; s.err_text = too_large; return false; }   // an int holds 2^31 - 1 at most
    s.at[s.count++] = a;
    return true;
}
constexpr const char* kActTooLarge = "activation larger than 2 GiB: lower the batch";

// A forward pass of n frames: the fused head in place of conv1 and conv2 where it runs, the layers one by one up to the chain, the chain up to conv7, then
// dense1 (and dense4, which reads conv7's output as well).
inline PilotPass pilot_pass(const PilotPlan& P, int n)
{
    PilotPass s;
    int i = 0;
    if (pilot_head_runs(P)) {
        s.head = head_call(P, n);
        PilotLaunch a{};
        a.kind = P.head.wsplit > 1 ? kLaunchHeadSplit : kLaunchHeadWhole; a.first = 0; a.last = a.dst = 1; a.src = kBufFrames; a.in_bytes = pilot_buffer_bytes(P, kBufFrames, n);
        a.grid_x = s.head.grid; a.grid_y = 1; a.block = 1024; a.lds = a.lds_max = P.head.lds;
        if (!pass_add(s, a, "frames larger than 2 GiB: lower the batch")) return s;
        i = 2;
    }
    for (; i < 7 && i != P.chain.first; ++i)
        if (!pass_add(s, layer_launch(P, i, n), kActTooLarge)) return s;
    if (i < 7) {                                                            // conv(i + 1) .. conv7 in one launch, activations in LDS
        PilotLaunch a{};
        a.kind = kLaunchChain; a.first = i; a.last = a.dst = 6; a.src = i - 1; a.in_bytes = pilot_buffer_bytes(P, a.src, n);
        a.grid_x = chain_grid(P.chain, n); a.grid_y = 1; a.block = kChainBlock; a.lds = a.lds_max = P.chain.lds;
        pass_add(s, a, nullptr);
    }
    s.dense = dense_call(P.L[7], n, P.cu_count, P.tun);                      // dense4 has dense1's shape: one plan for both
    for (int j = 7; j < P.n_layers; ++j) {
        PilotLaunch a{};
        a.kind = s.dense.nf == 2 ? kLaunchDense2 : kLaunchDense1; a.first = a.last = a.dst = j; a.src = 6; a.in_bytes = pilot_buffer_bytes(P, 6, n);
        a.grid_x = s.dense.grid; a.grid_y = 1; a.block = 256; a.lds = a.lds_max = s.dense.lds;
        pass_add(s, a, nullptr);
    }
    s.act0_valid = !pilot_head_runs(P); s.chain_mid_valid = P.chain.first < 0;
    return s;
}
// What the fused kernels of the last pass (of n frames) kept in LDS, as far as layers lo..hi need it: conv1 behind the fused head (lo == 0), and the chain's
// interior layers — all of them, conv(chain.first + 1) .. conv6, as soon as lo..hi touches one.  The two flags say what is valid already.
inline PilotPass pilot_materialise(const PilotPlan& P, int n, int lo, int hi, bool act0_valid, bool chain_mid_valid)
{
    PilotPass s;
    s.act0_valid = act0_valid; s.chain_mid_valid = chain_mid_valid;
    if (lo == 0 && !act0_valid) {
        if (!pass_add(s, layer_launch(P, 0, n), kActTooLarge)) return s;
        s.act0_valid = true;
    }
    if (P.chain.first >= 0 && hi >= P.chain.first && lo < 6 && !chain_mid_valid) {
        for (int j = P.chain.first; j < 6; ++j)
            if (!pass_add(s, layer_launch(P, j, n), kActTooLarge)) return s;
        s.chain_mid_valid = true;
    }
    return s;
}

}  // namespace trsim
