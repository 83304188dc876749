// trsim_train_conv.hpp — the rules of training the pilot's last convolutions (include/trsim_spec.h, "training the pilot's last convolutions") that can be
// wrong without a GPU, as arithmetic a host compiler builds without HIP: the check of trs_pilot_train_convs' mask, where the eight trained arrays lie in the
// master, m, v and gradient buffers, the index of a kernel value in the packed binary16 copy the forward kernels read (pack_layer's order), the split of the
// weight gradient's (frame, pixel) reduction over workgroups, and the sizes of the session's buffers.
// trsim_train_conv.hip includes it; tests/train_conv_driver.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/trsim.h"

// a rule the kernels apply as well: nothing to a plain host compiler
#ifdef __HIPCC__
#define TRS_HOST_DEVICE __host__ __device__
#else
#define TRS_HOST_DEVICE
#endif

namespace trsim {

constexpr int kConvTrainLayers = 4;                  // conv4 .. conv7: bit j of the mask, layer j below, row 3 + j of the pilot's plan
constexpr int kConvTrainArrays = 8;                  // kernel and bias of each, in the order of trs_pilot_train_convs
constexpr uint32_t kConvMaskAll = 0xFu;
constexpr int kConvChunk = 64;                       // output pixels per LDS chunk of the weight-gradient kernel: four k-steps of 16

// conv(4 + j) over an input of ih x iw: 3 x 3, stride 1, valid
struct ConvGeom {
    int IH, IW, OH, OW, CIN, COUT;
    size_t kernel_count() const { return (size_t)9 * CIN * COUT; }
    long out_pixels(int n) const { return (long)n * OH * OW; }
    long in_pixels(int n) const { return (long)n * IH * IW; }
};
inline ConvGeom train_conv_geom(int j, int ih, int iw)
{
    constexpr int cin[4] = {64, 64, 64, 128}, cout[4] = {64, 64, 128, 128};
    return ConvGeom{ih, iw, ih - 2, iw - 2, cin[j], cout[j]};
}

// nullptr: fine; else the refusal's text.  arrays: h_conv_arrays[8] of trs_pilot_train_convs
inline const char* train_conv_mask_error(uint32_t mask, const float* const* arrays)
{
    if (mask == 0 || (mask & ~kConvMaskAll)) return "conv_mask must name at least one of conv4 .. conv7 (bits 0..3) and nothing else";
    if (!arrays) return "h_conv_arrays is NULL";
    for (int j = 0; j < kConvTrainLayers; ++j)
        if (((mask >> j) & 1u) && (!arrays[2 * j] || !arrays[2 * j + 1])) return "the kernel or the bias of a layer named in conv_mask is NULL";
    return nullptr;
}
// the lowest trained layer: back-propagation stops there
inline int train_conv_lowest(uint32_t mask) { int j = 0; while (j < kConvTrainLayers && !((mask >> j) & 1u)) ++j; return j; }

// Where array a (0..7: kernel [3][3][CIN][COUT] and bias [COUT] of conv4 .. conv7, Keras layouts) lies in the master, m, v and gradient buffers, in floats:
// one after the other, each exactly its Keras size, so a layer's bias follows its kernel.  A layer whose bit is clear keeps its room (zeros in m, v, the gradient).
struct ConvTrainLayout {
    size_t off[kConvTrainArrays + 1];
    size_t count(int a) const { return off[a + 1] - off[a]; }
    static ConvTrainLayout of()
    {
        ConvTrainLayout t{};
        size_t o = 0;
        for (int j = 0; j < kConvTrainLayers; ++j) {
            const ConvGeom g = train_conv_geom(j, 3, 3);
            t.off[2 * j] = o; o += g.kernel_count();
            t.off[2 * j + 1] = o; o += (size_t)g.COUT;
        }
        t.off[kConvTrainArrays] = o;
        return t;
    }
};

// K[kh][kw][ci][co] in ConvLayer::w, in binary16 values: granule (kh run_pad + kw CIN / 8 + ci / 8) of output channel co, value ci % 8 of it (pack_layer;
// run_pad == run == 3 CIN / 8 and COUT_PAD == COUT for these layers)
TRS_HOST_DEVICE inline size_t train_conv_packed_index(const ConvGeom& g, int kh, int kw, int ci, int co)
{
    const int run_pad = 3 * g.CIN / 8;
    return ((size_t)(kh * run_pad + kw * (g.CIN / 8) + ci / 8) * g.COUT + co) * 8 + ci % 8;
}
// the same for value number e of the Keras kernel [3][3][CIN][COUT]: how the kernels that keep both copies go from one to the other
TRS_HOST_DEVICE inline size_t train_conv_packed_index(int CIN, int COUT, int e)
{
    const int co = e % COUT, t = e / COUT, ci = t % CIN, tap = t / CIN, kh = tap / 3, kw = tap - 3 * kh;
    return train_conv_packed_index(ConvGeom{0, 0, 0, 0, CIN, COUT}, kh, kw, ci, co);
}

// The weight gradient reduces over the P = n OH OW output pixels in (frame, row, column) order.  They are cut into chunks of 64; slice s of `slices` takes
// chunks s per_slice .. and a workgroup per (slice, tap) adds its chunks in order; the slices' partial sums are added in slice order afterwards.  The number
// of slices depends on (P, CU count) alone: about two workgroups per CU over the nine taps, at most one slice per chunk.
struct ConvSplit {
    long P; int chunks, per_slice, slices;
    long first(int s) const { return (long)s * per_slice * kConvChunk; }
    long end(int s) const { return std::min(P, (long)(s + 1) * per_slice * kConvChunk); }
};
inline ConvSplit train_conv_split(const ConvGeom& g, int n, int cu_count)
{
    ConvSplit s{};
    s.P = g.out_pixels(n);
    s.chunks = (int)((s.P + kConvChunk - 1) / kConvChunk);
    const int want = std::max(1, std::min(s.chunks, (2 * std::max(1, cu_count) + 8) / 9));
    s.per_slice = (s.chunks + want - 1) / want;
    s.slices = (s.chunks + s.per_slice - 1) / s.per_slice;
    return s;
}

// The most slices any batch of n <= n_cap frames can have.  slices(n) does not grow steadily with n (n = 1000 of 120x160 frames cuts conv7's 563 chunks into
// 57 slices of 10, n = 1024 its 576 chunks into 53 of 11), so a buffer is never sized from the split at n_cap: slices = ceil(chunks / per_slice) with
// per_slice = ceil(chunks / want) is at most want, which is at most (2 CUs + 8) / 9 and at most chunks(n) <= chunks(n_cap).
inline int train_conv_max_slices(const ConvGeom& g, int n_cap, int cu_count)
{
    const long chunks_cap = (g.out_pixels(n_cap) + kConvChunk - 1) / kConvChunk;
    return (int)std::max(1L, std::min(chunks_cap, (long)((2 * std::max(1, cu_count) + 8) / 9)));
}

// the session's buffers for frames whose x3 is ih3 x iw3, n_cap of them at most, down to layer `lowest`
struct ConvTrainSizes {
    size_t grad_floats;                     // G(l) in binary32, one buffer for every layer in turn: the largest of n_cap OH OW COUT
    size_t q_halfs[kConvTrainLayers];       // delta(l) in binary16 (0 below the lowest trained layer)
    size_t part_floats;                     // the weight gradient's partial sums [slices][3][3][CIN][COUT] and the bias's [slices][COUT]: the largest trained
                                            // layer at the most slices any n <= n_cap can have (train_conv_max_slices)
};
inline ConvTrainSizes train_conv_sizes(int ih3, int iw3, int n_cap, int cu_count, int lowest)
{
    ConvTrainSizes z{};
    int ih = ih3, iw = iw3;
    for (int j = 0; j < kConvTrainLayers; ++j) {
        const ConvGeom g = train_conv_geom(j, ih, iw);
        if (j >= lowest) {
            const size_t out = (size_t)g.out_pixels(n_cap) * g.COUT;
            z.q_halfs[j] = out;
            z.grad_floats = std::max(z.grad_floats, out);
            z.part_floats = std::max(z.part_floats, (size_t)train_conv_max_slices(g, n_cap, cu_count) * (g.kernel_count() + g.COUT));
        }
        ih = g.OH; iw = g.OW;
    }
    return z;
}

// what trs_pilot_train_debug_conv hands out (include/trsim.h, TRS_CONV_DBG_*): the floats of item `which` of layer j after a step of n frames, 0: unknown
inline size_t train_conv_debug_floats(const ConvGeom& g, int which, int n)
{
    switch (which) {
    case TRS_CONV_DBG_DELTA: return (size_t)g.out_pixels(n) * g.COUT;
    case TRS_CONV_DBG_GW: case TRS_CONV_DBG_MW: case TRS_CONV_DBG_VW: case TRS_CONV_DBG_PACK: return g.kernel_count();
    case TRS_CONV_DBG_GB: case TRS_CONV_DBG_MB: case TRS_CONV_DBG_VB: return (size_t)g.COUT;
    case TRS_CONV_DBG_SCALE_EXP: return 1;
    default: return 0;
    }
}

}  // namespace trsim
