// trsim_train.hpp — the rules of training the pilot's tail (include/trsim_spec.h, "training the pilot's tail") that can be wrong without a GPU, as arithmetic a
// host compiler builds without HIP: the defaults and refusals of trs_train_config, Adam's step size alpha_t, the exponent of the per-batch power-of-two scale
// as a function of a bit pattern, and where each of the eight trained arrays lies in the master, m, v and gradient buffers (all four share one layout) — and the
// same for the 14 arrays of a 28-array session (TrainSideLayout, the count and mask rules of trs_pilot_train_begin_ex).
// trsim_train.hip includes it; tests/train_driver.cpp and tests/train_side_driver.cpp run it on the CPU.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/trsim.h"

namespace trsim {

// the eight trained arrays in the order of trs_pilot_train_begin / _get: kernel and bias of dense1, dense2, dense3, output_layer
constexpr int kTrainArrays = 8;
constexpr int kTailIn[4] = {0, 100, 50, 25}, kTailOut[4] = {100, 50, 25, 2};   // kTailIn[0] is F, the flatten's length: TrainLayout::of fills it in
constexpr uint32_t kTrainMaskAll = 0xFu;                                       // bit l: layer l of dense1, dense2, dense3, output_layer is trained
// floats per frame of what a step keeps of its passes, TRS_TRAIN_DBG_OUT .. DELTA4 in order: out, z1 .. z3, delta1 .. delta4
constexpr int kTrainFrameItems = 8;
constexpr int kTrainFrameWidth[kTrainFrameItems] = {2, 100, 50, 25, 100, 50, 25, 2};
// the floats of items 0 .. upto - 1 together: where item `upto` begins in a frame's worth, and with all eight the whole of it
constexpr size_t train_frame_floats(int upto = kTrainFrameItems)
{
    size_t o = 0;
    for (int j = 0; j < upto; ++j) o += (size_t)kTrainFrameWidth[j];
    return o;
}

inline void train_defaults(trs_train_config* c)
{
    std::memset(c, 0, sizeof *c);
    c->struct_size = (uint32_t)sizeof *c;
    c->lr = 1e-3f; c->beta1 = 0.9f; c->beta2 = 0.999f; c->eps = 1e-7f;         // optimizers.Adam(lr=0.001) and Keras's defaults
    c->train_mask = kTrainMaskAll;
}

// nullptr: fine; else the refusal's text (a NaN is outside every range)
inline const char* train_config_error(const trs_train_config* c)
{
    if (!c) return "trs_train_config is NULL";
    if (c->struct_size != sizeof(trs_train_config)) return "trs_train_config.struct_size does not match this library (start from trs_default_train_config)";
    if (!(c->lr > 0.0f) || !std::isfinite(c->lr)) return "trs_train_config.lr must be positive and finite";
    if (!(c->beta1 >= 0.0f && c->beta1 < 1.0f)) return "trs_train_config.beta1 must lie in [0, 1)";
    if (!(c->beta2 >= 0.0f && c->beta2 < 1.0f)) return "trs_train_config.beta2 must lie in [0, 1)";
    if (!(c->eps > 0.0f) || !std::isfinite(c->eps)) return "trs_train_config.eps must be positive and finite";
    if (c->train_mask == 0 || (c->train_mask & ~kTrainMaskAll)) return "trs_train_config.train_mask must name at least one of the four layers (bits 0..3) and nothing else";
    return nullptr;
}

// ---- the session of a 28-array pilot, cnn_2d_speed_as_feature (include/trsim_spec.h, "training the pilot's tail, side branch") ----
// Its 14 trained arrays are arrays 14 .. 27 of trs_pilot_load's list: 0 .. 7 as above, but dense1's kernel, array 0, has (F + 16) x 100 values (rows F .. F + 15
// multiply feature3's output: W1Y); 8 .. 13 are kernel and bias of feature1 (1 -> 4), feature2 (4 -> 8), feature3 (8 -> 16).  Bits 4 .. 6 of the train mask
// name feature1 .. feature3; W1Y moves with dense1, bit 0.
constexpr int kTrainSideArrays = 14;
constexpr int kSideIn[3] = {1, 4, 8}, kSideOut[3] = {4, 8, 16};
constexpr int kSideRows = 16;                                                  // rows of dense1's kernel behind the flatten
constexpr uint32_t kTrainMaskSide = 0x70u, kTrainMaskAllSide = kTrainMaskAll | kTrainMaskSide;
// what a step keeps per frame of the branch, TRS_TRAIN_SIDE_FIN .. DY3 in order: fin, y1 .. y3, delta-y1 .. delta-y3; then the products fin delta-y1, the terms of
// feature1's kernel gradient (no debug item)
constexpr int kSideFrameItems = 8;
constexpr int kSideFrameWidth[kSideFrameItems] = {1, 4, 8, 16, 4, 8, 16, 4};
constexpr size_t side_frame_floats(int upto = kSideFrameItems)
{
    size_t o = 0;
    for (int j = 0; j < upto; ++j) o += (size_t)kSideFrameWidth[j];
    return o;
}
// the values trs_train_small_side_kernel and the side Adam own: W1Y, the three kernels, the three biases
constexpr int kSideValues = kSideRows * 100 + 4 + 32 + 128 + 4 + 8 + 16;

// the number of trained arrays of a pilot of n_pilot_arrays arrays (22, 28); 0: that pilot is not trained (42: both heads of cnn_2d_full_house feed conv7)
constexpr int train_arrays_of(int n_pilot_arrays) { return n_pilot_arrays == 22 ? kTrainArrays : (n_pilot_arrays == 28 ? kTrainSideArrays : 0); }
// nullptr: trs_pilot_train_begin_ex takes n_arrays for the loaded pilot; else the refusal's text, *limit set where the code is TRS_ERR_LIMIT
inline const char* train_count_error(int n_pilot_arrays, int n_arrays, bool* limit)
{
    *limit = false;
    if (n_pilot_arrays == 42) { *limit = true; return "the tail of a 42-array pilot (cnn_2d_full_house) is not trained: its two heads both feed conv7's gradient"; }
    if (n_arrays != kTrainArrays && n_arrays != kTrainSideArrays) return "n_arrays must be 8 (a 22-array pilot) or 14 (a 28-array pilot)";
    if (n_arrays != train_arrays_of(n_pilot_arrays)) return "n_arrays does not match the loaded pilot: 8 for a 22-array pilot, 14 for a 28-array one";
    return nullptr;
}
// the config of a session over n_arrays trained arrays: train_config_error, with bits 4 .. 6 allowed as well for 14
inline const char* train_config_error_ex(const trs_train_config* c, int n_arrays)
{
    if (!c || n_arrays != kTrainSideArrays || !(c->train_mask & kTrainMaskSide)) return train_config_error(c);
    if (c->train_mask & ~kTrainMaskAllSide) return "trs_train_config.train_mask must name layers of dense1 .. output_layer (bits 0..3) and feature1 .. feature3 (bits 4..6) and nothing else";
    trs_train_config tail = *c;
    tail.train_mask = kTrainMaskAll;                                           // (the mask is fine: the other fields by the one rule)
    return train_config_error(&tail);
}
// bit of the train mask that moves trained array a (0 .. 13): a / 2 for dense1 .. output_layer, 4 .. 6 for feature1 .. feature3
constexpr int train_mask_bit(int a) { return a >> 1; }

// alpha_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) in binary64 from the config's binary32 values, rounded once to binary32 (t >= 1)
inline float train_alpha(const trs_train_config& c, int64_t t)
{
    const double b1 = (double)c.beta1, b2 = (double)c.beta2;
    return (float)((double)c.lr * std::sqrt(1.0 - std::pow(b2, (double)t)) / (1.0 - std::pow(b1, (double)t)));
}
// 1 - beta in binary64, rounded once
inline float train_one_minus(float beta) { return (float)(1.0 - (double)beta); }

// The scale exponent s of a batch from the largest bit pattern of |delta1| (the integer maximum of the patterns is the maximum of the values):
// E = floor(log2(max)), s = 14 - E clamped to [-100, 100]; 0 for an all-zero batch.  A subnormal's E comes from its leading bit; Inf and NaN patterns give
// E = 128 like every exponent field of 255.
constexpr int train_scale_exponent(uint32_t max_abs_bits)
{
    const uint32_t a = max_abs_bits & 0x7FFFFFFFu;
    if (a == 0) return 0;
    int E = 0;
    if ((a >> 23) == 0) { int top = 22; while (!((a >> top) & 1u)) --top; E = top - 149; }
    else E = (int)(a >> 23) - 127;
    const int s = 14 - E;
    return s < -100 ? -100 : (s > 100 ? 100 : s);
}
// 2^e as a binary32 for |e| <= 126 (the scale and its inverse are exact)
inline float train_pow2(int e)
{
    const uint32_t bits = (uint32_t)(e + 127) << 23;
    float f; std::memcpy(&f, &bits, 4);
    return f;
}

// Where array a (0..7) lies in the master, m, v and gradient buffers, in floats: the arrays follow each other in order, each exactly its Keras size.
struct TrainLayout {
    size_t off[kTrainArrays + 1];        // off[8] = the total
    size_t count(int a) const { return off[a + 1] - off[a]; }
    static TrainLayout of(size_t F)
    {
        TrainLayout t{};
        size_t o = 0;
        for (int l = 0; l < 4; ++l) {
            const size_t in = l == 0 ? F : (size_t)kTailIn[l];
            t.off[2 * l] = o; o += in * (size_t)kTailOut[l];
            t.off[2 * l + 1] = o; o += (size_t)kTailOut[l];
        }
        t.off[kTrainArrays] = o;
        return t;
    }
};

// Where array a (0..13) of a 28-array session lies, in floats: the 22-array layout with array 0 grown by the 16 rows of W1Y, then feature1 .. feature3.  The
// first nine offsets are a TrainLayout (`tail`), which the kernels shared with the 22-array session take: gW1's GEMM and dense1's Adam cover rows 0 .. F - 1 of
// array 0, and W1Y, rows F .. F + 15, starts at w1y().
struct TrainSideLayout {
    size_t off[kTrainSideArrays + 1];    // off[14] = the total
    size_t F;
    size_t count(int a) const { return off[a + 1] - off[a]; }
    size_t w1y() const { return off[0] + F * 100; }
    TrainLayout tail() const
    {
        TrainLayout t{};
        for (int a = 0; a <= kTrainArrays; ++a) t.off[a] = off[a];
        return t;
    }
    static TrainSideLayout of(size_t F)
    {
        TrainSideLayout t{};
        t.F = F;
        const TrainLayout base = TrainLayout::of(F + (size_t)kSideRows);
        for (int a = 0; a <= kTrainArrays; ++a) t.off[a] = base.off[a];
        size_t o = base.off[kTrainArrays];
        for (int l = 0; l < 3; ++l) {
            t.off[kTrainArrays + 2 * l] = o; o += (size_t)kSideIn[l] * (size_t)kSideOut[l];
            t.off[kTrainArrays + 2 * l + 1] = o; o += (size_t)kSideOut[l];
        }
        t.off[kTrainSideArrays] = o;
        return t;
    }
};

// what trs_pilot_train_debug_side hands out (include/trsim.h, TRS_TRAIN_SIDE_*): the number of floats of item `which` after a step of n frames, 0 for an
// unknown item.  The seven side arrays in the order of the items: W1Y, then arrays 8 .. 13.
constexpr size_t kSideArrayCount[7] = {(size_t)kSideRows * 100, 4, 4, 32, 8, 128, 16};
inline size_t train_side_debug_floats(int which, int n)
{
    if (which >= TRS_TRAIN_SIDE_FIN && which <= TRS_TRAIN_SIDE_DY3) return (size_t)n * kSideFrameWidth[which];
    if (which >= TRS_TRAIN_SIDE_G && which < TRS_TRAIN_SIDE_G + 7) return kSideArrayCount[which - TRS_TRAIN_SIDE_G];
    if (which >= TRS_TRAIN_SIDE_M && which < TRS_TRAIN_SIDE_M + 7) return kSideArrayCount[which - TRS_TRAIN_SIDE_M];
    if (which >= TRS_TRAIN_SIDE_V && which < TRS_TRAIN_SIDE_V + 7) return kSideArrayCount[which - TRS_TRAIN_SIDE_V];
    return 0;
}

// what trs_pilot_train_debug hands out (include/trsim.h, TRS_TRAIN_DBG_*): the number of floats of item `which` after a step of n frames, 0 for an unknown item
inline size_t train_debug_floats(int which, int n, size_t F)
{
    const TrainLayout L = TrainLayout::of(F);
    if (which >= TRS_TRAIN_DBG_OUT && which <= TRS_TRAIN_DBG_DELTA4) return (size_t)n * kTrainFrameWidth[which];
    if (which >= TRS_TRAIN_DBG_GW1 && which <= TRS_TRAIN_DBG_GW4) return L.count(2 * (which - TRS_TRAIN_DBG_GW1));
    if (which >= TRS_TRAIN_DBG_GB1 && which <= TRS_TRAIN_DBG_GB4) return L.count(2 * (which - TRS_TRAIN_DBG_GB1) + 1);
    if (which >= TRS_TRAIN_DBG_M && which < TRS_TRAIN_DBG_M + kTrainArrays) return L.count(which - TRS_TRAIN_DBG_M);
    if (which >= TRS_TRAIN_DBG_V && which < TRS_TRAIN_DBG_V + kTrainArrays) return L.count(which - TRS_TRAIN_DBG_V);
    if (which == TRS_TRAIN_DBG_SCALE_EXP || which == TRS_TRAIN_DBG_LOSS) return 1;
    if (which == TRS_TRAIN_DBG_PACK1) return F * 100;
    if (which >= TRS_TRAIN_DBG_A1 && which <= TRS_TRAIN_DBG_A3) return (size_t)n * kTailIn[which - TRS_TRAIN_DBG_A1 + 1];   // what dense2, dense3, output_layer read
    return 0;
}

}  // namespace trsim
