// trsim_train.hpp — the rules of training the pilot's tail (include/trsim_spec.h, "training the pilot's tail") that can be wrong without a GPU, as arithmetic a
// host compiler builds without HIP: the defaults and refusals of trs_train_config, Adam's step size alpha_t, the exponent of the per-batch power-of-two scale
// as a function of a bit pattern, and where each of the eight trained arrays lies in the master, m, v and gradient buffers (all four share one layout).
// trsim_train.hip includes it; tests/train_driver.cpp runs it on the CPU.
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
