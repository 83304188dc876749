// trsim_augment.hpp — the rules of the augmented training minibatches (include/trsim_spec.h, "training minibatches, augmentation") in the one place
// trs_batch_aug_kernel, trs_sample_batch_aug and trs_loader_augment take them from.  Free of HIP headers, like trsim_loader.hpp:
// tests/augment_driver.cpp compiles it with a plain host compiler under AddressSanitizer + UBSan; under hipcc the draw is __host__ __device__.
//   augment_defaults, augment_is_off          everything off; off = no mirror, no gain jitter, no bias jitter
//   augment_config_error                      the refusals (nullptr: accepted); the loader config decides the one about TRS_LOADER_FULL_HOUSE
//   AugKey::of(seed, epoch) / of(aug, epoch)  the key of one (config, epoch); .draw(rec): mirror flag and {gR gG gB 0 bR bG bB 0} of a record
// The pixel rule is light_channel (trsim_tables.hpp), not restated here.
#pragma once
#include <cstdint>

#include "trsim_loader.hpp"

namespace trsim {

constexpr uint64_t kAugmentSalt = 0x6175676D656E7421ull;
constexpr int kAugmentParams = 8;                            // the per-env layout of trs_set_lighting

inline void augment_defaults(trs_augment_config* a)
{
    a->struct_size = sizeof(trs_augment_config);
    a->mirror_prob = 0.0f; a->gain_amp = 0.0f; a->bias_amp = 0.0f;
    a->per_channel = 0;
    a->seed = 0;
}

inline bool augment_is_off(const trs_augment_config* a) { return !a || (a->mirror_prob == 0.0f && a->gain_amp == 0.0f && a->bias_amp == 0.0f); }

// why this augmentation is refused for an accepted loader config (nullptr: it is not).  Every comparison is written so that a NaN is refused.
inline const char* augment_config_error(const trs_augment_config* a, const trs_loader_config* c)
{
    if (!a) return "null trs_augment_config";
    if (a->struct_size != sizeof(trs_augment_config)) return "trs_augment_config.struct_size mismatch";
    if (!(a->mirror_prob >= 0.0f && a->mirror_prob <= 1.0f)) return "trs_augment_config.mirror_prob must lie in [0, 1]";
    if (!(a->gain_amp >= 0.0f && a->gain_amp < 1.0f)) return "trs_augment_config.gain_amp must lie in [0, 1): the gain stays positive";
    if (!(a->bias_amp >= 0.0f && a->bias_amp <= 255.0f)) return "trs_augment_config.bias_amp must lie in [0, 255]";
    if (a->per_channel != 0 && a->per_channel != 1) return "trs_augment_config.per_channel must be 0 or 1";
    if (a->mirror_prob > 0.0f && c->loader == TRS_LOADER_FULL_HOUSE)
        return "trs_augment_config.mirror_prob > 0 with TRS_LOADER_FULL_HOUSE: loc/segment is a position on the track as driven, a mirrored frame shows another track";
    return nullptr;
}

struct AugDraw {
    uint32_t mirror;                                         // 0 or 1
    float gb[kAugmentParams];                                // {gR gG gB 0 bR bG bB 0}
};

// one (config, epoch): the draw of record r is a function of (seed, epoch, r) alone — not of the batch slot, `first`, the batch size or the split
struct AugKey {
    uint64_t a_epoch;                                        // A ^ (epoch << 32): k(e, r) = mix(a_epoch ^ r), r < 2^32
    uint32_t threshold;                                      // T: mirrored when d_0 < T
    float gain_amp, bias_amp;
    int per_channel;
    TRS_HD static AugKey of(uint64_t seed, int epoch)        // the key alone: everything off
    {
        AugKey k;
        k.a_epoch = mix(seed ^ kAugmentSalt) ^ ((uint64_t)(uint32_t)epoch << 32);
        k.threshold = 0; k.gain_amp = 0.0f; k.bias_amp = 0.0f; k.per_channel = 0;
        return k;
    }
    TRS_HD static AugKey of(const trs_augment_config& a, int epoch)
    {
        AugKey k = of(a.seed, epoch);
        k.threshold = (uint32_t)((double)a.mirror_prob * 16777216.0);
        k.gain_amp = a.gain_amp; k.bias_amp = a.bias_amp; k.per_channel = a.per_channel;
        return k;
    }
    TRS_HD static float unit(uint64_t key, uint64_t j)       // f_j: 24 bits as a float in [-1, 1), exact
    {
        const float d = (float)(uint32_t)(mix(key + j) >> 40);
        const float s = d * 0x1p-23f;
        return s - 1.0f;
    }
    TRS_HD AugDraw draw(uint32_t rec) const
    {
        const uint64_t key = mix(a_epoch ^ (uint64_t)rec);
        AugDraw d;
        d.mirror = (uint32_t)(mix(key) >> 40) < threshold ? 1u : 0u;
        for (int c = 0; c < 3; ++c) {
            const uint64_t j = per_channel ? (uint64_t)c : 0u;
            const float tg = unit(key, 1 + j) * gain_amp;    // two roundings: the product, then the sum
            d.gb[c] = 1.0f + tg;
            d.gb[4 + c] = unit(key, 4 + j) * bias_amp;
        }
        d.gb[3] = 0.0f; d.gb[7] = 0.0f;
        return d;
    }
};

}  // namespace trsim
