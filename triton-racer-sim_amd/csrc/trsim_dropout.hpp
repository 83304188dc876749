// trsim_dropout.hpp — the rules of training-mode dropout behind conv7 (include/trsim_spec.h, "training the pilot's tail, dropout") in the one place the
// kernels of trsim_train.hip, trs_pilot_train_dropout and trs_train_dropout_keep take them from: the defaults and refusals of trs_dropout_config, the
// threshold T and the scale s of a rate, the key chain (seed, step, site, frame) -> 64-bit word, and keep().  Free of HIP headers, like trsim_loader.hpp,
// whose mix it reuses: tests/dropout_driver.cpp compiles it with a plain host compiler under AddressSanitizer + UBSan; under hipcc the draws are
// __host__ __device__.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/trsim.h"
#include "trsim_loader.hpp"

namespace trsim {

constexpr int kDropoutSites = 4;                             // 0: conv7's output x7; 1 .. 3: relu(z1) .. relu(z3)
constexpr int kDropoutWidth[kDropoutSites] = {0, 100, 50, 25};   // units per frame (site 0: F, the flatten's length)
constexpr uint32_t kDropoutSitesAll = 0xFu;
constexpr uint64_t kDropoutSalt = 0x64726F706F757421ull;     // "dropout!"

inline void dropout_defaults(trs_dropout_config* c)
{
    std::memset(c, 0, sizeof *c);
    c->struct_size = (uint32_t)sizeof *c;
    c->rate = 0.1f;                                          // Dropout(0.1): components/keras_train.py:131-164
    c->sites = kDropoutSitesAll;
    c->seed = 0;
}

// nullptr: fine; else the refusal's text (a NaN is outside every range)
inline const char* dropout_config_error(const trs_dropout_config* c)
{
    if (!c) return "trs_dropout_config is NULL";
    if (c->struct_size != sizeof(trs_dropout_config)) return "trs_dropout_config.struct_size does not match this library (start from trs_default_dropout_config)";
    if (!(c->rate >= 0.0f && c->rate < 1.0f)) return "trs_dropout_config.rate must lie in [0, 1)";
    if (c->sites & ~kDropoutSitesAll) return "trs_dropout_config.sites names the four sites behind conv7 (bits 0..3) and nothing else";
    return nullptr;
}

// T = floor((double)rate 65536): a unit is dropped iff its 16-bit field is below T, so the effective rate is T / 65536 (rate in [0, 1): T <= 65535)
inline uint32_t dropout_threshold(float rate) { return (uint32_t)std::floor((double)rate * 65536.0); }
// s = (float)(65536 / (65536 - T)): the scale of the effective rate, one rounding
inline float dropout_scale(uint32_t T) { return (float)(65536.0 / (double)(65536u - T)); }

// the key chain: D = mix(seed ^ salt), Dt = mix(D ^ t) for the session's step t >= 1, key = mix(Dt ^ (site << 32 | i)) for frame slot i of the batch
TRS_HD inline uint64_t dropout_step_key(uint64_t seed, uint64_t t) { return mix(mix(seed ^ kDropoutSalt) ^ t); }
TRS_HD inline uint64_t dropout_frame_key(uint64_t Dt, uint32_t site, uint32_t i) { return mix(Dt ^ (((uint64_t)site << 32) | (uint64_t)i)); }
// units 4 w .. 4 w + 3 of a frame share word w = mix(key + w): sixteen bits each, unit 4 w lowest
TRS_HD inline uint64_t dropout_word(uint64_t key, uint32_t w) { return mix(key + (uint64_t)w); }
TRS_HD inline bool dropout_keep_field(uint64_t word, uint32_t k, uint32_t T) { return (uint32_t)((word >> (16u * (k & 3u))) & 0xFFFFu) >= T; }
TRS_HD inline bool dropout_keep(uint64_t key, uint32_t k, uint32_t T) { return dropout_keep_field(dropout_word(key, k >> 2), k, T); }

// what trs_train_dropout_keep refuses for an accepted config (nullptr: nothing)
inline const char* dropout_keep_error(int64_t t, int site, int n, int64_t width, const void* h_keep)
{
    if (t < 1) return "t counts the session's steps from 1";
    if (site < 0 || site >= kDropoutSites) return "site must be 0..3";
    if (n < 0 || width < 0 || width > 0xFFFFFFFFll) return "n or width out of range";
    if (!h_keep && n > 0 && width > 0) return "h_keep is NULL";
    return nullptr;
}

// the keep flags of step t at `site` for frame slots 0 .. n - 1 and units 0 .. width - 1: h_keep[i][k] = 1 kept, 0 dropped.  The site's bit of cfg.sites is
// not consulted: a site that is switched off applies no mask at all.
inline void dropout_keep_host(const trs_dropout_config& c, int64_t t, int site, int n, int64_t width, uint8_t* h_keep)
{
    const uint32_t T = dropout_threshold(c.rate);
    const uint64_t Dt = dropout_step_key(c.seed, (uint64_t)t);
    for (int i = 0; i < n; ++i) {
        const uint64_t key = dropout_frame_key(Dt, (uint32_t)site, (uint32_t)i);
        uint8_t* const row = h_keep + (size_t)i * (size_t)width;
        for (int64_t k0 = 0; k0 < width; k0 += 4) {
            const uint64_t word = dropout_word(key, (uint32_t)(k0 >> 2));
            for (int64_t k = k0; k < width && k < k0 + 4; ++k) row[k] = dropout_keep_field(word, (uint32_t)k, T) ? 1 : 0;
        }
    }
}

}  // namespace trsim
