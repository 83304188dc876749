// trsim_expert.hpp — the host side of the scripted expert (include/trsim_spec.h, "scripted expert"): what trs_set_expert and trs_step_expert decide
// before anything reaches the device.  Host-only and free of HIP headers, like trsim_post.hpp and trsim_pilot_plan.hpp: tests/expert_driver.cpp compiles it
// with a plain host compiler under AddressSanitizer + UBSan.
//   expert_config_error                          the refusals of trs_set_expert (nullptr: accepted)
//   build_track_yaw                              track_yaw[p] = (float)atan2(tx[p], tz[p]) in binary64 from the binary32 tangents
//   expert_capture_error, CapturePlan            trsim_loop.hpp (included here): the capture's refusals, which ticks of a call are captured and into
//                                                which slot, and the tick loop that asks
//   kExpertRow*                                  the layout of a record row
// and of the pilot in the loop with the expert's labels (include/trsim_spec.h, "pilot in the loop with the expert's labels"; trs_step_dagger):
//   dagger_defaults / dagger_config_error        the defaults and the refusals of trs_dagger_config (nullptr: accepted)
//   splitmix64, unit24, dagger_gate              the keyed generator of the expert's disturbance and the gate it decides: under hipcc __host__ __device__,
//                                                so trs_expert_kernel, trs_dagger_kernel and tests/dagger_driver.cpp take them from this one place
//   kDaggerStat*                                 the layout of a stats row
#pragma once
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "../../include/trsim.h"
#include "../../include/trsim_spec.h"
#include "trsim_loop.hpp"

#if defined(__HIPCC__)
#define TRS_HD __host__ __device__
#else
#define TRS_HD
#endif

namespace trsim {

// a record row of trs_step_expert's capture: float[kExpertRowFloats]
constexpr int kExpertRowFloats = 8;
enum { kExpertRowSteer = 0, kExpertRowThr, kExpertRowBrk, kExpertRowApplied, kExpertRowSpeed, kExpertRowCte, kExpertRowSegment, kExpertRowDone };

inline void expert_defaults(trs_expert_config* c)
{
    c->struct_size = sizeof(trs_expert_config);
    c->look = TRS_EXPERT_LOOK;
    c->k_cte = TRS_EXPERT_K_CTE; c->k_head = TRS_EXPERT_K_HEAD;
    c->thr_hi = TRS_EXPERT_THR_HI; c->thr_lo = TRS_EXPERT_THR_LO;
    c->target_speed = TRS_EXPERT_TARGET_SPEED;
    c->brake_over = TRS_EXPERT_BRAKE_OVER; c->brake_val = TRS_EXPERT_BRAKE_VAL;
    c->alpha = TRS_EXPERT_ALPHA; c->sigma = TRS_EXPERT_SIGMA;
    c->seed = TRS_EXPERT_SEED;
}

// why trs_set_expert refuses this config on a track of n_points points (nullptr: it does not)
inline const char* expert_config_error(const trs_expert_config* c, int n_points)
{
    if (!c) return "null trs_expert_config";
    if (c->struct_size != sizeof(trs_expert_config)) return "trs_expert_config.struct_size mismatch";
    if (c->look < 0 || c->look >= n_points) return "trs_expert_config.look must lie in [0, n_points)";
    for (const float f : {c->k_cte, c->k_head, c->thr_hi, c->thr_lo, c->target_speed, c->brake_over, c->brake_val, c->alpha, c->sigma})
        if (!std::isfinite(f)) return "trs_expert_config: every field must be finite";
    return nullptr;
}

inline void build_track_yaw(const float* tangent /* [n][2] (tx, tz) */, int n_points, float* out)
{
    for (int p = 0; p < n_points; ++p) out[p] = (float)std::atan2((double)tangent[2 * p], (double)tangent[2 * p + 1]);
}

// ---- the keyed generator: SplitMix64 of (seed, key), as the synthetic control generator of include/trsim_spec.h states it ----
TRS_HD inline uint64_t splitmix64(uint64_t seed, uint64_t key)
{
    uint64_t z = seed + key * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
TRS_HD inline float unit24(uint64_t z) { return (float)(z >> 40) * 5.9604644775390625e-08f; }   // u = (float)(z >> 40) * 2^-24 in [0, 1 - 2^-24]
TRS_HD inline uint64_t env_key(uint32_t gid, uint32_t k) { return ((uint64_t)gid << 32) | (uint64_t)k; }

// ---- pilot in the loop with the expert's labels ----
// a stats row of trs_dagger_stats: float[kDaggerStatFloats]
constexpr int kDaggerStatFloats = 6;
enum { kDaggerStatTicks = 0, kDaggerStatExpertTicks, kDaggerStatSumAbsCte, kDaggerStatMaxAbsCte, kDaggerStatSumAbsDiff, kDaggerStatDone };

inline void dagger_defaults(trs_dagger_config* c)
{
    c->struct_size = sizeof(trs_dagger_config);
    c->beta = TRS_DAGGER_BETA; c->hold = TRS_DAGGER_HOLD; c->expert_speed = TRS_DAGGER_EXPERT_SPEED;
    c->seed = TRS_DAGGER_SEED;
}

// why trs_step_dagger refuses this config (nullptr: it does not)
inline const char* dagger_config_error(const trs_dagger_config* c)
{
    if (!c) return "null trs_dagger_config";
    if (c->struct_size != sizeof(trs_dagger_config)) return "trs_dagger_config.struct_size mismatch";
    if (!std::isfinite(c->beta) || c->beta < 0.0f || c->beta > 1.0f) return "trs_dagger_config.beta must be finite and lie in [0, 1]";
    if (c->hold < 1) return "trs_dagger_config.hold < 1";
    if (c->expert_speed != 0 && c->expert_speed != 1) return "trs_dagger_config.expert_speed must be 0 or 1";
    return nullptr;
}

// the gate of global env `gid` in the block of ticks `block` = k / hold: the expert drives iff u < beta
TRS_HD inline bool dagger_gate(uint64_t seed, uint32_t gid, uint32_t block, float beta) { return unit24(splitmix64(seed, env_key(gid, block))) < beta; }

}  // namespace trsim
