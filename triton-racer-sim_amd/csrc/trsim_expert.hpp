// trsim_expert.hpp — the host side of the scripted expert (include/trsim_spec.h, "scripted expert"): what trs_set_expert and trs_step_expert decide
// before anything reaches the device.  Host-only and free of HIP headers, like trsim_post.hpp and trsim_pilot_plan.hpp: tests/expert_driver.cpp compiles it
// with a plain host compiler under AddressSanitizer + UBSan.
//   expert_config_error / expert_capture_error   the refusals of the two calls (nullptr: accepted)
//   build_track_yaw                              track_yaw[p] = (float)atan2(tx[p], tz[p]) in binary64 from the binary32 tangents
//   CapturePlan                                  which ticks of a call are captured, and into which slot
//   kExpertRow*                                  the layout of a record row
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/trsim.h"
#include "../../include/trsim_spec.h"

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

// why trs_step_expert refuses this capture on a handle with (render != 0) or without a camera (nullptr: it does not)
inline const char* expert_capture_error(const trs_expert_capture* c, bool render)
{
    if (!c) return nullptr;                                  // no capture
    if (c->struct_size != sizeof(trs_expert_capture)) return "trs_expert_capture.struct_size mismatch";
    if (c->every < 1) return "trs_expert_capture.every < 1";
    if (c->skip < 0) return "trs_expert_capture.skip < 0";
    if (c->capacity < 0) return "trs_expert_capture.capacity < 0";
    if (c->capacity > 0 && !c->d_rows) return "trs_expert_capture.d_rows is NULL";
    if (c->d_frames_or_null && !render) return "frames asked of a handle without a camera (render == 0): only rows can be captured";
    return nullptr;
}

inline void build_track_yaw(const float* tangent /* [n][2] (tx, tz) */, int n_points, float* out)
{
    for (int p = 0; p < n_points; ++p) out[p] = (float)std::atan2((double)tangent[2 * p], (double)tangent[2 * p + 1]);
}

// The capture plan of ONE trs_step_expert call.  slot_for(k, frame_ready) is asked once per tick, in tick order, with the driver's counter k and whether
// the frame of the state exists (or no frame is wanted): it returns the slot the tick is captured into and takes it, or -1.
struct CapturePlan {
    int every = 1, skip = 0, capacity = 0, used = 0;
    static CapturePlan of(const trs_expert_capture* c)
    {
        CapturePlan p;
        if (c) { p.every = c->every; p.skip = c->skip; p.capacity = c->capacity; }
        return p;
    }
    bool due(uint32_t k) const { return k >= (uint32_t)skip && (k - (uint32_t)skip) % (uint32_t)every == 0; }
    int slot_for(uint32_t k, bool frame_ready)
    {
        if (used >= capacity || !due(k) || !frame_ready) return -1;
        return used++;
    }
};

}  // namespace trsim
