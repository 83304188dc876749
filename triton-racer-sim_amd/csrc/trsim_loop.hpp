// trsim_loop.hpp — the tick loop of the closed loops (trs_step_pilot, trs_step_expert, trs_step_dagger): the ONE place where the order of a tick is
// written down.  Host-only and free of HIP headers, like trsim_post.hpp and trsim_pilot_plan.hpp: tests/loop_driver.cpp runs closed_loop over scripted ops
// with a plain host compiler under AddressSanitizer + UBSan, error paths included (on the device a failed tick cannot be provoked).
//   expert_capture_error   why a capture is refused (nullptr: accepted)
//   CapturePlan            which ticks of a call are captured, and into which slot
//   closed_loop            n_steps ticks over the ops of one entry point
#pragma once
#include <cstdint>

#include "../../include/trsim.h"

namespace trsim {

// why trs_step_expert and trs_step_dagger refuse this capture on a handle with (render != 0) or without a camera (nullptr: they do not)
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

// The capture plan of ONE call of a closed loop; closed_loop owns it.  slot_for(k, frame_ready) is asked once per tick, in tick order, with the driver's
// counter k and whether the frame of the tick exists (or no frame is wanted): it returns the slot the tick is captured into and takes it, or -1.
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

// n_steps ticks of a closed loop.  cap: the call's capture or nullptr; k: the driver's tick counter, carried by the caller from call to call (nullptr:
// the loop has no driver and captures nothing); n_captured: where the slots used so far are reported, or nullptr.  Ops has
//   int observe(const uint8_t** frame)             refresh the handle's view, run what acts before the label, *frame = the frame of this tick's record (nullptr: none yet)
//   int label(int slot)                            launch what writes the applied controls, and the row of `slot` when slot >= 0
//   int keep_frame(int slot, const uint8_t* frame)  copy the frame into `slot`, in front of the step (the handle recycles the buffer two steps on)
//   int step()                                     one env step on the applied controls
// each returning TRS_OK or the code the call ends with: nothing further is issued then, and k and *n_captured stay where the tick had brought them.
template <class Ops>
int closed_loop(Ops& ops, int n_steps, const trs_expert_capture* cap, uint32_t* k, int* n_captured)
{
    CapturePlan plan = CapturePlan::of(cap);
    const bool wants_frames = cap && cap->d_frames_or_null;
    if (n_captured) *n_captured = 0;
    for (int t = 0; t < n_steps; ++t) {
        const uint8_t* frame = nullptr;
        if (int rc = ops.observe(&frame)) return rc;
        const int slot = cap && k ? plan.slot_for(*k, !wants_frames || frame != nullptr) : -1;
        if (int rc = ops.label(slot)) return rc;
        if (k) ++*k;                                         // the driver's state has moved: the counter moves with it
        if (slot >= 0 && wants_frames)
            if (int rc = ops.keep_frame(slot, frame)) return rc;
        if (n_captured) *n_captured = plan.used;
        if (int rc = ops.step()) return rc;
    }
    return TRS_OK;
}

}  // namespace trsim
