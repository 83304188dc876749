// trsim_latency.hpp — the handle's observation latency (trs_set_latency; include/trsim_spec.h, "observation latency") as ONE member of trs_env.  Host only.
// trs_set_latency builds an ObsHistory beside the handle and move-assigns it; off is the assignment of an empty one: the buffers of the old setting go with
// the value they belong to (the caller has idled the stream).  The slot arithmetic is ObsRing's, the byte arithmetic obs_bytes' (trsim_plan.hpp); the kernel
// and the entry points are in trsim_latency.hip.
#pragma once
#include <cstdint>
#include <vector>

#include "trsim_mem.hpp"
#include "trsim_plan.hpp"

namespace trsim {
// While on() every step renders into a slot of ring_img / ring_dep, trs_obs_kernel files its telemetry in ring_tel and gathers every env's delayed record;
// the handle's img[] / depth[] then hold the gathered frames (envs with different delays) or lie idle (one delay for all: the view points into the ring).
struct ObsHistory {
    ObsRing ring;                                            // slot arithmetic; max_ticks == 0: off
    uint64_t base = 0;                                       // step_count when the history began: T = step_count - base
    bool uniform = true; int all = 0;                        // every env has the delay `all`
    DevBuf<int32_t> ticks; std::vector<int32_t> host;        // int32[n]: L_e, device and host
    DevBuf<uint8_t> ring_img; size_t img_stride = 0;         // [slots] frames of all envs, stride bytes apart (a multiple of 256)
    DevBuf<float> ring_dep; size_t dep_stride = 0;           // [slots] depth frames (cfg.depth), stride bytes apart
    DevBuf<float> ring_tel;                                  // [slots][6][n]: x y z speed cte | seg_idx (int32)
    DevBuf<float> tel[2];                                    // [6][n] the gathered telemetry, by T & 1
    DevBuf<uint8_t> flag[2];                                 // arrived[n] | mode[n] (TRS_MODE_AI where arrived, else TRS_MODE_HUMAN: the pilot tail's mask), by T & 1

    bool on() const { return ring.on(); }
    long long steps(uint64_t step_count) const { return (long long)(step_count - base); }   // T of "observation latency": steps since the history began
    int slot_of_last(uint64_t step_count) const { return ring.slot_of_step(steps(step_count)); }   // where the step that was counted last rendered
    uint8_t* frame(int slot) const { return ring_img.get() + (size_t)slot * img_stride; }
    float* depth(int slot) const { return reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(ring_dep.get()) + (size_t)slot * dep_stride); }
};
}  // namespace trsim
