// trsim_env.hpp — the handle behind `trs_env*` (include/trsim.h), shared by the translation units of libtrsim.so.
// Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trsim.h"
#include "trsim_device.hpp"
#include "trsim_latency.hpp"
#include "trsim_mem.hpp"
#include "trsim_tables.hpp"

namespace trsim {
struct Resident; struct Comm;
// What trs_load_track and trs_set_camera stage beside the handle, check, and then move-assign into it (trsim_scene.hip): the struct a feature is staged in is the
// member the handle holds, so a commit is one assignment and "none" is the assignment of {}.  The old value's buffers are released by the assignment.
struct TrackStage {                      // the device buffers of a track
    DevBuf<> blob_p, blob_r;             // physics LDS image | raster LDS image (+ the constants of a track with elevation and of the lens camera behind it)
    DevBuf<float> tangent, start_yaw;
    DevBuf<float> dpitch;                // [n_points] view pitch per raw track point (device: (float)pitch + dpitch[i])
};
struct LensStage {                       // the lens tables of a map for a camera
    DevBuf<> dev; size_t pal_off = 0;    // device: half-width planes F | L | D | M, then the lens palette at byte pal_off (LensBlock points into it)
    LensTables T;                        // host tables of the map (full frame), built by build_lens_tables
};
}  // namespace trsim

struct trs_env {
    trs_config cfg{};
    int device = 0, n = 0, H = 0, W = 0, cu_count = 0;
    hipStream_t sP = nullptr;            // the handle's stream: every launch, copy and timing event
    hipEvent_t ev[8] = {};
    // Memory the library allocates is held by DevBuf / PinnedBuf members (trsim_mem.hpp) and goes with the handle; raw pointers below are views.
    trsim::DevBuf<> slab;                // state + controls
    trsim::DevBuf<uint8_t> img[2];
    trsim::UniformRows uniform_ok;       // which frame buffer holds the present palette's uniform rows (sky, beyond the far plane) of every env: every step path asks it (trsim_plan.hpp)
    trsim::DevBuf<float> depth[2];
    trsim::TrackStage trk;               // the loaded track's device buffers (track_commit)
    trsim::DevBuf<float4> cam;           // [kRing][n]
    trsim::DevBuf<float> cam_pitch;      // [kRing][n] the frames' view pitches (tracks with elevation)
    trsim::Scene scene;                       // what is rendered besides the track's geometry: the features set, the frame filter, the camera (trsim_scene.hpp)
    trsim::LensStage lens;                    // the lens camera's tables for the loaded map, as lens_stage built them ({}: the pinhole, or no track yet)
    const float* light = nullptr;             // view: scene lighting's registered float[n][8], the caller's or light_own's (nullptr unless scene.light_on)
    trsim::DevBuf<float> light_own;           // trs_set_lighting_host's copy
    trsim::ObsHistory obs;                    // observation latency (trs_set_latency; trsim_latency.hpp): while obs.on() every step renders into its ring and trs_obs_kernel runs behind it
    trsim::DevBuf<unsigned long long> stats;
    trsim::DevBuf<double> loc_q; trsim::DevBuf<int32_t> loc_out; int loc_cap = 0;   // trs_locate: room for loc_cap queries
    trsim::DevBuf<uint8_t> pre;          // processed frames of the env (trs_preprocess with d_dst == NULL)
    trsim::PinnedBuf<> pinned;           // trs_fetch_outputs staging
    trsim::DevBuf<int32_t> mux_state; int mux_tick = 0;   // ControlMultiplexer state per car (trs_control_mux)
    trsim::DevBuf<uint8_t> tmp_in, tmp_out; trsim::DevBuf<float> tmp_f; size_t tmp_cap = 0;   // host-frame staging with room for tmp_cap frames
    trsim::DevBuf<int> hsv_tab;
    trsim::DevBuf<unsigned> dyn_tab;    // FParams::tabs of the dynamic-brightness frame filter that is set (hsv reciprocals | in-range byte masks | sel)
    trsim::DevBuf<> edge_scratch;        // work arrays of the Canny layer for frames beyond LDS
    trsim::PParams pp{};
    trsim::RParams rp{};
    trsim::TrackTables tab;
    bool track_loaded = false;
    int lds_p = 0, lds_r = 0, pts_bytes = 0;
    uint64_t step_count = 0;
    float *ctl_steer = nullptr, *ctl_thr = nullptr, *ctl_brk = nullptr;   // views into slab, like the state arrays in pp
    uint8_t* ctl_reset = nullptr;
    size_t img_bytes = 0;
    int lds_step = 0, lds_off_phys = 0;
    trsim::DevBuf<float> seq_buf;        // device copy of host control sequences (trs_step_sequence_host)
    void* pilot = nullptr;               // trsim_pilot.hip context (cnn_2d_speed_control weights + activations), released by trs_pilot_free
    void* expert = nullptr;              // trsim_expert.hip context (the scripted expert of trs_set_expert: tables, disturbance state, tick counter), released by trs_expert_free
    trs_pilot_tuning pilot_tuning{}; bool has_pilot_tuning = false;   // trs_pilot_set_tuning: kernel choices of the next trs_pilot_load
    trsim::PinnedBuf<unsigned long long> fault;   // pinned host word the kernels set when they refuse to run (dynamic LDS not at offset 0)
    trsim::DevBuf<float> glue;           // device scratch of the *_host control glue (trs_driver_assist_host, trs_control_mux_host)
    trsim::DevBuf<void> scratch[32];     // trs_scratch
    // the tub image encoder (trs_encode_jpeg; include/trsim_spec.h, "tub image (JPEG)")
    trsim::DevBuf<> jpg_tab; int jpg_quality = 0;   // device copy of jpeg::Tables (trsim_jpeg_tables.hpp) for jpg_quality; 0: none yet
    trsim::DevBuf<uint8_t> jpg_slots, jpg_blob; trsim::DevBuf<int32_t> jpg_len; trsim::DevBuf<long long> jpg_off;   // trs_encode_jpeg_host: slots, lengths, packed files, offsets
    trsim::PinnedBuf<> jpg_pin;          // ... and the staging of its offsets and lengths
    // the tub image decoder (trs_decode_jpeg; include/trsim_spec.h, "tub image (JPEG), decoding")
    int jpd_lds_max = 0;                 // LDS a workgroup may take on the handle's device, queried at the first call; 0: not yet
    trsim::DevBuf<uint8_t> jpd_files, jpd_dst; trsim::DevBuf<> jpd_meta;   // trs_decode_jpeg_host: the files, the frames, offsets | lengths | statuses
    // the camera codec (trs_jpeg_roundtrip, trs_set_camera_codec; include/trsim_spec.h, "camera codec (JPEG round trip)")
    int codec_quality = 0;               // trs_set_camera_codec: trs_step_pilot feeds the pilot codec(frame, codec_quality); 0: off
    trsim::DevBuf<int32_t> jpc_steps; int jpc_quality = 0;   // device copy of jpeg::quant_steps (trsim_jpeg_tables.hpp) for jpc_quality; 0: none yet
    trsim::DevBuf<uint8_t> jpc_dst;      // the handle's codec buffer: n_envs frames (d_dst NULL, and the pre-pass of trs_step_pilot)
    trsim::DevBuf<uint8_t> jpc_in, jpc_out;   // trs_jpeg_roundtrip_host: the frames up and down
    uint64_t d2h_bytes = 0, h2d_bytes = 0;                  // trs_counters: what the library itself copied
    trsim::Comm* comm = nullptr;         // trsim_comm.hip: the RCCL communicator of trs_comm_init, nullptr = none
    hipEvent_t ev_order = nullptr;       // trs_stream_wait_external / trs_stream_signal_external
    trsim::Resident* res = nullptr;      // trsim_resident.hip: the resident worker (trs_set_step_mode), nullptr = never used
};

// ---- trsim_latency.hip (observation latency: the launch behind every step while one is set, and what the car is told) ----
namespace trsim {
int launch_obs(trs_env* e);                               // file the step that has just been counted in the ring and gather every env's delayed record
int latency_restart(trs_env* e);                          // the history begins here (trs_set_latency, trs_load_track); the handle's stream is idle
void obs_view(const trs_env* e, trs_obs_view* o);         // trs_get_observation's view (obs.on())
}  // namespace trsim

// ---- trsim_resident.hip (the resident worker: one step per trs_step call without a launch per step) ----
namespace trsim {
bool resident_on(const trs_env* e);                       // resident mode selected for this handle
bool resident_selected(const trs_env* e);                 // ... or selected and gone back to launches for now (the GPU is shared): it comes back by itself
void resident_retry(trs_env* e);                          // a handle that fell back to launches (GPU shared with another process) tries resident mode again when due
// hand n steps to the worker; c: the controls of the call (Controls, trsim_plan.hpp) as device pointers or host-pinned pointers the device can read;
// step k of the call is posted with c.after(k).  resident_post_host: c holds host arrays, held controls, staged per step in pinned memory.
// Both return TRS_OK, an error (< 0) or kResidentFellBack (> 0, not an error): the worker's launch was found not co-resident (another process's
// worker on the GPU), the handle is back in TRS_STEP_LAUNCH, the first *n_done steps of the call are on the stream as launches and the caller
// launches the rest itself.
constexpr int kResidentFellBack = 1;
int resident_post(trs_env* e, const Controls& c, int n, int* n_done);
int resident_post_host(trs_env* e, const Controls& h, int n_steps, int* n_done);
hipStream_t resident_copy_stream(trs_env* e);             // a stream that is not blocked by the worker (the handle's own when none runs)
int resident_wait(trs_env* e);                            // every posted step complete (the worker stays resident)
int resident_quiesce(trs_env* e);                         // ... and the worker has left the GPU: the stream is free again
void resident_note_launch(trs_env* e);                    // a step was launched on the stream while resident mode is selected (pilot loop)
void resident_destroy(trs_env* e);
int sync_handle(trs_env* e);                               // the handle's stream is idle (a resident worker is asked to leave first)
int quiesce_handle(trs_env* e);                            // a resident worker has left; queued work may still be running
void comm_destroy(trs_env* e);
bool resident_running(const trs_env* e);
void resident_clear_fault(trs_env* e);                     // trs_load_track puts every env on a defined state again
int check_fault(trs_env* e);                               // TRS_ERR_DEVICE (sticky) once a kernel has reported a layout fault
int ensure_hsv_table(trs_env* e);                          // e->hsv_tab holds OpenCV's reciprocal tables (hsv_reciprocals, trsim_filter.hpp); uploaded once (trsim_scene.hip)

// the instantiation of the step kernel and of the resident worker that the handle's state selects (Scene::variant, trsim_scene.hpp)
inline Variant variant_of(const trs_env* e) { return e->scene.variant(e->rp.depth != 0); }
// ... for the refusals by policy (variant_clash): a handle without a track has no HILLS bit, whatever a failed reload left behind
inline Variant variant_now(const trs_env* e) { return variant_of(e) & (e->track_loaded ? ~0u : ~kVHills); }
// The two LDS questions of every refusal, about the variant v the handle would run after the change beside lds_step bytes of tables (trsim_plan.hpp)
inline LdsFit handle_fit(const trs_env* e, Variant v, int lds_step) { return lds_fit(lds_step, e->pp.envs_per_wg, e->H, e->W, v, resident_on(e)); }
// the dynamic-brightness frame filter that is set, as the DYN instantiations take it (all zero without one); lds_off: its region in the kernel's LDS layout
inline FParams fparams_of(const trs_env* e, int lds_off) { return dyn_fparams(e->scene, e->H, e->dyn_tab.get(), lds_off); }
// trsim_hip.hip's part in trs_load_track (trsim_scene.hip): its kernels may use the LDS the new track needs, or the refusal that they cannot
int track_kernel_attributes(const trs_env* e, const TrackLayout& L, bool hills);
}  // namespace trsim
