// trsim_internal.hpp — what the translation units of libtrsim.so share besides the handle (trsim_env.hpp): the accessors trsim_hip.hip defines for the
// others, and the macros every unit exports and checks HIP calls with (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/trsim.h"
#include "trsim_loop.hpp"             // the tick loop the closed loops below are run through (host-only)

#define TRS_EXPORT extern "C" __attribute__((visibility("default")))

// a failed HIP call ends the entry point with TRS_ERR_DEVICE and "<call>: <hipGetErrorString>" as trs_last_error()
#define HIPCHK(call)                                                                                             \
    do {                                                                                                         \
        hipError_t _e = (call);                                                                                  \
        if (_e != hipSuccess) return trs_internal_fail(TRS_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

namespace trsim {
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
}

namespace trsim { struct Controls; }   // trsim_plan.hpp

struct TrsEnvView {
    int device, n, H, W, render;
    hipStream_t stream;
    const uint8_t* latest_frame;      // uint8[n][H][W][3] of the last completed step, or nullptr
    const float* speed;               // 'gym/speed'
    const int32_t* seg_idx; int n_points;   // LocationTracker index and track length ('loc/segment' = idx / n_points * 10)
    float *ctl_steer, *ctl_thr, *ctl_brk;   // the handle's own control staging arrays (device)
    uint64_t step_count;
    unsigned long long* stats;        // TRS_F_STATS (device, uint64[64])
    // an observation latency is set (trs_set_latency): what the cars are told after the last step (nullptr before the first step of the history) —
    // trs_step_pilot reads these instead of latest_frame / speed / seg_idx, and masks the cars whose first observation has not arrived
    bool obs_on;
    const uint8_t* obs_frame; const float* obs_speed; const int32_t* obs_seg_idx;
    const uint8_t* obs_mode;          // uint8[n]: TRS_MODE_AI where the env's observation has arrived, else TRS_MODE_HUMAN
    int codec_quality;                // trs_set_camera_codec: trs_step_pilot feeds the pilot codec(frame) of the frame it reads (0: the frame itself)
};

bool trs_internal_view(trs_env* e, TrsEnvView* out);
void** trs_internal_pilot_slot(trs_env* e);
void** trs_internal_expert_slot(trs_env* e);   // the scripted expert's context (trsim_expert.hip), nullptr while none is set
const trs_pilot_tuning* trs_internal_pilot_tuning(trs_env* e);   // what trs_pilot_set_tuning stored, or nullptr (defaults)
void trs_internal_set_pilot_tuning(trs_env* e, const trs_pilot_tuning* t);
int trs_internal_fail(int code, const std::string& msg);
const uint8_t* trs_internal_latest_frame(const trs_env* e);   // what a NULL frame source means to trs_normalize, trs_preprocess and trs_encode_jpeg (nullptr: no camera)
int trs_internal_camera_codec(trs_env* e, const uint8_t* d_frames, const uint8_t** d_out);   // codec(n_envs frames, the quality that is set) into the handle's codec buffer, on the stream (trsim_jpeg_codec.hip)
int trs_internal_step_launch(trs_env* e, const float* d_st, const float* d_th, const float* d_br);   // one env step by launch, whatever the step mode
// one env step with index `step` by launch, on the handle's stream, WITHOUT moving the step counter: a step that was posted to a resident worker
// (the counter moved at the post) and has to run as a launch after all (trsim_resident.hip, fall_back_to_launches)
int trs_internal_replay_launch(trs_env* e, const trsim::Controls& c, uint64_t step);   // (c: the post's own pointers, held: stride 0)
void trs_internal_note(const std::string& msg);            // what trs_last_error() returns, without failing the call
void trs_internal_count(trs_env* e, uint64_t d2h_bytes, uint64_t h2d_bytes);   // trs_counters bookkeeping for copies made outside trsim_hip.hip
void trs_pilot_free(void* ctx);       // defined in trsim_pilot.hip, called by trs_destroy
// ---- the closed loops: trs_step_pilot (trsim_pilot.hip), trs_step_expert and trs_step_dagger (trsim_expert.hip) ----
// Each is its argument checks and a small ops object handed to trsim::closed_loop (trsim_loop.hpp), where the order of a tick is written down.
// The view of one tick: trs_internal_view, which asks a resident worker to leave the handle's stream; at most once per tick.
inline int trs_internal_tick_view(trs_env* e, TrsEnvView* v)
{
    return trs_internal_view(e, v) ? TRS_OK : trs_internal_fail(TRS_ERR_DEVICE, "the handle's stream could not be taken over from the resident worker");
}
// what the ops of every loop share: the handle, the call's capture (or nullptr), the view of the current tick (observe refreshes it) and the two ops that
// do not depend on who drives
struct TrsLoopOps {
    trs_env* e; const trs_expert_capture* cap; TrsEnvView v;
    int keep_frame(int slot, const uint8_t* frame);         // device to device into the capture's slot, on the view's stream (trsim_hip.hip: the size is the handle's)
    int step() { return trs_internal_step_launch(e, v.ctl_steer, v.ctl_thr, v.ctl_brk); }
};
// The pilot's part, defined in trsim_pilot.hip, that trs_step_dagger shares with trs_step_pilot.
// trs_internal_pilot_loop_check: what the closed loop refuses before its first tick (no pilot, cfg, n_steps, model type, no camera); TRS_OK or the failed code.
// trs_internal_pilot_tick: the `observe` of both loops.  Refreshes *v (trs_internal_tick_view), chooses the frame the pilot reads today (the latest one; the
// delayed one under an observation latency, with that observation's speed, segment and mode mask), puts it through the camera codec when one is set, and runs
// the pilot into the handle's control arrays (v->ctl_*) — or writes zero controls when no frame exists yet.  *fed: the frame that was fed (nullptr: none).
int trs_internal_pilot_loop_check(trs_env* e, const trs_pilot_config* cfg, int n_steps);
int trs_internal_pilot_tick(trs_env* e, const trs_pilot_config* cfg, TrsEnvView* v, const uint8_t** fed);
// ---- training the pilot's tail (trsim_train.hip; the session itself is the training units' own: trsim_train_session.hpp) ----
// The loaded pilot behind conv7 as a training step sees it: device pointers into the pilot's own buffers (views), defined in trsim_pilot.hip.
struct TrsPilotTail {
    int arch, n_cap, G; size_t F;         // TRS_PILOT_*, the plan's capacity, dense1's granules and the flatten's length F = 8 G
    const void* x7;                       // conv7's activation of the last pass: binary16 [n][F]
    const float* slab; int slices; size_t slab_stride;   // dense1's split-K slabs of the last pass: `slices` of [n][100], slab_stride floats apart
    unsigned short* w1_pack; float* b1;   // dense1 as trs_pilot_dense_kernel reads it: granules [G][128][8] of binary16, bias [128]
    float *w2, *b2, *w3, *b3, *w4, *b4;   // the small layers where the tail kernel reads them (Keras layouts)
    // a 28-array pilot: where trs_pilot_tail_ex_kernel reads dense1's rows behind the flatten (W1Y [16][100]) and kernel and bias of feature1 .. feature3, in
    // that order (slots XO_W1Y, XO_F1W .. XO_F3B of the tail's blob, which holds w2 .. b4 as well); nullptr each for a 22-array pilot
    float* side[7];
    void** train;                        // the session's slot in the pilot's context (nullptr in it: none open)
};
int trs_internal_pilot_tail(trs_env* e, TrsEnvView* v, TrsPilotTail* t);   // the view and the tail of the loaded pilot, or the refusal of every pilot entry point (no handle, no pilot)
// What a training step may put between the two halves of that pass: fn(arg, x7, n) runs after conv7 has been launched and before dense1 is, and launches
// on the view's stream whatever rewrites conv7's activation in place (dropout at site 0); a non-zero return ends the pass with that code.
struct TrsPilotX7Hook { int (*fn)(void* arg, void* x7, int n); void* arg; };
int trs_internal_pilot_dense_forward(trs_env* e, const TrsEnvView& v, const uint8_t* d_frames, int n, TrsPilotTail* t, const TrsPilotX7Hook* between = nullptr);   // conv1..7 and dense1 of trs_pilot_forward on the stream; *t refreshed
void trs_train_free(void* session);   // defined in trsim_train.hip, called by trs_pilot_free; nullptr is fine
// ---- training the pilot's last convolutions (trsim_train_conv.hip) ----
// conv4 .. conv7 of the loaded pilot as a training step sees them (views into the pilot's own buffers), defined in trsim_pilot.hip.  With `materialise`
// the interior activations x4 .. x6 of the last pass are written by the single-layer kernels where the chain kept them in LDS (materialise_layers), on the stream.
struct TrsPilotConvs {
    int n_cap, cu_count;
    struct Layer {
        int IH, IW, OH, OW, CIN, COUT, COUT_PAD, run_pad;
        const void* in; const void* out;      // x(l-1) and x(l) of the last pass: binary16 [n][H][W][C]
        unsigned short* w; float* bias;       // ConvLayer::w (granules, pack_layer's order) and ConvLayer::bias [COUT_PAD]
    } L[4];
};
int trs_internal_pilot_convs(trs_env* e, const TrsEnvView& v, bool materialise, TrsPilotConvs* out);
void trs_expert_free(void* ctx);      // defined in trsim_expert.hip, called by trs_destroy and by trs_load_track (a new track switches the expert off); nullptr is fine
