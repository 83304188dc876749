/* trsim.h — C ABI of libtrsim.so, the MI355X-native batched env that replaces the
 * per-car simulator bridge of Triton-AI/Triton-Racer-Sim.
 *
 * Every entry point states the reference interface it stands in for.  Paths are
 * relative to /root/reference/TritonRacerSim/.  The reference is Python, so its
 * "FFI" for this path is ctypes: the binding a maintainer would add is shown in
 * INTEGRATION.md and shipped as triton-racer-sim_amd/_ffi.py.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success and a negative trs_status on error (never aborts, never throws);
 * trs_last_error() gives the message of the last failing call on this thread.
 * One handle = one GPU + one HIP stream; a handle is not re-entrant, different
 * handles are independent.  "d_" parameters are device pointers on the handle's
 * GPU, "h_" parameters are host pointers.
 *
 * The CPU oracle (oracle/libtrsim_oracle.so, test infrastructure only) exports
 * the same signatures with the prefix trso_ instead of trs_.
 */
#ifndef TRSIM_H
#define TRSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trs_env trs_env;

typedef enum trs_status {
    TRS_OK = 0,
    TRS_ERR_ARG = -1,      /* bad argument / bad config */
    TRS_ERR_STATE = -2,    /* call order (e.g. step before load_track) */
    TRS_ERR_DEVICE = -3,   /* no GPU, HIP error */
    TRS_ERR_NOMEM = -4,
    TRS_ERR_LIMIT = -5     /* track / image too large for the LDS-resident layout */
} trs_status;

/* Replaces the `gym_config` dict of GymInterface.__init__ (components/gyminterface.py:16-51;
 * keys img_w/img_h/sim_latency of core/config.py:8-9,98) plus the free parameters of
 * SURVEY.md Appendix B.  Fill with trs_default_config() first, then override. */
typedef struct trs_config {
    uint32_t struct_size;      /* = sizeof(trs_config), checked */
    int32_t  n_envs;           /* envs in THIS shard (one shard per GPU) */
    int32_t  env_id_base;      /* global id of local env 0 (RNG + start pose are keyed by global id) */
    int32_t  img_h, img_w;     /* config.py:8-9 -> 120, 160; img_w % 4 == 0 */
    int32_t  render;           /* 0 = physics only (BASELINE config 2), 1 = RGB camera */
    int32_t  auto_reset;       /* 1 = an env that finished (off track) restarts on its next step */
    int32_t  depth;            /* 1 = also write a binary32 z-depth image [n_envs][img_h][img_w] (BASELINE config 5 frame format) */
    uint64_t seed;             /* synthetic-control RNG seed, default 0x5EED */
    /* physics (trsim_spec.h) */
    float dt, max_steer, inv_wheelbase, accel_max, drag_lin, roll_res, brake_max;
    float v_max, v_rev_max, offtrack_cte, offtrack_penalty, cam_fwd;
    /* track surface + camera (binary64: only used on the host to build tables) */
    double road_half, edge_half, centre_half, dash_period, dash_on, map_margin;
    double fov_v_deg, cam_h, cam_pitch_deg, z_far;
} trs_config;

/* Device-resident outputs of the last completed step: what GymInterface.step returns
 * (components/gyminterface.py:76: last_image, pos_x, pos_y, pos_z, speed, cte) for every env,
 * plus LocationTracker's integer index (components/track_data_process.py:89-101). */
typedef struct trs_state_view {
    int32_t n_envs, img_h, img_w, n_points;
    const uint8_t* img;        /* uint8[n_envs][img_h][img_w][3] RGB, NULL when render == 0 */
    const float*   pos_x;      /* 'gym/x'     */
    const float*   pos_y;      /* 'gym/y'     */
    const float*   pos_z;      /* 'gym/z'     */
    const float*   speed;      /* 'gym/speed' = |v| */
    const float*   cte;        /* 'gym/cte'   */
    const float*   yaw;
    const float*   vel;        /* signed longitudinal speed */
    const int32_t* seg_idx;    /* LocationTracker index; 'loc/segment' = idx / n_points * 10 */
    const float*   ep_return;  /* running return of the current episode */
    const float*   last_return;/* return of the last finished episode */
    const int32_t* ep_len;
    const uint8_t* done;       /* 1 = this step ended the episode (off track / lost) */
    uint64_t step_count;       /* steps taken since create */
    const float*   depth;      /* float[n_envs][img_h][img_w] z-depth of the last frame, NULL unless cfg.depth */
} trs_state_view;

/* selectors for trs_copy_to_host */
enum {
    TRS_F_IMG = 0, TRS_F_POS_X, TRS_F_POS_Y, TRS_F_POS_Z, TRS_F_SPEED, TRS_F_CTE, TRS_F_YAW, TRS_F_VEL,
    TRS_F_SEG_IDX, TRS_F_EP_RETURN, TRS_F_LAST_RETURN, TRS_F_EP_LEN, TRS_F_DONE,
    TRS_F_MAP,       /* packed 2-bit class map, uint32[map_h][map_words] (parity checks) */
    TRS_F_ROWTAB,    /* float[img_h][2]  (row_lz, row_k)  */
    TRS_F_PALETTE,   /* uint32[img_h][4] 0x00BBGGRR       */
    TRS_F_TANGENT,   /* float[n_points][2] (tx, tz)       */
    TRS_F_STEER_FILT,/* float[n_envs] synthetic low-pass state */
    TRS_F_STATS,     /* uint64[64]: [0] off-track events, [1] resets since load_track, [2] layout faults, [3] fp16 saturations counted by trs_pilot_range_check, [8..] diagnostics */
    TRS_F_DEPTH,     /* float[n_envs][img_h][img_w] */
    TRS_F_ROWDEPTH,  /* float[img_h] */
    TRS_F_CTL_STEER, /* float[n_envs]: the handle's own control arrays — what trs_step_host uploaded or the pilot of  */
    TRS_F_CTL_THR,   /*   trs_step_pilot produced last ('ai/steering', 'ai/throttle', 'ai/breaking' of KerasPilot.step, */
    TRS_F_CTL_BRK,   /*   keras_pilot.py:92-95)                                                                       */
    TRS_F_DPITCH,    /* float[n_points]: the view-pitch offset per raw track point of a track with elevation (include/trsim_spec.h, "tracks with elevation"); all zeros on a flat track */
    TRS_F_LENS_TABLE,   /* float[img_h][img_w][4] per pixel of the lens camera (include/trsim_spec.h, "lens camera"): F, L, depth (binary32) and the lens palette
                           row as a uint32 bit pattern in word 3; the full frame, rebuilt from the host tables whatever the device keeps.  Only while a lens is set */
    TRS_F_LENS_PALETTE  /* uint32[513][4] 0x00BBGGRR: the lens palette the kernels shade from (static frame filter applied).  Only while a lens is set */
};

typedef struct trs_map_info {
    int32_t map_w, map_h, map_words;   /* cells, cells, uint32 per map row */
    double  cell, x0, z0;              /* world size of a cell, world coords of cell (0,0)'s corner */
    int32_t n_points;
    int32_t lds_bytes;                 /* dynamic LDS the step kernel is launched with */
} trs_map_info;

void trs_default_config(trs_config* cfg);

/* GymInterface.__init__ (components/gyminterface.py:49-64): connect + state init, minus the
 * TCP client, the scene load and the two 1 s sleeps (:121,:135).  `device` is a HIP device index. */
int trs_create(const trs_config* cfg, int device, trs_env** out);

/* GymInterface.onShutdown -> SDClient.stop (components/gyminterface.py:81-82). */
int trs_destroy(trs_env* env);

/* Replaces load_scene(scene_name) (components/gyminterface.py:54,166-169) and the JSON load of
 * LocationTracker.__init__ (components/track_data_process.py:72-73): raw centre-line samples
 * [x,y,z] (Unity, y up), duplicates kept.  Builds the class map and camera tables, uploads
 * them, places every env on its start pose (point (37*gid) mod n). */
int trs_load_track(trs_env* env, const double* h_xyz, int n_points);

/* reset_car (components/gyminterface.py:171-174) for the masked envs (NULL = all); host mask. */
int trs_reset(trs_env* env, const uint8_t* h_mask_or_null);

/* GymInterface.step (components/gyminterface.py:66-76) + send_controls (:156-161) for the whole
 * shard: steering/throttle in [-1,1], brake in [0,1] (NULL = 0, the `breaking is None` case :70),
 * reset truthy = restart that env (:73-74; NULL = none).  n_steps > 1 holds the controls.
 * Device pointers; asynchronous on the handle's stream. */
int trs_step(trs_env* env, const float* d_steering, const float* d_throttle,
             const float* d_brake, const uint8_t* d_reset, int n_steps);

/* Same with host arrays (the N = 1 Component path); copies the controls, then trs_step. */
int trs_step_host(trs_env* env, const float* h_steering, const float* h_throttle,
                  const float* h_brake, const uint8_t* h_reset, int n_steps);

/* Benchmark driver: controls come from the counter-based generator of trsim_spec.h
 * (SURVEY.md §8d), evaluated inside the step kernel.  steps_per_launch >= 1. */
int trs_step_synthetic(trs_env* env, int n_steps, int steps_per_launch);

/* n_steps env steps with a DIFFERENT control set per step (open-loop action sequences: action repeat, shooting-method
 * planners): d_steering / d_throttle / d_brake are [n_steps][n_envs] device arrays (d_brake NULL = 0), d_reset
 * [n_envs] applies to the first step.  Like trs_step_synthetic the call runs steps_per_launch steps per kernel launch
 * (the physics team runs ahead of the raster team through the LDS ring), so a consumer that decides on whole sequences
 * gets the multi-step throughput.  Every step's frame is rendered; the state and frame of the LAST step remain. */
int trs_step_sequence(trs_env* env, const float* d_steering, const float* d_throttle, const float* d_brake,
                      const uint8_t* d_reset, int n_steps, int steps_per_launch);
int trs_step_sequence_host(trs_env* env, const float* h_steering, const float* h_throttle, const float* h_brake,
                           const uint8_t* h_reset, int n_steps, int steps_per_launch);

/* How trs_step / trs_step_host / trs_step_synthetic / trs_step_sequence reach the GPU — the per-tick call of the reference's
 * drive loop (core/car.py:45-53: one component.step per tick with that tick's values; components/gyminterface.py:66-76).
 *   TRS_STEP_LAUNCH   (default) every call launches the step kernel(s) on the handle's stream.
 *   TRS_STEP_RESIDENT a worker kernel stays on the GPU (tables staged once, env state in LDS, one workgroup per CU) and a
 *     call only POSTS the step: control pointers into a ring in pinned host memory that the worker polls.  No kernel launch,
 *     no kernel boundary, no table re-staging per step; the physics team runs ahead of the raster team as far as posted
 *     steps allow; up to 8 steps may be in flight, a post beyond that waits.  Like every step path it stores the rows of a frame
 *     that do not depend on the pose once per frame buffer and palette, not every step: the frame buffers are read-only for the
 *     consumer (trs_get_state).  The worker leaves by itself after `idle_us`
 *     (<= 0: 2000) without a post and is started again by the next one.  While it is resident it owns the handle's stream:
 *     trs_sync waits for the posted steps only (completion flags in host memory), trs_copy_to_host / trs_fetch_outputs copy
 *     on a side stream, and every OTHER call that needs the stream (reset, set_pose, load_track, image path, control glue,
 *     pilot, events) first asks the worker to leave.  Frames and telemetry of a completed step are in HBM (written through);
 *     a consumer that reads them on its own stream does so after trs_sync.  Device-resident controls must be complete
 *     (their producer synchronised) when trs_step is called, and stay untouched until that step is done.  Physics-only
 *     handles (cfg.render == 0, BASELINE configs[1]) get their own worker since round 4 (trs_physics_worker_kernel: one env per wave,
 *     the same mailbox and completion flags; a tick costs a post instead of a launch).  Every frame filter of trs_set_frame_filter is rendered by the worker (the dynamic-brightness one by its own
 *     instantiation since round 3).
 *     Kernels of other streams that need more than ~35 KB of LDS per workgroup cannot start while the worker is resident.
 *     ONE resident worker per GPU at a time — a worker needs every workgroup of its grid on the GPU at once, one slot with most of the LDS per
 *     CU — and the library arbitrates (round 5; the reference's independent GymInterface instances simply work side by side,
 *     components/gyminterface.py:49-76):
 *       - handles of ONE process (any threads): the handle whose step needs a worker takes the GPU over; the other handle's worker finishes what
 *         was posted to it and leaves first.  Alternating handles cost a worker start per alternation (tens of microseconds), never idle_us and
 *         never an error; results are those of each handle stepped alone.  The host side of resident mode is serialised per GPU by a lock.
 *       - ANOTHER process's worker on the same GPU cannot be asked to leave.  A worker launch that does not get its whole grid onto the GPU
 *         notices within 2-4 ms (every workgroup reports in before the first post is taken), consumes nothing and leaves; a launch that has not
 *         started at all after 250 ms is cancelled.  In both cases the handle goes back to TRS_STEP_LAUNCH by itself: the posted steps run as
 *         launches, the call returns TRS_OK, trs_last_error() carries a note and trs_get_step_mode reports it.  No 2 s stall, no broken handle.
 *         Resident mode is tried again by itself 100 ms later (doubling up to 2 s while the GPU stays shared).  A worker leaves after 50 ms
 *         whatever happens and is started again by the next post: the gap is where the other process's kernels (its launches, or its own
 *         worker) get the CUs, so processes that keep a shared GPU busy take turns of 50 ms.
 *       - physics-only handles: ceil(n_envs / 4) workgroups must fit the GPU at once (a few thousand envs); trs_set_step_mode returns
 *         TRS_ERR_LIMIT with the capacity beyond that (use TRS_STEP_LAUNCH with several steps per launch for such shards). */
enum { TRS_STEP_LAUNCH = 0, TRS_STEP_RESIDENT = 1 };
int trs_set_step_mode(trs_env* env, int mode, int idle_us);
/* The handle's step mode now (either pointer may be NULL).  *fell_back = 1: resident mode had been selected and the library went back to
 * TRS_STEP_LAUNCH by itself because a worker launch was not co-resident (the GPU is shared with another process's worker, see above);
 * the library tries resident mode again by itself (100 ms later, doubling up to 2 s), trs_set_step_mode(TRS_STEP_RESIDENT) does so at once. */
int trs_get_step_mode(trs_env* env, int* mode, int* fell_back);
/* Resident mode only (a no-op otherwise): the worker leaves the GPU now — every posted step is complete in memory when the call
 * returns — and the next posted step starts a new one.  For a caller about to run work of ANOTHER stream or library that needs
 * the CUs the worker occupies (one workgroup slot and most of the LDS on every CU): a collective, a large kernel.  The step mode
 * stays TRS_STEP_RESIDENT. */
int trs_quiesce(trs_env* env);
/* trs_step followed by trs_sync in ONE call: the lock-step consumer of core/car.py:45-53 (post the controls, wait for the frame) crosses
 * the FFI once per tick instead of twice.  Same arguments and errors as trs_step. */
int trs_step_wait(trs_env* env, const float* d_steering, const float* d_throttle, const float* d_brake_or_null, const uint8_t* d_reset_or_null, int n_steps);
/* ---- test hooks of the resident worker: NOT part of libtrsim.so.  They exist only in builds with -DTRS_TEST_HOOKS (csrc/libtrsim_testhooks.so, which
 * __graft_entry__.build() compiles for tests/test_resident.py beside the product library: the same sources + these two entry points).  No reference interface
 * stands behind them.  trs_resident_debug_lifetime: a worker leaves by itself after life_us microseconds (default 50,000; <= 0 restores it) and the next post
 * starts a new one — many worker generations under load.  Needs trs_set_step_mode first.  trs_resident_debug_abort: sets the running worker's abort bit from
 * outside, as a wave does whose bounded wait gave up: every wave must leave within its next poll and the next call must fail with TRS_ERR_DEVICE ("resident
 * worker gave up") instead of hanging. */
#ifdef TRS_TEST_HOOKS
int trs_resident_debug_lifetime(trs_env* env, int life_us);
int trs_resident_debug_abort(trs_env* env);
#endif

/* Telemetry of the last step (components/gyminterface.py:76,95-104) as device pointers.
 * The frame buffers behind `img` and `depth` (two each, alternating by step) are READ-ONLY for the consumer, in every step mode: rows of a frame that do
 * not depend on the pose (sky, ground beyond the far plane: the leading rows of a flat track's frame) are stored once per buffer and palette, and later
 * steps into that buffer store only the rows that see the track.  After trs_sync the view is always a whole frame; a consumer that wrote into it would
 * find its bytes in those rows two steps later.  Copy a frame before changing it (trs_preprocess writes to a buffer of its own). */
int trs_get_state(trs_env* env, trs_state_view* out);

/* Synchronising copy of one field to host memory (`which` = TRS_F_*). `bytes` must match. */
int trs_copy_to_host(trs_env* env, int which, void* h_dst, size_t bytes);

/* What GymInterface.step returns (components/gyminterface.py:76), all fields of all envs in ONE synchronisation: the
 * copies are queued behind the last step on the handle's stream into a pinned staging buffer, followed by a single
 * stream wait.  Any pointer may be NULL.  h_img: uint8[n_envs][H][W][3]; the others n_envs elements each. */
int trs_fetch_outputs(trs_env* env, uint8_t* h_img, float* h_x, float* h_y, float* h_z, float* h_speed, float* h_cte,
                      int32_t* h_seg_idx, uint8_t* h_done);

/* ---- observation latency: what the car is told, `sim_latency` of the reference's gym_config per env (include/trsim_spec.h, "observation latency") ----
 * The reference delays every telemetry packet by sim_latency ms (components/gyminterface.py:96).  Here an env's delay is L_e ticks: after step T of the
 * history its observation is the truth record of step T - L_e (frame, depth frame, x, y, z, speed, cte, index), or the constructor's state (zeros,
 * arrived = 0) while T - L_e < 1.  The history begins at trs_set_latency and at trs_load_track; resets do not restart it.  Everything that shows what the
 * simulator did (trs_get_state, trs_fetch_outputs, trs_copy_to_host, rewards, done, returns) stays the truth, bit for bit; trs_pilot_act,
 * trs_pilot_forward*, trs_preprocess and trs_normalize with NULL sources keep meaning the newest rendered frame (pass the view's pointers for the
 * delayed one); trs_step_pilot alone switches: the controls of tick T + 1 are KerasPilot.step(observation after T) where it has arrived, else (0, 0, 0).
 *   h_ticks: int32[n_envs], each in [0, max_ticks]; 1 <= max_ticks <= 30.  NULL: off — from the next step on every byte any call shows is what a
 *   handle that never set a latency shows.  TRS_ERR_ARG for values out of range; TRS_ERR_NOMEM (the message names the bytes it wanted) when the ring
 *   of max_ticks + 2 frame slots does not fit; TRS_ERR_STATE while resident mode is selected — trs_set_step_mode(TRS_STEP_RESIDENT) is refused
 *   likewise while a latency is set.  A refused call leaves the handle unchanged.  The call synchronises the handle.
 * With a latency set every step is one launch (n_steps > 1, sequences and steps_per_launch > 1 loop single-step launches: the results do not change),
 * followed by one launch of trs_obs_kernel.  One delay for all envs moves no frame byte: the view's `img` points into the ring slot of step T - L.
 * The view handed out after step T stays intact while step T + 1 runs, like the frames of trs_get_state.  Physics-only handles: img == NULL. */
typedef struct trs_obs_view {
    uint32_t struct_size;
    int32_t  n_envs, img_h, img_w;
    const uint8_t* img;              /* uint8[n_envs][H][W][3], NULL without a camera */
    const float*   depth;            /* float[n_envs][H][W], NULL unless cfg.depth */
    const float *pos_x, *pos_y, *pos_z, *speed, *cte;
    const int32_t* seg_idx;
    const uint8_t* arrived;          /* uint8[n_envs]: 1 once T - L_e >= 1 */
} trs_obs_view;
int trs_set_latency(trs_env* env, const int32_t* h_ticks_or_null, int max_ticks);
int trs_get_latency(trs_env* env, int32_t* h_ticks_out_or_null, int* max_ticks_out);   /* *max_ticks_out == 0: off (ticks then all 0) */
int trs_get_observation(trs_env* env, trs_obs_view* out);   /* device pointers; TRS_ERR_STATE while latency is off */
/* like trs_fetch_outputs: the observation of all envs in one synchronisation, any pointer NULL */
int trs_fetch_observation(trs_env* env, uint8_t* h_img, float* h_x, float* h_y, float* h_z, float* h_speed, float* h_cte,
                          int32_t* h_seg_idx, uint8_t* h_arrived);

/* ---- tub images: frames on the device -> the img_k.jpg files of the reference's tubs (include/trsim_spec.h, "tub image (JPEG)") ----
 * The reference writes a record's image with Image.fromarray(img).save(path) (components/datastorage.py:78): baseline JPEG, quality 75, 4:2:0.
 * trs_encode_jpeg writes the same bytes, for quality in 1..100, from frames that never leave the device.
 *   d_src: uint8[n_images][H][W][3] of the handle's size, 4-byte aligned; NULL = the latest frames, as trs_normalize resolves them (n_images ==
 *     n_envs; behind every step mode, frame filter, lens, lighting and latency: the call reads whole frames after the step).
 *   d_dst: n_images slots of `cap` bytes; frame i's file starts at d_dst + i * cap.  d_len[i]: the file's length when it fits in the slot, the
 *     NEGATED length when it does not (the slot's content is then undefined).  No byte at or beyond d_dst + (i + 1) * cap and no byte of another
 *     slot is ever written; bytes of a slot beyond the file's end are left untouched.  Asynchronous, on the handle's stream.
 *   trs_jpeg_header_bytes: the length of SOI..SOS for the handle's H x W (the same for every quality).  A cap of header + 2 + H * W * 3 / 4 holds
 *     every rendered frame seen so far at quality 75 many times over; noise at quality 100 can take more than H * W * 3.
 *   trs_encode_jpeg_host: the same into handle-owned slots, then the fitting files packed back to back: h_blob[h_off[i] .. h_off[i + 1]) is
 *     frame i's file, h_off has n_images + 1 entries, h_len (optional) is d_len.  A frame that did not fit has h_off[i + 1] == h_off[i] and
 *     h_len[i] < 0.  One synchronisation, two device-to-host copies (offsets and lengths; min(blob_cap, n_images * cap) bytes of files).
 *     TRS_ERR_LIMIT when the files need more than blob_cap: h_off and h_len are valid, nothing is written past h_blob + blob_cap.
 *   TRS_ERR_ARG: quality outside 1..100, cap < header + 2, n_images < 1 (or != n_envs with d_src NULL), a NULL destination.  TRS_ERR_STATE: d_src
 *     NULL on a handle without a camera.  TRS_ERR_LIMIT: img_w > 672 (the kernel gives every 8 x 8 block of a 16-row stripe a lane of its 256).
 *   The kernel runs min(n_images, 4 x CU count) workgroups, each looping over frames.  Resident mode: the worker leaves the GPU first, as for
 *   trs_normalize, and trs_sync then waits for the encoder like for a launched step. */
int trs_jpeg_header_bytes(trs_env* env, int quality);   /* > 0: bytes of SOI..SOS; < 0: trs_status */
int trs_encode_jpeg(trs_env* env, const uint8_t* d_src_or_null, int n_images, int quality, uint8_t* d_dst, int cap, int32_t* d_len);
int trs_encode_jpeg_host(trs_env* env, const uint8_t* d_src_or_null, int n_images, int quality, int cap,
                         uint8_t* h_blob, size_t blob_cap, int64_t* h_off, int32_t* h_len_or_null);

/* ---- tub images, read back: img_k.jpg files on the device -> frames on the device (include/trsim_spec.h, "tub image (JPEG), decoding") ----
 * The reference's loaders open every img_i.jpg with Pillow (components/keras_train.py:33-57).  trs_decode_jpeg gives the same bytes, for files that
 * are already on the device (the encoder's slots, an uploaded tub) and frames that stay there (trs_pilot_forward, trs_pilot_act).
 *   File i is d_files[d_off[i] .. d_off[i] + d_len[i]); files may start at any byte offset.  That covers the slots of trs_encode_jpeg
 *     (d_off[i] = i * cap, d_len = the encoder's d_len) and a packed blob (d_off = the blob's offsets, d_len[i] = d_off[i + 1] - d_off[i]).
 *   d_dst: uint8[n_images][H][W][3] of the handle's size (rows are stored by dwords when img_w is a multiple of 4 and d_dst is 4-byte aligned).
 *   d_status[i]:  0 decoded, frame i written | 1 skipped: d_len[i] <= 0 (e.g. the encoder's overflow report), frame i untouched |
 *     2 unsupported: a JPEG file outside the accepted kind (progressive, grayscale, other sampling than 4:2:0, restart intervals, 16-bit tables,
 *       an Adobe segment, img_w <= 4, ...), frame i untouched: decode it on the host | 3 the file's size is not the handle's, frame i untouched |
 *     4 corrupt (truncated, a code no table holds, a marker inside the scan), frame i undefined.
 *   No byte outside frame i is written for file i, and no byte outside [d_off[i], d_off[i] + d_len[i]) is read, whatever the file holds.
 *   Asynchronous, on the handle's stream; needs no camera (cfg.render == 0 handles with a size work).  Resident mode: as for trs_encode_jpeg.
 *   trs_decode_jpeg_host: files packed in host memory (h_off has n_images + 1 entries, as trs_encode_jpeg_host fills it) -> h_dst, h_status;
 *     frames with status 1..3 are left as the caller had them.  Uploads the files, one synchronisation.
 *   TRS_ERR_ARG: n_images < 1, a NULL pointer (a refused call writes nothing).  TRS_ERR_LIMIT: the image is wider than the kernel's plan holds: a
 *     workgroup keeps the sample rows of 4 files (one per wave) in LDS, 40.25 KiB + 3.5 KiB per 16 columns; with 160 KiB per workgroup: img_w > 544
 *     (the error text gives the limit for the device's LDS, which is queried).
 *   The kernel runs min(ceil(n_images / 4), 2 x CU count) workgroups of 4 waves, each wave looping over files. */
int trs_decode_jpeg(trs_env* env, const uint8_t* d_files, const int64_t* d_off, const int32_t* d_len, int n_images,
                    uint8_t* d_dst /* uint8[n][H][W][3] */, int32_t* d_status);
int trs_decode_jpeg_host(trs_env* env, const uint8_t* h_blob, const int64_t* h_off /* n + 1 */, int n_images,
                         uint8_t* h_dst, int32_t* h_status);

/* ---- camera codec: the JPEG round trip every frame of the reference's pilot has been through (include/trsim_spec.h, "camera codec (JPEG round trip)") ----
 * The simulator sends 'cam/img' as a JPEG and GymInterface.on_msg_recv decodes it (components/gyminterface.py:97-99); DataStorage saves it as JPEG
 * again (components/datastorage.py:78): the reference's pilot trains and drives on lossy frames.  codec(frame, q) is what trs_decode_jpeg gives for
 * the file trs_encode_jpeg writes for `frame` at quality q — what Pillow gives for save(quality = q), then open — computed in one kernel without
 * the file: entropy coding is lossless, so the quantised coefficients go straight to the dequantiser.  Parity with the closed simulator's own
 * encoder is unpinned: its quality is not known.
 *   trs_jpeg_roundtrip: d_src uint8[n_images][H][W][3] of the handle's size, 4-byte aligned; NULL = the latest frames, as trs_encode_jpeg resolves
 *     them (n_images == n_envs; behind every step mode, lens, lighting, hills and latency: the call reads whole frames after the step).  d_dst: the
 *     same shape, 4-byte aligned; NULL = the handle's own codec buffer (n_images <= n_envs), returned through *d_out (may be NULL).  No byte outside
 *     frame i of d_dst is written for frame i, and d_src is only read.  Asynchronous, on the handle's stream.  Resident mode: the worker leaves the
 *     GPU first, as for trs_encode_jpeg, and trs_sync then waits for the kernel like for a launched step.
 *   trs_jpeg_roundtrip_host: host frames in (NULL = the latest frames) and out, synchronous (the N = 1 Component path).
 *   TRS_ERR_ARG: quality outside 1..100, n_images < 1 (or != n_envs with a NULL source, or > n_envs with a NULL destination), a misaligned pointer,
 *     a destination range that overlaps the source (a pixel is made from its neighbours' blocks: the call does not work in place).  TRS_ERR_STATE: a
 *     NULL source on a handle without a camera.  TRS_ERR_LIMIT: img_w <= 4 (the triangle filter needs more than two chroma columns), or img_w beyond
 *     what the kernel's plan holds: a workgroup keeps a 16-row stripe (raw rows, sample planes before and after the transform) in LDS, 9.5 KiB +
 *     2 KiB per 16 columns; with 160 KiB: img_w > 1200 (the error text gives the limit).  A refused call writes nothing.
 *   The kernel runs min(n_images, 4 x CU count) workgroups, each looping over frames.
 *   trs_set_camera_codec(quality): while a quality in 1..100 is set, trs_step_pilot feeds the pilot codec(frame, quality) of whichever frame it reads
 *     — the latest frame, or the delayed observation frame while a latency is set (cars nothing has reached yet stay masked) — by one pre-pass per
 *     step into the handle's codec buffer.  Everything that shows what the simulator did stays the truth, bit for bit: trs_get_state,
 *     trs_fetch_outputs, trs_copy_to_host, trs_get_observation, trs_encode_jpeg with a NULL source, depth.  0: off — from the next step on every byte
 *     and control is what a handle that never set a codec gives.  TRS_ERR_STATE: no camera; a frame filter is set (trs_set_frame_filter: the fused
 *     filter would run in FRONT of the codec, the reference's ImgPreprocessing runs behind the decoded frame — trs_preprocess on the codec's frames
 *     gives that order); trs_set_frame_filter with a filter is refused likewise while a codec is set.  A refused call leaves the handle unchanged.
 *   trs_get_camera_codec: the quality that is set, 0: none. */
int trs_jpeg_roundtrip(trs_env* env, const uint8_t* d_src_or_null, int n_images, int quality, uint8_t* d_dst_or_null, const uint8_t** d_out);
int trs_jpeg_roundtrip_host(trs_env* env, const uint8_t* h_src_or_null, int n_images, int quality, uint8_t* h_dst);
int trs_set_camera_codec(trs_env* env, int quality);
int trs_get_camera_codec(trs_env* env, int* quality);

/* Overwrite env pose (x, y, z, yaw, v) from host arrays of n_envs floats — test hook. */
int trs_set_pose(trs_env* env, const float* h_x, const float* h_y, const float* h_z,
                 const float* h_yaw, const float* h_v);

/* LocationTracker.step / __find_closest for a batch of binary64 query points
 * (components/track_data_process.py:81-101): h_idx_out[i] = integer nearest-point index. */
int trs_locate(trs_env* env, const double* h_xyz, int n_queries, int32_t* h_idx_out);

int trs_map_info_get(trs_env* env, trs_map_info* out);

/* ---- image path: ImgPreprocessing (components/img_preprocessing.py:37-102) + pilot normalisation ---- */

/* The `preprocessing_*` keys of core/config.py:15-28. */
typedef struct trs_pre_config {
    uint32_t struct_size;
    int32_t  dynamic_brightness;     /* preprocessing_dynamic_brightness_enabled (config.py:20) */
    double   brightness_baseline;    /* preprocessing_brightness_baseline, 550 (config.py:21) */
    float    contrast_ratio;         /* preprocessing_contrast_enhancement_ratio, 1.0 (config.py:18) */
    float    contrast_offset;        /* preprocessing_contrast_enhancement_offset, 125 (config.py:19) */
    int32_t  color_filter_enabled;   /* preprocessing_color_filter_enabled (config.py:22) */
    int32_t  n_filters;              /* <= 4 */
    uint8_t  hsv_lo[4][3], hsv_hi[4][3];   /* preprocessing_color_filter_hsvs (config.py:23), OpenCV 8-bit HSV, H in [0,180) */
    int32_t  dst_channel[4];         /* preprocessing_color_filter_destination_channels (config.py:24) */
    int32_t  edge_detection_enabled; /* preprocessing_edge_detection_enabled (config.py:25): cv2.Canny(img, a, b) layer (img_preprocessing.py:76-79) */
    int32_t  edge_threshold_a;       /* preprocessing_edge_detection_threshold_a, 60 (config.py:26) */
    int32_t  edge_threshold_b;       /* preprocessing_edge_detection_threshold_b, 100 (config.py:27) */
    int32_t  edge_dst_channel;       /* preprocessing_edge_detection_destination_channel, 2 (config.py:28) */
} trs_pre_config;

void trs_default_pre_config(trs_pre_config* cfg);

/* ImgPreprocessing.__process (img_preprocessing.py:37-102) for n_images frames of the env's image size: brightness /
 * contrast trim in binary32 exactly as numpy evaluates it (mean over rows 40..118, :88-99), the HSV in-range masks
 * (:65-74) and the Canny edge layer (:76-79; work arrays in LDS up to ~26,000 pixels, in an L2-resident scratch beyond)
 * written over their destination channels (:57-63).
 * d_src NULL = the env's latest frame (n_images must then be n_envs); d_dst NULL = the env's own processed-image
 * buffer (returned through *d_out).  Device pointers; asynchronous on the handle's stream. */
int trs_preprocess(trs_env* env, const trs_pre_config* cfg, const uint8_t* d_src, uint8_t* d_dst, int n_images,
                   const uint8_t** d_out);

/* Same for host frames (the N = 1 Component path): upload, process, download, synchronous. */
int trs_preprocess_host(trs_env* env, const trs_pre_config* cfg, const uint8_t* h_src, uint8_t* h_dst, int n_images);

/* ImgPreprocessing fused behind the rasteriser: with a filter set, every frame the env renders IS
 * 'cam/processed_img' — no extra pass over HBM and no extra kernel.  Possible because the trim (:92-99) and the HSV
 * in-range masks (:65-74) are functions of a pixel's colour alone and a rendered pixel's colour comes from the
 * per-row palette.  Without dynamic brightness the library filters the palette (4 classes x img_h rows) once on the
 * host and the kernel is unchanged.  With dynamic brightness (:88-91: the frame's own mean over rows 40..118) the step
 * kernel classifies those rows first, reduces the three channel sums per env, filters a per-env palette in LDS with
 * that frame's delta and shades from it; every pixel is still classified once.  Refused: the Canny layer, a
 * neighbourhood operator (use trs_preprocess).  cfg NULL = back to raw frames.  Takes effect from the next rendered
 * frame; survives trs_load_track. */
int trs_set_frame_filter(trs_env* env, const trs_pre_config* cfg_or_null);

/* ---- lens camera: the camera keys of the reference's gym_config that trs_config has no counterpart for ----
 * fish_eye_x, fish_eye_y and offset_x of DEFAULT_GYM_CONFIG (components/gyminterface.py:16-45): a per-pixel ray model with two
 * barrel strengths and a lateral camera mount, defined in include/trsim_spec.h ("lens camera"; parity with the simulator unpinned).
 *   fish_eye_x, fish_eye_y in [0, 2] (0 = pinhole along that axis); offset_x in world units, + = right of the heading, |offset_x| <= 2.
 * NULL or all zero selects the pinhole path: every frame then is byte for byte what a handle that never set a camera renders.
 * Out-of-range values return TRS_ERR_ARG and leave the handle unchanged.  Flat tracks only: a lens on a track with elevation is refused
 * (TRS_ERR_STATE), and so is trs_load_track of such a track while a lens is set; the dynamic-brightness frame filter and a lens exclude
 * each other in either order (TRS_ERR_STATE).  trs_load_track of another flat track rebuilds the lens tables for its map.  Takes effect
 * from the next step (a resident worker is quiesced and the next one starts with the new camera).  The image width must be a multiple of 8
 * for a lens (the kernels store half of the mirror-symmetric per-pixel table). */
typedef struct trs_camera {
    uint32_t struct_size;            /* = sizeof(trs_camera), checked */
    double   fish_eye_x, fish_eye_y; /* gym_config fish_eye_x / fish_eye_y */
    double   offset_x;               /* gym_config offset_x, world units */
} trs_camera;

void trs_default_camera(trs_camera* cam);   /* the pinhole: all zero */
int trs_set_camera(trs_env* env, const trs_camera* cam_or_null);
int trs_get_camera(trs_env* env, trs_camera* out);

/* ---- scene lighting: a colour gain and bias per env, for domain randomisation (include/trsim_spec.h, "scene lighting") ----
 * d_params: a caller-owned device array float[n_envs][8], {gR, gG, gB, 0, bR, bG, bB, 0} per env, read under the contract of trs_step's control
 * arrays: every frame a call renders uses the values as they stand when that call starts (behind trs_stream_wait_external in launch mode, behind
 * the post in resident mode), so values rewritten between steps need no new call (a running resident worker is not stopped for them).
 * trs_set_lighting_host copies a host array into a device buffer the handle owns and registers that.  NULL (either call) returns to the unlit
 * kernels: frames are then byte for byte what a handle that never set lighting renders.  Gain 1 and bias 0 are the identity.  Depth, state,
 * indices and returns are not touched.  With a frame filter, frames are filter(lit raw frame) (dynamic brightness: the mean of the lit frame).
 * Refused with TRS_ERR_STATE, the handle unchanged: a physics-only handle (cfg.render == 0), a lens camera (trs_set_camera) — in either order;
 * TRS_ERR_LIMIT where the lit palettes do not fit in LDS beside the track's tables (or beside the resident worker's state in resident mode).
 * Survives trs_load_track and trs_set_frame_filter.  The registering call itself synchronises the handle (and stops a resident worker). */
int trs_set_lighting(trs_env* env, const float* d_params_or_null);
int trs_set_lighting_host(trs_env* env, const float* h_params_or_null);

/* Pilot-side normalisation (components/keras_pilot.py:49-55, keras_train.py:41-42): float32(img) / 255.
 * d_src NULL = latest frame; d_dst = float[n_images][H][W][3] device buffer. */
int trs_normalize(trs_env* env, const uint8_t* d_src, float* d_dst, int n_images);
int trs_normalize_host(trs_env* env, const uint8_t* h_src, float* h_dst, int n_images);

/* DriverAssistance.step (components/driver_assistance.py:13-31) for N cars, in place on device control arrays:
 * mode 0 = 'steering' (|steering| <= k / speed, throttle -0.1 when limited), mode 1 = 'speed' (throttle = brake = 0
 * above k / steering).  d_speed NULL = the env's own 'gym/speed'.  Evaluated in binary64 like the reference's Python
 * floats, stored as binary32. */
int trs_driver_assist(trs_env* env, int mode, double k, float* d_steering, float* d_throttle, float* d_brake,
                      const float* d_speed, int n);
int trs_driver_assist_host(trs_env* env, int mode, double k, float* h_steering, float* h_throttle, float* h_brake,
                           const float* h_speed, int n);

/* ControlMultiplexer.step (components/controlmultiplexer.py:24-43) for N cars, one call = one tick of the Car loop.
 * Per car: mode HUMAN -> (usr steering, usr throttle, usr breaking); AI_STEERING -> (ai steering, usr throttle,
 * usr breaking); AI -> (ai steering, ai throttle, ai breaking) (:26-31); any other mode value leaves that car's outputs
 * untouched (the reference returns an empty tuple and the pool keeps its values).  Entering AI from another mode (:33)
 * starts the enabled launch locks (:45-70), which override steering / throttle (:37-40) until they end.  The reference
 * ends a lock from a thread that sleeps `duration` seconds; with the env's fixed tick this becomes `*_lock_ticks`
 * ticks = ceil(duration x loop_hz) counted from the tick of the transition, and the reference's re-trigger behaviour is
 * kept: EVERY trigger schedules its own end, so a lock restarted while an older one is pending ends when the OLDER
 * sleep elapses (up to 8 pending ends per car are tracked).  State (last mode, lock flags, pending ends, tick
 * counter) lives in the handle; n <= n_envs. */
enum { TRS_MODE_HUMAN = 0, TRS_MODE_AI_STEERING = 1, TRS_MODE_AI = 2 };   /* DriveMode (components/controller.py:7-10) */

typedef struct trs_mux_config {
    uint32_t struct_size;
    int32_t  throttle_lock_enabled;   /* ai_launch_boost_throttle_enabled, False (core/config.py:57) */
    float    throttle_lock_value;     /* ai_launch_boost_throttle_value, 1.0 (config.py:58) */
    int32_t  throttle_lock_ticks;     /* ai_launch_boost_throttle_duration 5 s (config.py:59) x 20 Hz = 100; >= 1 */
    int32_t  steering_lock_enabled;   /* ai_launch_lock_steering_enabled, False (config.py:61) */
    float    steering_lock_value;     /* ai_launch_lock_steering_value, 0.0 (config.py:62) */
    int32_t  steering_lock_ticks;     /* ai_launch_lock_steering_duration 3 s (config.py:63) x 20 Hz = 60; >= 1 */
} trs_mux_config;

void trs_default_mux_config(trs_mux_config* cfg);

/* Device pointers (float[n], mode uint8[n]); d_mux_* are what the next trs_step consumes ('mux/steering',
 * 'mux/throttle', 'mux/breaking').  Asynchronous on the handle's stream. */
int trs_control_mux(trs_env* env, const trs_mux_config* cfg, const uint8_t* d_mode,
                    const float* d_usr_steering, const float* d_usr_throttle, const float* d_usr_breaking,
                    const float* d_ai_steering, const float* d_ai_throttle, const float* d_ai_breaking,
                    float* d_mux_steering, float* d_mux_throttle, float* d_mux_breaking, int n);
/* Host arrays in and out (h_mux_* are read first: a car with an unknown mode keeps its values), synchronous. */
int trs_control_mux_host(trs_env* env, const trs_mux_config* cfg, const uint8_t* h_mode,
                         const float* h_usr_steering, const float* h_usr_throttle, const float* h_usr_breaking,
                         const float* h_ai_steering, const float* h_ai_throttle, const float* h_ai_breaking,
                         float* h_mux_steering, float* h_mux_throttle, float* h_mux_breaking, int n);
/* Back to the constructor's state (controlmultiplexer.py:10-20): last mode HUMAN, no lock, tick 0. */
int trs_control_mux_reset(trs_env* env);

/* ---- pilot in the loop: cnn_2d_speed_control (BASELINE config 5) ---- */

/* Post-processing constants of KerasPilot (components/keras_pilot.py:31-38; core/config.py:65-66,76-80). */
typedef struct trs_pilot_config {
    uint32_t struct_size;
    float   spd_ctl_threshold;            /* 1.1 */
    int32_t spd_ctl_break;                /* 0: reverse throttle when overspeeding; 1: brake instead (keras_pilot.py:88-90) */
    float   spd_ctl_reverse_multiplier;   /* 1.0 */
    float   spd_ctl_break_multiplier;     /* 1.0 */
    int32_t smooth_steering_enabled;      /* keras_pilot.py:147-153 */
    float   smooth_steering_threshold;    /* 0.9 */
    int32_t model_type;                   /* TRS_PILOT_* below; both types run the same network (keras_train.py:386-395) */
} trs_pilot_config;

enum {
    TRS_PILOT_SPD_CTL = 0,  /* ModelType.CNN_2D_SPD_CTL: outputs (steering, speed / 20) + the speed controller (keras_pilot.py:78-95) */
    TRS_PILOT_CNN_2D = 1,   /* ModelType.CNN_2D: outputs (steering, throttle), both capped to [-1, 1], breaking 0 (keras_pilot.py:56-64) */
    TRS_PILOT_SPD_FTR = 2,  /* ModelType.CNN_2D_SPD_FTR: Keras_2D_CNN.get_model(num_feature_vectors = 1) (keras_train.py:127-174,390-392); the model also
                               reads speed / 20; outputs (steering, throttle) capped, breaking 0 (keras_pilot.py:67-76) */
    TRS_PILOT_FULL_HOUSE = 3 /* ModelType.CNN_2D_FULL_HOUSE: Keras_2D_FULL_HOUSE.get_model (keras_train.py:184-245,396-398); inputs frame, speed / 20,
                               'loc/segment'; outputs (steering, speed / 20) + the speed controller (keras_pilot.py:97-118) */
};

void trs_default_pilot_config(trs_pilot_config* cfg);

/* Which kernel serves which layer is decided by trs_pilot_load from the frame size (table: DESIGN.md §3 "shape -> kernel").  This
 * struct is the ONE place where that choice can be overridden — by tests that compare a kernel with the simpler kernel it replaced
 * (same weights, same frames; tests/test_pilot.py) and by measurements (scripts/).  Nothing in the library reads the environment
 * for it.  trs_default_pilot_tuning fills in the defaults; trs_pilot_set_tuning stores a copy in the handle, used by every later
 * trs_pilot_load (NULL = back to the defaults). */
typedef struct trs_pilot_tuning {
    uint32_t struct_size;
    int32_t no_fuse;             /* 0; 1: conv1 and conv2 as separate kernels (trs_conv_u8_kernel, trs_conv_span_kernel) */
    int32_t fuse_band_r2;        /* 6: conv2 rows per band of the fused head (trs_conv12_band_kernel); 0: never fuse */
    int32_t fuse_wsplit_max;     /* 4: a band may be cut into up to this many parts in width (240x320 needs 2); 1: never (a frame whose whole-width band does not fit LDS then runs unfused) */
    int32_t fuse_roll;           /* 1: with a (frame, part) per CU or more, a workgroup walks a frame's bands top to bottom and computes the 3 conv1 rows two bands share once; 0: never */
    int32_t span_layers_mask;    /* 0x6: bit i = conv(i+1) on trs_conv_span_kernel when it is not served by a fused / frame kernel (else trs_conv_lt_kernel) */
    int32_t frame5;              /* 1: conv3 on trs_conv_frame5_kernel (whole input frames in LDS, or row bands of them where a frame does not fit: 240x320); 0: span kernel; 2 = 1 (until round 4: "also in row bands") */
    int32_t frame_layers_mask;   /* 0x78: bit i = conv(i+1) (3x3 layers) on trs_conv_frame_kernel where its input fits LDS (else trs_conv_lt_kernel) */
    int32_t chain_layers;        /* 4: conv4..conv7 in one launch (trs_conv_chain_kernel) when F frames of every activation fit LDS; 3: conv5..7; 0: off */
    int32_t dense;               /* 1: dense1 / dense4 with 64 frames per workgroup where K is long (240x320), else 32; 2: always 32 (A/B) */
    int32_t ksplit;              /* 0: automatic; else K slices of dense1 */
} trs_pilot_tuning;
void trs_default_pilot_tuning(trs_pilot_tuning* t);
int trs_pilot_set_tuning(trs_env* env, const trs_pilot_tuning* t_or_null);

/* Load the weights of Keras_2D_CNN.get_model(input_shape=(img_h,img_w,3), num_outputs=2) (components/keras_train.py:127-174,
 * selected for cnn_2d_speed_control at :393-395): 11 layers, in order conv1..conv7, dense1, dense2, dense3, output_layer;
 * h_arrays[2*i] = kernel in Keras layout ([KH][KW][CIN][COUT] / [IN][OUT], float32), h_arrays[2*i+1] = bias.  Replaces
 * load_model(model_path) (components/keras_pilot.py:26); weights are rounded to binary16 (fp16) for the MFMA convolutions (bfloat16 until round 2: the same MFMA rate, 3 fewer mantissa bits). */
int trs_pilot_load(trs_env* env, const float* const* h_arrays, int n_arrays);
/* n_arrays selects the architecture (kernel, bias per layer, Keras layouts; BY LAYER NAME, in this order — the order of
 * model.get_weights() of a functional model with several inputs depends on Keras's layer sorting, so bind by name):
 *   22  conv1..conv7, dense1, dense2, dense3, output_layer                           cnn_2d_speed_control, cnn_2d
 *   28  ... as above (dense1 has 16 more input rows), feature1, feature2, feature3     cnn_2d_speed_as_feature
 *   42  conv1..conv7, dense1 (+64 rows), dense2, dense3, output_speed, feature1..3, current_spd_1..3,
 *       dense4 (+128 rows), dense5, dense6, out_steering                              cnn_2d_full_house
 * The rows of dense1 / dense4 over the flattened conv7 output run on the matrix cores (fp16 weights); the small branches and
 * everything behind them are fp32. */

/* model(img_arr) of KerasPilot.step (keras_pilot.py:49-55,81): uint8 frames -> raw outputs float[n_images][2]
 * (steering, speed/20).  d_frames NULL = the env's latest frames (n_images == n_envs). */
int trs_pilot_forward(trs_env* env, const uint8_t* d_frames, int n_images, float* d_out);
int trs_pilot_forward_host(trs_env* env, const uint8_t* h_frames, int n_images, float* h_out);
/* ... for the model types with more inputs (keras_pilot.py:67-71,97-104): speed is divided by 20 inside, segment is 'loc/segment';
 * NULL = the env's own (n_images == n_envs). */
int trs_pilot_forward_ex(trs_env* env, const uint8_t* d_frames, const float* d_speed, const float* d_segment, int n_images, float* d_out);
int trs_pilot_forward_host_ex(trs_env* env, const uint8_t* h_frames, const float* h_speed, const float* h_segment, int n_images, float* h_out);

/* Activations of one layer of the last forward pass as float32 (tests): layer 0..6 = conv1..conv7 output
 * [n][OH][OW][C], 7 = dense1 [n][100]. */
int trs_pilot_debug_layer(trs_env* env, int layer, float* h_dst, size_t n_floats);

/* The reference runs the network in fp32 (components/keras_pilot.py:49-59: float32 frames into a Keras model); this library stores activations as
 * binary16 and SATURATES them at 65504 in every convolution epilogue (an overflow cannot become an infinity downstream) — silently, because a
 * per-step counter would cost every epilogue instructions.  trs_pilot_range_check is how a model's range is validated: after a forward pass
 * on representative frames (trs_pilot_forward / _host / trs_pilot_act / trs_step_pilot) it counts the saturated elements (stored value 65504) of
 * every convolution's activation of THAT pass — the ones the fused kernels keep in LDS are recomputed by the single-layer kernels — into
 * h_out[0..6] (conv1..conv7) and their sum into h_out[7]; the sum is also added to TRS_F_STATS[3].  0 everywhere = the pass stayed inside
 * binary16's range and differs from fp32 by rounding only (about 1e-3 relative per output at the top of the range, tests/test_pilot.py). */
int trs_pilot_range_check(trs_env* env, uint64_t h_out[8]);

/* KerasPilot.step (keras_pilot.py:45-95,139-153) for n cars on DEVICE arrays — the part of a device-resident pilot -> mux -> sim
 * graph (car_templates/manage.py:46-75): model(d_frames), then the model type's post-processing, written to d_steering /
 * d_throttle / d_breaking (float[n]: 'ai/steering', 'ai/throttle', 'ai/breaking').  d_frames NULL = the env's latest frames
 * (n == n_envs; no frame yet -> zeros, keras_pilot.py:46-47); d_speed NULL = the env's own 'gym/speed'; d_segment ('loc/segment',
 * read by cnn_2d_full_house only) NULL = from the env's own tracker index; d_mode (uint8[n],
 * TRS_MODE_*) NULL = every car in an AI mode, else cars outside AI / AI_STEERING get (0, 0, 0) (:139).  Asynchronous on the
 * handle's stream; frames never leave the device. */
int trs_pilot_act(trs_env* env, const trs_pilot_config* cfg, const uint8_t* d_frames, const float* d_speed, const float* d_segment,
                  const uint8_t* d_mode, float* d_steering, float* d_throttle, float* d_breaking, int n);

/* Closed loop for n_steps (the reference's tick order, car_templates/manage.py:46-75: the pilot acts on the frame the
 * sim stored on the previous tick): controls = KerasPilot.step(frame, speed) for ModelType.CNN_2D_SPD_CTL
 * (keras_pilot.py:78-95: cap steering, predicted speed x 20, calcThrottle / calcBreak of utils/mapping.py:23-35) or for
 * ModelType.CNN_2D (:56-64: both outputs capped, breaking 0), smooth steering for both,
 * then one env step with those controls.  Before the first frame exists the controls are (0, 0, 0) (keras_pilot.py:46-47). */
int trs_step_pilot(trs_env* env, const trs_pilot_config* cfg, int n_steps);

/* ---- scripted expert: the stand-in for the reference's human driver (include/trsim_spec.h, "scripted expert"; HIP library only) ----
 * The reference's training data comes from a person with a joystick: JoystickController writes 'usr/steering', 'usr/throttle', 'usr/breaking'
 * (components/controller.py:24).  The expert is a rule on the env's own state (the truth, never a delayed observation): steer against the cross-track
 * error and the heading error `look` track points ahead, hold a speed.  It exists per handle, on the device, in launch mode.
 *   trs_set_expert: validates, builds track_yaw from the handle's tangents and uploads the tables; zeroes the driver's tick counter k and its disturbance
 *     state w.  cfg NULL: the expert is switched off.  h_target: float[n_envs] speed target per env (NULL: cfg.target_speed for all); h_profile:
 *     float[n_points] speed limit per track point (NULL: none).  TRS_ERR_STATE without a track; a later trs_load_track switches the expert off again.
 *     TRS_ERR_ARG: struct_size, look outside [0, n_points), a field that is not finite.  The call synchronises the handle.
 *   trs_expert_act: the pure rule (no disturbance; k and w do not move) for envs 0..n-1 of whatever state the handle is in, into device arrays float[n]
 *     ('usr/steering', 'usr/throttle', 'usr/breaking'; after trs_step_pilot: DAgger labels).  n <= n_envs.  Asynchronous on the handle's stream.
 *   trs_step_expert: the closed loop in the shape of trs_step_pilot.  Per tick ONE launch of trs_expert_kernel writes the applied controls (label plus
 *     the disturbance) into the handle's own control arrays (TRS_F_CTL_*) and, when a capture is due, the record rows; one env step by launch follows.
 *     Resident mode and latency as for trs_step_pilot: a resident worker is asked to leave, and the truth is stepped.
 *   Capture (cap NULL: none).  The tick with counter k is captured when k >= skip and (k - skip) % every == 0, until `capacity` slots of THIS call are
 *     full; a tick is not captured when frames are asked for and no frame exists yet (before the handle's first step).  Slot s: d_rows[s][n_envs][8] =
 *     (steering label, throttle label, breaking label, applied steering, speed, cte, 'loc/segment' = (float)((double)seg_idx / n_points * 10), done) and,
 *     with d_frames, d_frames[s][n_envs][H][W][3]: the rendered frame of the state the label was computed on (the truth, not the camera codec's frame:
 *     put a data set through trs_jpeg_roundtrip afterwards), copied device to device on the handle's stream in front of the step.  No byte of a slot
 *     that is not captured is written.  *n_captured (may be NULL): slots filled by this call.
 *     TRS_ERR_ARG: struct_size, every < 1, skip < 0, capacity < 0, capacity > 0 without d_rows, d_frames on a handle without a camera.
 *     TRS_ERR_STATE: no expert set.  A refused call leaves the handle unchanged. */
typedef struct trs_expert_config {
    uint32_t struct_size;
    int32_t  look;                   /* 6: track points ahead for the heading error */
    float    k_cte, k_head;          /* 1, 2 */
    float    thr_hi, thr_lo;         /* 0.6 below the speed target, 0.1 at or above it */
    float    target_speed;           /* 6 */
    float    brake_over, brake_val;  /* 1.15, 0.5: brake_val while speed > target * brake_over */
    float    alpha, sigma;           /* 0.1, 0: the low-pass constant and the amplitude of the steering disturbance */
    uint64_t seed;                   /* 0: the seed of the disturbance */
} trs_expert_config;
typedef struct trs_expert_capture {
    uint32_t struct_size;
    int32_t  every, skip, capacity;
    uint8_t* d_frames_or_null;
    float*   d_rows;
} trs_expert_capture;
void trs_default_expert_config(trs_expert_config* cfg);
int trs_set_expert(trs_env* env, const trs_expert_config* cfg_or_null, const float* h_target_or_null, const float* h_profile_or_null);
int trs_expert_act(trs_env* env, float* d_steering, float* d_throttle, float* d_breaking, int n);
int trs_step_expert(trs_env* env, int n_steps, const trs_expert_capture* cap_or_null, int* n_captured_or_null);

/* ---- pilot in the loop with the expert's labels: dataset aggregation, DAgger (include/trsim_spec.h, "pilot in the loop with the expert's labels";
 *      HIP library only) ----
 * trs_step_expert records states the EXPERT reaches; a trained pilot drifts into states the expert never visits.  Here the loaded pilot drives, or a keyed
 * mixture of pilot and expert, and the expert's answer to every visited state is the recorded label.  Needs trs_set_expert, trs_pilot_load and a camera.
 *   trs_step_dagger: the closed loop in the shape of trs_step_pilot, for n_steps ticks.  Per tick: the pilot acts exactly as in trs_step_pilot (same frame
 *     source: the latest frame, the delayed one under trs_set_latency, the codec's under trs_set_camera_codec; same speed, segment and mode mask; (0, 0, 0)
 *     before a frame exists) into the handle's control arrays; ONE launch of trs_dagger_kernel computes the expert's pure label on the truth (the
 *     disturbance state w does NOT move and sigma is ignored — unlike trs_step_expert), draws the gate, overwrites the control arrays (TRS_F_CTL_*) with the
 *     applied controls, writes the record row when a capture is due and updates the stats; one env step by launch follows.  The driver's tick counter k
 *     (zeroed by trs_set_expert, shared with trs_step_expert) advances by one per tick.
 *     Gate: per global env id and per block of `hold` ticks of k, the expert drives iff u < beta, u from SplitMix64 of cfg.seed (beta 0: never, beta 1:
 *     always); identical in every shard.  Applied steering: the label where the expert drives, else the pilot's.  expert_speed = 1: throttle and brake are
 *     ALWAYS the labels ("applied as labelled", as in trs_step_expert), so the speed label of the speed_ctl and full_house loaders — the car's own speed /
 *     20 — shows the expert's speed behaviour.  expert_speed = 0: throttle and brake follow the gate like the steering; those two loaders' speed label is
 *     then the PILOT's own speed and is not a correction.
 *   Capture: trs_expert_capture and its rule as for trs_step_expert (every, skip, capacity per call, no byte of an uncaptured slot written, no capture of
 *     frames while no frame exists).  Row: (steering label, throttle label, breaking label, applied steering, speed, cte, 'loc/segment', done) —
 *     TRS_LABEL_EXPERT is the correction, TRS_LABEL_APPLIED what the car was given.  Frame: the frame the pilot was FED this tick (the codec's output under a
 *     camera codec; the delayed frame under a latency, zeros for cars nothing has reached yet; otherwise the latest frame) — unlike trs_step_expert, which
 *     captures the rendered truth.  It is the pair the pilot is judged on, and the pair the reference's tubs hold under sim_latency.
 *   trs_dagger_stats: float[n_envs][6] per env, updated on every tick of trs_step_dagger whether captured or not: ticks, ticks the expert drove, sum |cte|,
 *     max |cte|, sum |pilot steering - label|, ticks with done set (cte and done of the state the label was computed on; binary32 additions in tick order,
 *     counts exact below 2^24 ticks).  h_out (may be NULL): filled, the call then synchronises; *d_out (may be NULL): the handle-owned device array;
 *     reset != 0: zeroed behind the read.  trs_set_expert zeroes them too; resets of a car touch neither k nor the stats.
 *   Refusals (a refused call leaves the handle, k and the stats unchanged).  TRS_ERR_STATE: no expert set, no pilot loaded, no camera; trs_dagger_stats
 *     without an expert.  TRS_ERR_ARG: either struct_size, beta not finite or outside [0, 1], hold < 1, expert_speed not 0 or 1, n_steps < 1, the pilot
 *     config's model type not matching the weights (as trs_step_pilot), the capture refusals of trs_step_expert.
 *   Resident mode as for trs_step_pilot and trs_step_expert: a resident worker is asked to leave. */
typedef struct trs_dagger_config {
    uint32_t struct_size;
    float    beta;                   /* 0.5: the probability that the expert holds the wheel in a block of `hold` ticks */
    int32_t  hold;                   /* 1: ticks per block of the gate */
    int32_t  expert_speed;           /* 1: throttle and brake always as labelled; 0: they follow the gate */
    uint64_t seed;                   /* 0: the seed of the gate */
} trs_dagger_config;
void trs_default_dagger_config(trs_dagger_config* cfg);
int trs_step_dagger(trs_env* env, const trs_pilot_config* pilot_cfg, const trs_dagger_config* cfg, int n_steps, const trs_expert_capture* cap_or_null,
                    int* n_captured_or_null);
int trs_dagger_stats(trs_env* env, float* h_out_or_null, const float** d_out_or_null, int reset);

/* ---- training minibatches: DataLoader.load's split, shuffle and batch on the device (include/trsim_spec.h, "training minibatches"; HIP library only) ----
 * The reference's trainer turns every record into float32 on the host, splits 0.8 / 0.2, shuffles and batches with drop_remainder
 * (components/keras_train.py:33-69).  Here the set stays where trs_step_expert's capture left it — d_frames uint8[n_records][H][W][3] of the handle's
 * size, d_rows float[n_records][8] — and a training step asks for one minibatch at a time.
 *   trs_sample_batch: positions first .. first + batch - 1 of epoch `epoch` of split `split` (TRS_SPLIT_*), gathered by ONE launch of trs_batch_kernel,
 *     asynchronous on the handle's stream.  Slot k of the batch holds the record at position first + k:
 *       d_images    [batch][H][W][3] (TRS_LAYOUT_NHWC) or [batch][3][H][W] (TRS_LAYOUT_NCHW) of float, binary16 or uint8 (cfg.dtype)
 *       d_features  float[batch][F], F = 0, 0, 1, 2 for TRS_LOADER_SPEED_CTL, _DEFAULT, _SPEED_FEATURE, _FULL_HOUSE (may be NULL when F == 0)
 *       d_labels    float[batch][2]
 *       d_index     int32[batch], the record numbers (may be NULL)
 *     A physics-only set has no frames: d_frames and d_images are both NULL.  batch == 0 is accepted and writes nothing.
 *     TRS_ERR_ARG, nothing written: struct_size, an unknown loader / label / layout / dtype / split, NCHW with uint8, n_records < 0, n_train outside
 *     [0, n_records], epoch < 0, first < 0, batch < 0, first + batch beyond the split, d_rows or d_labels NULL, d_features NULL with F > 0, exactly
 *     one of d_frames and d_images NULL, d_images not 16-byte aligned, any other pointer not 4-byte aligned, frames on a handle without a camera
 *     (cfg.render == 0).  Source and destination must not overlap.  A resident worker leaves the GPU first, as for trs_normalize.
 *   trs_loader_order: the same record numbers on the host, positions first .. first + count - 1, without a GPU (callable on a machine that has none):
 *     which records a batch held.  The refusals that concern cfg, split, epoch and the range are the same. */
enum { TRS_LOADER_SPEED_CTL = 0, TRS_LOADER_DEFAULT = 1, TRS_LOADER_SPEED_FEATURE = 2, TRS_LOADER_FULL_HOUSE = 3 };   /* the order of TRS_PILOT_* */
enum { TRS_LABEL_EXPERT = 0, TRS_LABEL_APPLIED = 1 };     /* 'mux/steering' = the expert's label, or the disturbed steering the car was given */
enum { TRS_LAYOUT_NHWC = 0, TRS_LAYOUT_NCHW = 1 };
enum { TRS_DTYPE_F32 = 0, TRS_DTYPE_F16 = 1, TRS_DTYPE_U8 = 2 };
enum { TRS_SPLIT_TRAIN = 0, TRS_SPLIT_VAL = 1 };
typedef struct trs_loader_config {
    uint32_t struct_size;
    int32_t  loader, label, layout, dtype;   /* TRS_LOADER_SPEED_CTL, TRS_LABEL_EXPERT, TRS_LAYOUT_NCHW, TRS_DTYPE_F32 */
    int32_t  n_records, n_train;             /* 0, 0: the caller's set */
    uint64_t seed;                           /* 0 */
} trs_loader_config;
void trs_default_loader_config(trs_loader_config* cfg);
int trs_sample_batch(trs_env* env, const trs_loader_config* cfg, const uint8_t* d_frames_or_null, const float* d_rows, int split, int epoch, int first,
                     int batch, void* d_images_or_null, float* d_features_or_null, float* d_labels, int32_t* d_index_or_null);
int trs_loader_order(const trs_loader_config* cfg, int split, int epoch, int first, int count, int32_t* h_index);

/* ---- training minibatches, augmentation: mirror and colour jitter inside the gather (include/trsim_spec.h, "training minibatches, augmentation") ----
 * A record is varied between epochs without another pass over the batch: mirrored left to right with its steering label negated, and lit again by the
 * scene-lighting rule (light_channel, rule R1) with a gain and a bias per record.  The draws are keyed by (aug.seed, epoch, record number), not by the
 * batch slot: reproducible, the same in every shard, and readable on the host.
 *   trs_default_augment_config: everything off (mirror_prob, gain_amp, bias_amp = 0).
 *   trs_sample_batch_aug: trs_sample_batch with the augmentation applied by the same single launch.  It replaces the torch passes a user runs behind the
 *     plain batch today (flip where flagged, x * gain + bias, clamp, the label's sign).  aug NULL, or a config that is off, launches trs_batch_kernel as
 *     trs_sample_batch does: the same bytes at the same cost.  Otherwise ONE launch of trs_batch_aug_kernel: every frame byte x becomes
 *     light_channel(x, gain_c, bias_c) before the conversion of cfg.dtype, a mirrored record has out[y][x] = lit[y][W - 1 - x] in every channel and the
 *     sign bit of its label[0] flipped; label[1], the features, d_index and the order are trs_sample_batch's.  A physics-only set gets the label rule alone.
 *     TRS_ERR_ARG, nothing written: every refusal of trs_sample_batch; aug.struct_size; mirror_prob outside [0, 1], gain_amp outside [0, 1), bias_amp
 *     outside [0, 255] (a NaN is outside); per_channel not 0 or 1; mirror_prob > 0 with TRS_LOADER_FULL_HOUSE (loc/segment is a position on the track as
 *     driven).
 *   trs_loader_augment: what positions first .. first + count - 1 of (split, epoch) get, on the host without a GPU or a handle, like trs_loader_order —
 *     it replaces reading the draws back from a batch: h_index (may be NULL) the record numbers, h_mirror[count] 0 / 1, h_params[count][8] =
 *     {gR gG gB 0 bR bG bB 0}, the layout of trs_set_lighting.  The refusals of trs_loader_order and those of aug above; aug must not be NULL. */
typedef struct trs_augment_config {
    uint32_t struct_size;
    float    mirror_prob;            /* 0: the probability that a record is mirrored */
    float    gain_amp, bias_amp;     /* 0, 0: gain_c = 1 + f * gain_amp, bias_c = f * bias_amp, f drawn from [-1, 1) */
    int32_t  per_channel;            /* 0: one gain and one bias for R, G and B; 1: one per channel */
    uint64_t seed;                   /* 0: the seed of the draws (independent of trs_loader_config.seed) */
} trs_augment_config;
void trs_default_augment_config(trs_augment_config* aug);
int trs_sample_batch_aug(trs_env* env, const trs_loader_config* cfg, const trs_augment_config* aug_or_null, const uint8_t* d_frames_or_null,
                         const float* d_rows, int split, int epoch, int first, int batch, void* d_images_or_null, float* d_features_or_null,
                         float* d_labels, int32_t* d_index_or_null);
int trs_loader_augment(const trs_loader_config* cfg, const trs_augment_config* aug, int split, int epoch, int first, int count, int32_t* h_index_or_null,
                       uint8_t* h_mirror, float* h_params);

/* ---- training the pilot's tail: dense1 .. output_layer on the device, conv1 .. conv7 frozen (include/trsim_spec.h, "training the pilot's tail") ----
 * The reference's trainer continues from a saved model (components/keras_train.py:376,400-401) with optimizers.Adam(lr=0.001) on 'mse' (:404).  Here the
 * loaded pilot of a 22-array model type (cnn_2d_speed_control, cnn_2d) is trained where it drives: a step runs the convolutions and dense1 by the kernels
 * of trs_pilot_forward, takes the loss and its gradient through the four dense layers, and moves them by Adam, all on the handle's stream and without a
 * byte crossing to the host.  After a step the handle drives with the updated pilot (trs_pilot_forward, trs_pilot_act, trs_step_pilot, trs_step_dagger).
 * What stays out: conv1 .. conv3 (conv4 .. conv7 can be trained as well: the next section), dropout behind conv1 .. conv6 (behind conv7 and the hidden
 * dense layers: the section after it), cnn_2d_full_house (42 arrays; the 28-array type: "training the speed-as-feature pilot" below), feature caching
 * across epochs, any exchange of gradients between GPUs.
 *   trs_pilot_train_begin: fp32 master weights and Adam's m and v (zero) for the eight arrays dense1 .. output_layer, t = 0.  The handle keeps dense1 as
 *     binary16 only, so h_tail_arrays[0], dense1's kernel float[F][100] as trs_pilot_load got it, is read from the host; the other seven arrays are taken
 *     from the device, where the tail kernel reads them (entries 1..7 are not read and may be NULL).  cfg NULL: the defaults.
 *   trs_pilot_train_step: one step on d_frames uint8[n][H][W][3] and d_labels float[n][2], 1 <= n <= n_envs; d_loss (may be NULL) receives the loss of the
 *     batch BEFORE the update, sum (out - y)^2 / (2 n).  Asynchronous on the handle's stream.  A resident worker is asked to leave, as for trs_pilot_forward.
 *   trs_pilot_train_get: the fp32 masters in Keras layouts into h_tail_arrays_out[0..7] (a NULL entry is skipped) and the step count; synchronises.
 *   trs_pilot_train_debug: item `which` (TRS_TRAIN_DBG_*) of the last step as floats; the sibling of trs_pilot_debug_layer.  Synchronises.
 *   trs_pilot_train_end: releases the session's buffers; the handle keeps driving with the trained weights.
 *   Refusals.  TRS_ERR_STATE: no pilot loaded; begin twice; step, get, debug or end without begin; trs_pilot_load or trs_pilot_set_tuning between begin
 *     and end (end the session first).  TRS_ERR_LIMIT: a pilot of 28 or 42 arrays (28: trs_pilot_train_begin_ex).  TRS_ERR_ARG: the config (struct_size; lr or eps not positive and
 *     finite; a beta outside [0, 1); train_mask 0 or with bits beyond 3), a NULL dense1 kernel, n outside [1, n_envs], NULL frames or labels, an unknown
 *     item or a size that is not the item's. */
typedef struct trs_train_config {
    uint32_t struct_size;
    float    lr, beta1, beta2, eps;  /* 0.001, 0.9, 0.999, 1e-7: optimizers.Adam(lr=0.001) with Keras's defaults */
    uint32_t train_mask;             /* 0xF: bit l = layer l of dense1, dense2, dense3, output_layer is trained; a masked layer keeps every bit */
} trs_train_config;
enum {
    TRS_TRAIN_DBG_OUT = 0,           /* float[n][2]: the outputs the loss was taken on */
    TRS_TRAIN_DBG_Z1, TRS_TRAIN_DBG_Z2, TRS_TRAIN_DBG_Z3,                          /* pre-activations [n][100], [n][50], [n][25] */
    TRS_TRAIN_DBG_DELTA1, TRS_TRAIN_DBG_DELTA2, TRS_TRAIN_DBG_DELTA3, TRS_TRAIN_DBG_DELTA4,   /* [n][100], [n][50], [n][25], [n][2] */
    TRS_TRAIN_DBG_GW1, TRS_TRAIN_DBG_GW2, TRS_TRAIN_DBG_GW3, TRS_TRAIN_DBG_GW4,    /* [F][100], [100][50], [50][25], [25][2] */
    TRS_TRAIN_DBG_GB1, TRS_TRAIN_DBG_GB2, TRS_TRAIN_DBG_GB3, TRS_TRAIN_DBG_GB4,
    TRS_TRAIN_DBG_M = 16,            /* + a (0..7): Adam's m of array a, in the order of trs_pilot_train_begin */
    TRS_TRAIN_DBG_V = 24,            /* + a: Adam's v */
    TRS_TRAIN_DBG_SCALE_EXP = 32,    /* 1 float: the exponent s of the batch's scale 2^s */
    TRS_TRAIN_DBG_LOSS = 33,         /* 1 float */
    TRS_TRAIN_DBG_PACK1 = 34,        /* float[F][100]: dense1's binary16 copy as the dense kernel reads it, widened */
    /* (35 stays unknown) the activations dense2, dense3 and output_layer read, float[n][100], [n][50], [n][25]: relu(z), or a'(l) of "training the pilot's
     * tail, dropout" where a site is on; valid with or without dropout */
    TRS_TRAIN_DBG_A1 = 36, TRS_TRAIN_DBG_A2 = 37, TRS_TRAIN_DBG_A3 = 38
};
void trs_default_train_config(trs_train_config* cfg);
int trs_pilot_train_begin(trs_env* env, const trs_train_config* cfg_or_null, const float* const* h_tail_arrays);
int trs_pilot_train_step(trs_env* env, const uint8_t* d_frames, const float* d_labels, int n, float* d_loss_or_null);
int trs_pilot_train_get(trs_env* env, float* const* h_tail_arrays_out, int* t_out_or_null);
int trs_pilot_train_debug(trs_env* env, int which, float* h_dst, size_t n_floats);
int trs_pilot_train_end(trs_env* env);

/* ---- training the pilot's last convolutions: conv4 .. conv7 (include/trsim_spec.h, "training the pilot's last convolutions") ----
 * Between trs_pilot_train_begin and the session's first step, trs_pilot_train_convs adds conv4 .. conv7 (all 3 x 3, stride 1, valid, 64 or 128 channels)
 * to what the session trains; conv1 .. conv3 stay as loaded.  Every later step also back-propagates from dense1 down to the lowest layer named, on the
 * matrix cores, and moves the named layers by the session's Adam (the same alpha_t and t as the tail).  Without the call a session is the tail's alone.
 *   trs_pilot_train_convs: bit j of conv_mask names conv(4 + j); any non-empty subset.  h_conv_arrays[8]: kernel float[3][3][CIN][COUT] and bias
 *     float[COUT] of conv4 .. conv7 as trs_pilot_load got them, the source of the fp32 masters (the handle keeps binary16 only); the two entries of a
 *     layer whose bit is clear may be NULL.
 *   trs_pilot_train_get_convs: the masters into h_out[0..7] (a NULL entry is skipped); for a layer that is not trained, the arrays as given (untouched
 *     where they were NULL).  Synchronises.
 *   trs_pilot_train_debug_conv: item `which` (TRS_CONV_DBG_*) of conv(4 + layer) after the last step as floats.  Synchronises.
 *   Refusals.  TRS_ERR_STATE: no session, after the session's first step, a second call; get or debug before the call (debug: before a step).
 *     TRS_ERR_ARG: a zero mask, bits above 3, a NULL array of a named layer, an unknown layer or item, a size that is not the item's, delta of a layer
 *     below the lowest trained one. */
enum {
    TRS_CONV_DBG_DELTA = 0,          /* float[n][OH][OW][COUT]: delta(l), the stored binary16 values times 2^-s_l */
    TRS_CONV_DBG_GW = 1,             /* float[3][3][CIN][COUT] (zeros for a layer that is not trained, like the five below) */
    TRS_CONV_DBG_GB = 2,             /* float[COUT] */
    TRS_CONV_DBG_MW = 3, TRS_CONV_DBG_VW = 4,   /* Adam's m and v of the kernel */
    TRS_CONV_DBG_MB = 5, TRS_CONV_DBG_VB = 6,   /* and of the bias */
    TRS_CONV_DBG_SCALE_EXP = 7,      /* 1 float: the exponent s_l of the layer's scale */
    TRS_CONV_DBG_PACK = 8            /* float[3][3][CIN][COUT]: the binary16 copy the forward kernels read, widened, in Keras layout */
};
int trs_pilot_train_convs(trs_env* env, uint32_t conv_mask, const float* const* h_conv_arrays);
int trs_pilot_train_get_convs(trs_env* env, float* const* h_out);
int trs_pilot_train_debug_conv(trs_env* env, int layer, int which, float* h_dst, size_t n_floats);

/* ---- training with dropout behind conv7 (include/trsim_spec.h, "training the pilot's tail, dropout") ----
 * The reference's trainer puts Dropout(0.1) behind every convolution and every hidden dense layer (components/keras_train.py:131-164).  Between
 * trs_pilot_train_begin and the session's first step, trs_pilot_train_dropout switches training-mode dropout on at the four sites the session owns:
 * bit 0 of `sites` conv7's output x7 (the flatten dense1 reads), bits 1 .. 3 relu(z1), relu(z2), relu(z3).  The draws are keyed integers of (seed, the
 * session's step count, site, the frame's slot in the batch, the unit), so a host restates every mask without a GPU (trs_train_dropout_keep).  out, the
 * loss and every gradient of a step are those of the dropped network; inference never drops (trs_pilot_forward, trs_pilot_act, trs_step_pilot,
 * trs_step_dagger are untouched).  The sites behind conv1 .. conv6 stay out: they lie inside the forward kernels that also drive.
 *   trs_pilot_train_dropout: cfg NULL: the defaults.  rate 0, a clear site bit or no call: that site computes what it computed without this section, bit
 *     for bit, by the same kernels.
 *   trs_train_dropout_keep: h_keep[i][k] = 1 when unit k < width of frame slot i < n is kept at step t >= 1 (the first step of a session is 1) at `site`,
 *     else 0; cfg's sites are not consulted.  Host arithmetic only: no handle, no GPU work; the sibling of trs_loader_order and trs_loader_augment.
 *   Refusals.  trs_pilot_train_dropout: TRS_ERR_STATE without a session, after the session's first step, on a second call; TRS_ERR_ARG for a struct_size
 *     mismatch, a rate that is NaN or outside [0, 1), sites with bits above 3.  trs_train_dropout_keep: TRS_ERR_ARG for the config, t < 1, a site outside
 *     0..3, a negative n or width, a NULL h_keep. */
typedef struct trs_dropout_config {
    uint32_t struct_size;
    float    rate;                   /* 0.1: Dropout(0.1); the effective rate is floor(rate 65536) / 65536 */
    uint32_t sites;                  /* 0xF: bit 0 = x7, bits 1..3 = relu(z1) .. relu(z3) */
    uint64_t seed;                   /* 0 (at offset 16: four bytes of padding before it) */
} trs_dropout_config;
void trs_default_dropout_config(trs_dropout_config* cfg);
int trs_pilot_train_dropout(trs_env* env, const trs_dropout_config* cfg_or_null);
int trs_train_dropout_keep(const trs_dropout_config* cfg_or_null, int64_t t, int site, int n, int64_t width, uint8_t* h_keep);

/* ---- training the speed-as-feature pilot: side branch and tail (include/trsim_spec.h, "training the pilot's tail, side branch") ----
 * cnn_2d_speed_as_feature (28 arrays) feeds speed / 20 through feature1 -> feature2 -> feature3 (1 -> 4 -> 8 -> 16, ReLU) and concatenates the result
 * behind the flatten in front of dense1 (components/keras_train.py:127-174,390-392).  The _ex entry points open the session of either trained model type;
 * its 14 trained arrays are arrays 14 .. 27 of trs_pilot_load's list: dense1 (kernel float[F + 16][100]) .. output_layer, then feature1 .. feature3.  Bits
 * 4 .. 6 of trs_train_config.train_mask name feature1 .. feature3 (rows F .. F + 15 of dense1's kernel move with dense1, bit 0); cfg NULL trains all seven
 * layers.  trs_pilot_train_convs, trs_pilot_train_dropout (site 0 masks x7 alone: the concatenation lies behind that Dropout; the feature layers have
 * none), trs_pilot_train_debug, trs_pilot_train_end and the conv getters serve either session.  cnn_2d_full_house (42 arrays) stays refused.
 *   trs_pilot_train_begin_ex: n_arrays = 8 with a 22-array pilot is trs_pilot_train_begin; n_arrays = 14 with a 28-array pilot opens the side session.
 *     Only h_arrays[0], dense1's whole kernel as trs_pilot_load got it, is read from the host; the rest come from the device.
 *   trs_pilot_train_step_ex: d_features float[n][1], speed / 20 per frame as trs_sample_batch writes it for TRS_LOADER_SPEED_FEATURE; required for a
 *     28-array session, ignored for a 22-array one (where the call is trs_pilot_train_step).
 *   trs_pilot_train_get_ex: the 8 or 14 masters (a NULL entry is skipped) and the step count; synchronises.
 *   trs_pilot_train_debug_side: item `which` (TRS_TRAIN_SIDE_*) of the last step of a 28-array session as floats.  Synchronises.
 *   Refusals.  TRS_ERR_LIMIT: a 42-array pilot.  TRS_ERR_ARG: n_arrays that is neither 8 nor 14 or does not match the loaded pilot; the config (bits beyond 6,
 *     or beyond 3 for 8 arrays); a NULL dense1 kernel; NULL d_features on a 28-array session; trs_pilot_train_step or trs_pilot_train_get on a 28-array
 *     session (use _ex); an unknown item or a size that is not the item's.  TRS_ERR_STATE: trs_pilot_train_debug_side on a 22-array session, and as above. */
enum {
    TRS_TRAIN_SIDE_FIN = 0,          /* float[n][1]: the feature as the step read it */
    TRS_TRAIN_SIDE_Y1, TRS_TRAIN_SIDE_Y2, TRS_TRAIN_SIDE_Y3,       /* the branch's activations (behind the ReLU) [n][4], [n][8], [n][16] */
    TRS_TRAIN_SIDE_DY1, TRS_TRAIN_SIDE_DY2, TRS_TRAIN_SIDE_DY3,    /* the loss's gradient by the branch's pre-activations [n][4], [n][8], [n][16] */
    /* + j (0..6): the side arrays W1Y float[16][100] (rows F .. F + 15 of dense1's kernel), feature1's kernel [1][4] and bias, feature2's [4][8] and bias,
     * feature3's [8][16] and bias */
    TRS_TRAIN_SIDE_G = 8,            /* the gradient of side array j */
    TRS_TRAIN_SIDE_M = 16,           /* Adam's m */
    TRS_TRAIN_SIDE_V = 24            /* Adam's v */
};
int trs_pilot_train_begin_ex(trs_env* env, const trs_train_config* cfg_or_null, const float* const* h_arrays, int n_arrays);
int trs_pilot_train_step_ex(trs_env* env, const uint8_t* d_frames, const float* d_features, const float* d_labels, int n, float* d_loss_or_null);
int trs_pilot_train_get_ex(trs_env* env, float* const* h_arrays_out, int n_arrays, int* t_out_or_null);
int trs_pilot_train_debug_side(trs_env* env, int which, float* h_dst, size_t n_floats);

/* ---- multi-GPU: the one exchange (north_star: "a single RCCL all-gather over xGMI of episode returns") ----
 * One process (or thread) per GPU owns one handle = one shard of envs; shards never exchange state.  The reference has no
 * distributed layer at all; this replaces what a user would otherwise script around N copies of manage.py.
 * Rank 0 obtains a 128-byte id and hands it to the other ranks over any host channel (file, environment, socket,
 * torch.distributed store); every rank then calls trs_comm_init (collective).  world == 1 needs no id (with one, the RCCL path
 * itself runs).  RCCL is bound at run time: libtrsim.so does not link against it. */
#define TRS_COMM_ID_BYTES 128
int trs_comm_get_unique_id(void* id_out_128);
int trs_comm_init(trs_env* env, int rank, int world, const void* unique_id_128_or_null);
int trs_comm_destroy(trs_env* env);
/* All ranks receive 'ep_return' of every env of every shard, ordered by rank (= by global env id when shards own contiguous
 * ranges): ncclAllGather of n_envs floats per rank on the handle's stream, behind the steps queued so far.  *d_out_all (may be
 * NULL) receives the handle-owned device buffer float[world * n_envs]; h_out_all (may be NULL) is filled and the call then
 * synchronises.  Latency-bound (4 B per env): issue it per reporting interval, never per step. */
int trs_allgather_returns(trs_env* env, const float** d_out_all, float* h_out_all);

/* ---- ordering against the caller's own HIP streams ----
 * The handle works on its own non-blocking stream.  trs_stream_wait_external: work queued on the handle after this call waits
 * for everything queued so far on `hip_stream` (the producer of device-resident controls, e.g. a policy on torch's stream).
 * trs_stream_signal_external: everything queued on `hip_stream` after this call waits for the handle's work so far (a consumer
 * of device-resident frames / telemetry).  Launch mode: event waits, no host synchronisation.  Resident mode: the host waits
 * (steps are posted by the host; completion is a flag in host memory).  Note that 'cam/img' alternates between two buffers:
 * the frame of step s stays intact while step s + 1 renders, and is overwritten by step s + 2. */
int trs_stream_wait_external(trs_env* env, void* hip_stream);
int trs_stream_signal_external(trs_env* env, void* hip_stream);

/* ---- device-resident part graphs: buffers and small uploads without a framework ----
 * trs_scratch: a handle-owned device buffer per slot (0..31), grown on demand (contents undefined after growth), freed by
 * trs_destroy — where a host-side part keeps 'ai/steering' etc. between parts.  trs_upload: host -> device on the handle's
 * stream (per-car modes, joystick values); returns once the source may be reused.  trs_counters: bytes the library itself has
 * copied device -> host [0] and host -> device [1] since trs_create (tests assert that a device-resident loop copies no frames). */
int trs_scratch(trs_env* env, int slot, size_t bytes, void** d_out);
int trs_upload(trs_env* env, void* d_dst, const void* h_src, size_t bytes);
int trs_counters(trs_env* env, uint64_t out[4]);

/* stream control + device-side timing (HIP events on the handle's stream) */
int trs_sync(trs_env* env);
int trs_event_record(trs_env* env, int slot);                 /* slot 0..7 */
int trs_event_elapsed_ms(trs_env* env, int slot_a, int slot_b, float* ms_out);
int trs_device_count(int* out);

const char* trs_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TRSIM_H */
