// trsim_hip.hip — the core of libtrsim.so for gfx950 (MI355X, CDNA4): the handle behind `trs_env*` from creation to destruction, the kernels that advance
// and render the envs, and the entry points of include/trsim.h that go with them.  What lives here:
//   kernels      trs_step_kernel<DEPTH, DYN, HILLS, LENS, LIGHT> (camera on: ONE launch per env step on ONE stream; 768-thread workgroups own a contiguous
//                range of envs and are wave-specialised — a physics team of one wave per env, a raster team of 8 waves; the variants that are built:
//                trsim_plan.hpp), trs_physics_kernel (camera off: the same wave-per-env routine, K steps per launch) and
//                trs_locate_kernel (batched LocationTracker).  Their
//                device-side pieces — the spec's arithmetic, the nearest-point search, the raster walk — are in trsim_device.hpp.
//   host         the step dispatch (step_call: posted to the resident worker or launched), create / destroy, reset, pose, locate, state, fetch, sync, events,
//                scratch, and the internal accessors the other translation units reach the handle through (trsim_internal.hpp, trsim_env.hpp).
// The rest of the ABI lives in translation units of its own:
//   trsim_scene.hip    what a handle renders: track loading, the lens camera, scene lighting, the palette upload with the static frame filter
//                      (trs_set_frame_filter); trsim_scene.hpp, host only, decides and lays out what is uploaded; this unit gives it track_kernel_attributes
//   trsim_image.hip    trs_preprocess (trim, colour masks, dynamic brightness, Canny) and trs_normalize, kernels and host
//   trsim_control.hip  trs_driver_assist and trs_control_mux, kernels and host
//   trsim_resident.hip the resident worker (trs_set_step_mode)            trsim_pilot.hip  the pilot network and trs_step_pilot
//   trsim_jpeg.hip / trsim_jpeg_decode.hip  the tub image codec           trsim_comm.hip   the RCCL communicator
//   trsim_jpeg_codec.hip  the camera codec (trs_jpeg_roundtrip, trs_set_camera_codec)
//   trsim_latency.hip  observation latency (trs_set_latency): trs_obs_kernel, the launch behind every step while one is set, and the handle's ObsHistory
//   trsim_filter.hpp   host only: the static colour filter of ONE colour, OpenCV's reciprocal tables, the check of a trs_pre_config
//
// Inside a multi-step call the raster team renders step t-1 while the physics team computes step t; the host opens the call with a physics-only launch
// and closes it with a raster-only launch (the lag never leaves the call).  A single-step call is one launch: the raster team writes the rows that need
// no pose (sky, far ground) and then waits per env for the physics team's progress counter.  All LDS staging is LDS-DMA before one barrier.
// Rejected on measurements: all-wave fused phases; two kernels on three streams + hipGraph.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (spec rule R1: no implicit FMA contraction).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/trsim.h"
#include "../../include/trsim_spec.h"
#include "trsim_device.hpp"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"
#include "trsim_tables.hpp"

using trsim::Controls;   // the controls of a step call and their slices (trsim_plan.hpp)
namespace {



#ifndef TRS_STAMPS
#define TRS_STAMPS 0   /* 1 = diagnostic build: s_memtime stamps per phase into stats[8..] (scripts/stamps.sh), never shipped */
#endif
#if TRS_STAMPS
#define STAMP(slot)                                                                                         \
    do {                                                                                                    \
        if (blockIdx.x == 7 && (threadIdx.x == 0 || threadIdx.x == kRasterStampThread)) {                                                   \
            unsigned long long _t;                                                                          \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                      \
            STAMP_STATS[8 + (threadIdx.x ? 24 : 0) + (slot)] = _t;                                                      \
        }                                                                                                   \
    } while (0)
#else
#define STAMP(slot) do { } while (0)
#endif


#undef STAMP_STATS
#define STAMP_STATS sp.ra.stats
// ---------------------------------------------------------------------------------------------
// Fused, wave-specialised step kernel (camera on).  One launch per env step, one stream.
//   raster team  = waves 0..7  (512 threads): rasterises the frame of camera-ring slot `r_slot`
//   physics team = waves 8..11 (one wave per env, no workgroup barriers): advances the envs one step and
//                  writes their camera parameters to ring slot `p_slot`
//   seq = 1  (single-step call): raster waits for this launch's physics and renders the SAME step
//   seq = 0  (inside a multi-step call): raster renders the PREVIOUS step while physics computes the next one;
//            the host issues a physics-only first launch and a raster-only last launch, so the lag never
//            leaves the call.

struct SParams {
    PParams ph;                         // physics side (blob = px|py|pz|tan image; cam = ring base)
    RParams ra;                         // raster side
    uint8_t* img0; uint8_t* img1;       // frame of absolute step s goes to img[s & 1]
    float* dep0; float* dep1;           // z-depth frames, same double buffering (NULL unless cfg.depth)
    int n_phys;                         // physics steps this launch advances (0 = raster-only flush)
    int r_first, r_last;                // raster renders launch-local steps r_first..r_last; -1 = the step before this
                                        // launch (camera parameters from the global ring, written by the previous launch)
    unsigned step_base;                 // absolute index of this launch's physics step 0
    int lds_off_phys, lds_off_cam, lds_off_prog, cam_stride;   // LDS: physics image, float4 lcam[n_phys][cam_stride], int pprog[cam_stride]
    int skip_uniform;                   // bit b: frame buffer b (steps with index & 1 == b) already holds this palette's uniform rows (sky, beyond the far plane: they
                                        // depend on neither the pose nor the step) of every env — an earlier step wrote them and nothing has touched them since: only the
                                        // rows that see the track are written.  Every step path gets it from the handle's UniformRows (trsim_plan.hpp), launch_step here.
    FParams fp;
};

// Physics-only envs (BASELINE config 2): the same barrier-free wave-per-env routine, 4 envs per 256-thread workgroup,
// K steps per launch.  The track image is staged once per launch; nothing is synchronised after that.

__global__ __launch_bounds__(kPhysBlock) void trs_physics_kernel(const PParams p)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the track image goes global -> LDS by LDS-DMA (1 KB per wave instruction, no registers, no ds_write pass)
    stage_lds_dma(p.blob, p.blob_bytes, (unsigned)(uintptr_t)smem, wave, kPhysBlock / 64, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float4* const lsink = reinterpret_cast<float4*>(smem + p.off_scratch);          // per-wave sinks for the camera hand-off slots
    int* const psink = reinterpret_cast<int*>(smem + p.off_scratch + (kPhysBlock / 64) * 16);
    __syncthreads();
    const int e = blockIdx.x * (kPhysBlock / 64) + wave;
    if (e >= p.n_envs) return;
    EnvRegs st;
    env_load(p, e, st);
    for (int k = 0; k < p.n_steps; ++k)
        env_step<true>(p, smem, e, st, p.step_off + (uint32_t)k, k, p.cam, &lsink[wave], &psink[wave], lane);   // (no raster wave beside this one: the select forms, see spec_sincos_sel)
    env_store(p, e, st, lane);
}

// The pose of env j's frame of step sidx (ring: lcam[step][cam_stride], prev: the poses of the step before the launch, staged in the prologue): any step of
// the launch is there once the physics team has finished it for the env (pprog).  The view pitch of a track with elevation lies the same way (HILLS).
template <typename T>
__device__ __forceinline__ T pose_of(const int* pprog, const T* ring, const T* prev, int cam_stride, int sidx, int j)
{
    if (sidx < 0) return prev[j];
    while (__hip_atomic_load(&pprog[j], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < sidx + 1) __builtin_amdgcn_s_sleep(2);
    return ring[sidx * cam_stride + j];
}

template <bool DEPTH, bool DYN, bool HILLS = false, bool LENS = false, bool LIGHT = false>   // HILLS: a track with elevation (its own instantiations: the flat kernels' loops do not change for it);
__global__ __launch_bounds__(kBlock) void trs_step_kernel(const SParams sp)           // LENS: the lens camera on a flat track (likewise); LIGHT: scene lighting (flat or HILLS)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const bool raster_team = tid < kRasterThreads;
    const RParams& p = sp.ra;
    const unsigned lds0 = (unsigned)(uintptr_t)smem;        // LDS byte address of the dynamic segment
    if (lds0 != 0u) {                                       // the map addressing below assumes LDS offset 0 (no static __shared__ in this kernel:
        if (tid == 0 && blockIdx.x == 0) {                  // tests/test_build_lint.py checks .group_segment_fixed_size == 0); refusing is LOUD:
            atomicAdd(&p.stats[2], 1ull);                   // every later synchronisation of the handle fails (trsim::check_fault)
            __hip_atomic_store(p.fault, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    STAMP(0);
    const int e_begin = blockIdx.x * p.envs_per_wg;
    const int e_end = min(e_begin + p.envs_per_wg, p.n_envs);
    float4* const lcam = reinterpret_cast<float4*>(smem + sp.lds_off_cam);     // [n_phys][cam_stride]
    int* const pprog = reinterpret_cast<int*>(smem + sp.lds_off_prog);         // [cam_stride] physics steps finished per env
    const bool rendering = sp.r_last >= sp.r_first;
    for (int j = tid; j < sp.cam_stride; j += kBlock) pprog[j] = 0;
    // behind the progress counters (step_lds_layout, the layout the host's launch_step sized this launch by): tracks with elevation keep float lpitch[n_phys + 1][cam_stride]
    // (view pitch per step and env), then the batch's row tables and the raster team's barrier counter; the block of constants sits behind the raster image in memory
    const StepLds lds = step_lds_behind(sp.lds_off_prog, sp.cam_stride, p.H, variant_bits(DEPTH, DYN, HILLS, LENS, LIGHT), sp.n_phys);
    const int lds_off_pitch = lds.pitch, lds_off_hill = lds.hill;
    float* const lpitch = reinterpret_cast<float*>(smem + lds_off_pitch);
    int* const hbar = reinterpret_cast<int*>(smem + lds_off_hill + hill_batch(p.H) * hill_table_bytes(p.H));
    const trsim::HillBlock* const hill = HILLS ? hill_block(p) : nullptr;
    if (HILLS && tid == 0) *hbar = 0;
    // scene lighting (LIGHT): the workgroup's lighting parameters float[cam_stride][8], read once per launch (a call's frames all use the values as they stood when it
    // started), then the raster waves' lit palettes (light_wave_palette) — behind the row tables of a track with elevation, else where those would sit
    const int lds_off_light = lds.light;
    float* const llight = reinterpret_cast<float*>(smem + lds_off_light);
    const unsigned lds_off_lpal = (unsigned)lds_off_light + (unsigned)sp.cam_stride * 32u;
    const int lfilt = LIGHT ? hill_block(p)->filt : 0;   // (once per kernel)
    if constexpr (DYN) {
        if (tid < 32) reinterpret_cast<int*>(smem + sp.fp.lds_off + 4 * p.H * 16)[tid] = 0;   // esum[2][4][3], dbar
        dyn_stage_tables(smem, sp.fp, p.H, tid, kBlock, reinterpret_cast<const uint32_t*>(p.blob + p.off_pal));                   // OpenCV's reciprocals + the in-range byte masks (behind the prologue's barrier)
    }
    // ---- prologue: everything is staged global -> LDS by LDS-DMA (global_load_lds_dwordx4: one wave instruction moves
    // 64 lanes x 16 B = 1 KB, lane-linear, no registers and no ds_write pass), all requests are in flight together and
    // one workgroup barrier closes the stage.  Raster waves: the class map + row tables (one linear image at LDS offset
    // 0); physics waves: the track image.  The previous step's poses ride along through a register. ----
    const int pw = wave - kRasterThreads / 64;                                // physics wave index (< 0 for the raster team)
    float4* const lcam_prev = lcam + max(sp.n_phys, 1) * sp.cam_stride;       // [cam_stride] poses of step_base - 1
    {
        const bool has_c = raster_team && rendering && sp.r_first < 0 && tid < e_end - e_begin;
        float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4* const cam_prev = sp.ph.cam + (size_t)((sp.step_base - 1u) & (kRing - 1)) * sp.ph.n_envs;
        if (has_c) cv = cam_prev[e_begin + tid];
        if (raster_team) {
            if (rendering) stage_lds_dma(p.blob, p.blob_bytes, 0u, wave, kRasterThreads / 64, lane);
        } else if (sp.n_phys > 0) {
            stage_lds_dma(sp.ph.blob, sp.ph.blob_bytes, (unsigned)sp.lds_off_phys, pw, kPhysWaves, lane);
        }
        if (LENS && raster_team && rendering) lens_stage_palette(p, (unsigned)lds_off_hill, wave, lane);   // the lens palette sits where a hilly track keeps its row tables
        if (LIGHT && raster_team && rendering) {
            const float* const lsrc = hill_block(p)->light + (size_t)e_begin * 8;
            for (int j = tid; j < (e_end - e_begin) * 8; j += kRasterThreads) llight[j] = lsrc[j];
        }
        if (has_c) lcam_prev[tid] = cv;
        if (raster_team && rendering && sp.r_first < 0)
            for (int j = tid + kRasterThreads; j < e_end - e_begin; j += kRasterThreads) lcam_prev[j] = cam_prev[e_begin + j];
        if (HILLS && raster_team && rendering && sp.r_first < 0) {             // ... and its view pitch (a track with elevation)
            const float* const pitch_prev = hill->cam_pitch + (size_t)((sp.step_base - 1u) & (kRing - 1)) * sp.ph.n_envs;
            for (int j = tid; j < e_end - e_begin; j += kRasterThreads) lpitch[max(sp.n_phys, 1) * sp.cam_stride + j] = pitch_prev[e_begin + j];
        }
    }
    STAMP(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                          // this wave's DMA pieces have landed
    __syncthreads();
    STAMP(2);

    // ---- physics team: one wave per env, no workgroup synchronisation; runs up to n_phys steps ahead of the raster ----
    if (!raster_team) {
        if (sp.n_phys <= 0) return;
        float4* const ring = sp.ph.cam;
        const unsigned char* const lphys = smem + sp.lds_off_phys;
        if (p.envs_per_wg <= kPhysWaves) {
            // at most one env per physics wave: its state lives in registers for all the steps of this launch
            const int e = e_begin + pw;
            if (e < e_end) {
                const int j = e - e_begin;
                EnvRegs st;
                env_load(sp.ph, e, st);
                for (int k = 0; k < sp.n_phys; ++k) {
                    const uint32_t t = sp.step_base + (uint32_t)k;
                    env_step(sp.ph, lphys, e, st, t, k, ring + (size_t)(t & (kRing - 1)) * sp.ph.n_envs, &lcam[k * sp.cam_stride + j], &pprog[j], lane,
                             hill, HILLS ? &lpitch[k * sp.cam_stride + j] : nullptr);
                }
                env_store(sp.ph, e, st, lane);
            }
        } else {
            // several envs per wave: step-major order keeps every env's raster fed; state goes through L2 between steps
            for (int k = 0; k < sp.n_phys; ++k) {
                const uint32_t t = sp.step_base + (uint32_t)k;
                float4* const cam_out = ring + (size_t)(t & (kRing - 1)) * sp.ph.n_envs;
                for (int e = e_begin + pw; e < e_end; e += kPhysWaves) {
                    const int j = e - e_begin;
                    EnvRegs st;
                    env_load(sp.ph, e, st);
                    env_step(sp.ph, lphys, e, st, t, k, cam_out, &lcam[k * sp.cam_stride + j], &pprog[j], lane,
                             hill, HILLS ? &lpitch[k * sp.cam_stride + j] : nullptr);
                    env_store(sp.ph, e, st, lane);
                }
                if (sp.n_phys > 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // stores have reached L2 before the next step reloads them
            }
        }
        STAMP(3);
        return;
    }
    if (!rendering) return;

    // ---- raster team ----
    // A thread owns one 4-pixel column group (u0 fixed) and walks image rows, so the pixel-centre offsets uf are
    // loop constants.  The first `uni_rows` rows (sky, ground beyond the far plane) have four equal class colours: they
    // need neither the class map nor the camera pose and are written FIRST, while the map is still on its way and (in a
    // single-step call) while the physics team integrates.  Per pixel of the other rows: 1 packed fma (gx,gz), 2
    // saturating converts + 2 min (= floor + clamp), 3 address ops, 1 LDS map read, shift + bit-field extract, 1 palette
    // address op, 1 LDS palette read.
    const RasterThread rth = raster_thread(p, smem, tid);
    [[maybe_unused]] const f2v* const lrow = rth.lrow;
    [[maybe_unused]] const float* const lrowdepth = rth.lrowdepth;
    [[maybe_unused]] const unsigned gwm1 = rth.gwm1, ghm1 = rth.ghm1, pitch = rth.pitch;
    [[maybe_unused]] const int cg = rth.cg, vstart = rth.vstart, col_off = rth.col_off;
    [[maybe_unused]] const f2v ufa = rth.ufa, ufb = rth.ufb, ufc = rth.ufc, ufd = rth.ufd;
    [[maybe_unused]] const size_t row_bytes = (size_t)rth.row_bytes;
    trsim::LensBlock lb{};
    LensCacheStep<DEPTH> lcache;
    if constexpr (LENS) {
        lb = *lens_block(p);   // (uniform address: scalar loads)
        lens_cache_load(p, rth, lb, lcache);                   // this thread's table entries, once for every frame of the kernel
    }
    for (int sidx = sp.r_first; sidx <= sp.r_last; ++sidx) {
    const unsigned abs_step = sp.step_base + (unsigned)sidx;                  // sidx = -1: the step before this launch
    uint8_t* const img = (abs_step & 1u) ? sp.img1 : sp.img0;
    float* const dep = (abs_step & 1u) ? sp.dep1 : sp.dep0;
    // (Writing the uniform rows of ALL the workgroup's envs first — so that more bytes are in flight while a single-step call
    // waits for its poses — was measured in round 2: the single-step call did not get shorter (16.7 us both ways) and the
    // pipelined launch got 6 % LONGER (13.5 -> 14.4 us at 1024 envs: the frames are then written in two sweeps over all envs
    // instead of one contiguous 57.6 KB stream per env).  Env by env it is.)
    for (int e = e_begin; e < e_end; ++e) {
        if constexpr (HILLS) {
            // ---- a track with elevation: the envs go through in batches — poses and view pitches of the batch, its row tables between two team barriers
            // (trsim_device.hpp, hill_batch_build), then the same row loop on each env's table
            const int HB = hill_batch(p.H);
            if ((e - e_begin) % HB != 0) continue;                            // the batch leader's iteration does the work
            const int nbatch = (e_end - e_begin + HB - 1) / HB;
            const int it = (sidx - sp.r_first) * nbatch + (e - e_begin) / HB; // batches so far (the same in every wave)
            const int nb = min(HB, e_end - e);
            float4 cams[kHillBatchMax]; float Pv[kHillBatchMax];
#pragma unroll
            for (int bi = 0; bi < kHillBatchMax; ++bi) {
                cams[bi] = make_float4(0.f, 0.f, 0.f, 1.f); Pv[bi] = 0.f;
                if (bi < nb) {
                    const int j = e - e_begin + bi;
                    cams[bi] = pose_of(pprog, lcam, lcam_prev, sp.cam_stride, sidx, j);
                    Pv[bi] = sidx < 0 ? lpitch[max(sp.n_phys, 1) * sp.cam_stride + j] : lpitch[sidx * sp.cam_stride + j];   // (its view pitch lies the same way, behind the same wait)
                }
            }
            auto never = [](bool) { return false; };                          // (a launch has no abort: every raster wave arrives)
            (void)hill_batch_build(p, smem, (unsigned)lds_off_hill, Pv, nb, hbar, it * 2 * (kRasterThreads / 64), tid, lane, never, LIGHT ? llight + (e - e_begin) * 8 : nullptr);
#pragma unroll
            for (int bi = 0; bi < kHillBatchMax; ++bi)
                if (bi < nb)
                    raster_hill_frame<DEPTH>(p, rth, smem, (unsigned)lds_off_hill, bi, hbar, it * 2 * (kRasterThreads / 64), frame_desc<DEPTH>(p, img, dep, e + bi), cams[bi]);
            continue;
        }
        if constexpr (LENS) {
            // ---- the lens camera: every row of the frame from the per-pixel table (no uniform rows: sky and far pixels follow the lens per pixel)
            raster_lens_frame(p, rth, lb, lcache, (unsigned)lds_off_hill, frame_desc<DEPTH>(p, img, dep, e), pose_of(pprog, lcam, lcam_prev, sp.cam_stride, sidx, e - e_begin));
            continue;
        }
        if constexpr (DYN) {
            // ---- dynamic brightness behind the rasteriser: the frame's own mean over rows [w0, w1) only needs the class of
            // every pixel there, so, for up to kDynBatch envs at a time: (A) classify those rows once (classes kept in
            // registers), sum the RAW colours per channel, reduce over the team; (B) every thread filters entries of the
            // per-env palettes with each frame's delta; (C) shade all rows from those palettes.  No extra pass over HBM, each
            // pixel classified once, two team barriers per batch.
            if ((e - e_begin) % kDynBatch != 0) continue;                     // the batch leader does the work
            const int nbatch = (e_end - e_begin + kDynBatch - 1) / kDynBatch;
            const int it = (sidx - sp.r_first) * nbatch + (e - e_begin) / kDynBatch;   // batches so far (same in every wave)
            float4 cams[kDynBatch];
#pragma unroll
            for (int bi = 0; bi < kDynBatch; ++bi) {
                const int eb = e + bi;
                cams[bi] = make_float4(0.f, 0.f, 0.f, 1.f);
                if (eb < e_end) cams[bi] = pose_of(pprog, lcam, lcam_prev, sp.cam_stride, sidx, eb - e_begin);
            }
            (void)raster_dyn_batch<DEPTH, LIGHT>(p, sp.fp, rth, smem, cams, min(kDynBatch, e_end - e), img, dep, e, it, tid, lane, [](bool) { return false; },   // a launch has no abort: every raster wave arrives
                                                 LIGHT ? llight + (e - e_begin) * 8 : nullptr, lds_off_lpal);
            continue;
        }
        // rows with four equal class colours need no map lookup and no pose: they are written first, and in a single-step
        // call while the physics team still integrates
        const FrameDesc fd = frame_desc<DEPTH>(p, img, dep, e);
        RasterThread rl = rth;                                                // (LIGHT: shaded from this wave's lit copy of the palette)
        if constexpr (LIGHT && !HILLS && !DYN) rl.pal_off = light_wave_palette(p, lds_off_lpal, llight + (e - e_begin) * 8, lfilt, wave, lane);
        if (!((sp.skip_uniform >> (abs_step & 1u)) & 1)) raster_uniform_rows<DEPTH>(p, rl, fd);
        // -- rows that see the track
        raster_ground_rows<DEPTH>(p, rl, fd, pose_of(pprog, lcam, lcam_prev, sp.cam_stride, sidx, e - e_begin));
    }
    }
    STAMP(5);
}

// trs_step_kernel by variant bits, nullptr where none is built: the launch (launch_step) and the LDS attribute of every instantiation (track_kernel_attributes) go through it
using StepKernel = void (*)(SParams);
template <Variant V> StepKernel step_kernel_of()
{
    if constexpr (variant_built(V)) return &trs_step_kernel<(V & kVDepth) != 0, (V & kVDyn) != 0, (V & kVHills) != 0, (V & kVLens) != 0, (V & kVLight) != 0>;
    else return nullptr;
}
template <Variant... V> std::array<StepKernel, kVariants> step_kernel_table(std::integer_sequence<Variant, V...>) { return {step_kernel_of<V>()...}; }
const std::array<StepKernel, kVariants> kStepKernels = step_kernel_table(std::make_integer_sequence<Variant, kVariants>{});

#undef STAMP_STATS

// Batched LocationTracker.__find_closest (components/track_data_process.py:89-101): one wave per query,
// track staged in LDS once per workgroup, queries grid-strided.
__global__ __launch_bounds__(kLocBlock) void trs_locate_kernel(const unsigned char* blob, int stage_bytes, const NearParams g,
                                                               const double* q, int nq, int32_t* out)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const uint4* src = reinterpret_cast<const uint4*>(blob);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (int i = tid; i < (stage_bytes >> 4); i += kLocBlock) dst[i] = src[i];
    }
    __syncthreads();
    constexpr int kW = kLocBlock / 64;
    for (int qi = blockIdx.x * kW + wave; qi < nq; qi += gridDim.x * kW) {
        double best;
        int idx;
        wave_nearest(g, smem, q[3 * qi], q[3 * qi + 1], q[3 * qi + 2], lane, best, idx);
        if (lane == 0) out[qi] = idx;
    }
}

// ---------------------------------------------------------------------------------------------
// host side

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }


// the frame buffers written by the last step (nullptr without a camera / without cfg.depth)
// (with an observation latency set: the ring slot of the last step — every step then renders into the ring, trsim_latency.hpp, ObsHistory)
const uint8_t* latest_frame(const trs_env* e)
{
    if (!e->cfg.render) return nullptr;
    return e->obs.on() ? e->obs.frame(e->obs.slot_of_last(e->step_count)) : e->img[(e->step_count + 1) & 1].get();
}
const float* latest_depth(const trs_env* e)
{
    if (!(e->cfg.render && e->cfg.depth)) return nullptr;
    return e->obs.on() ? e->obs.depth(e->obs.slot_of_last(e->step_count)) : e->depth[(e->step_count + 1) & 1].get();
}

int grid_of(const trs_env* e) { return (e->n + e->pp.envs_per_wg - 1) / e->pp.envs_per_wg; }
int steps_that_fit(const trs_env* e, Variant v, int lds_step) { return trsim::steps_that_fit(lds_step, e->pp.envs_per_wg, e->H, e->W, v); }

// the handle's stream is idle: a resident worker (trs_set_step_mode) is asked to leave first — it owns the stream while it runs
int sync_all(trs_env* e)
{
    if (e->res) { int rc = trsim::resident_quiesce(e); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(e->sP));
    return trsim::check_fault(e);
}

// anything about to be queued on the handle's stream must not end up behind a resident worker
int quiesce(trs_env* e) { return e->res ? trsim::resident_quiesce(e) : TRS_OK; }

// one launch of the fused step kernel: physics steps [step_base, step_base + n_phys) and the frames of launch-local
// steps r_first..r_last (-1 = step_base - 1, whose camera parameters the previous launch left in the global ring)
int launch_step(trs_env* e, const Controls& c, int n_phys, int r_first, int r_last, uint64_t step_base)
{
    const Variant v = trsim::variant_of(e);
    const StepKernel kernel = kStepKernels[v];
    if (!kernel) return fail(TRS_ERR_STATE, "internal error: no step kernel is built for this combination of camera, track, frame filter and lighting");
    SParams sp;
    sp.ph = e->pp;
    sp.ph.ctl_steer = c.steer; sp.ph.ctl_thr = c.thr; sp.ph.ctl_brk = c.brk; sp.ph.ctl_reset = c.reset; sp.ph.ctl_stride = c.stride;
    sp.ph.synth = c.synth; sp.ph.n_steps = n_phys; sp.ph.write_cam = 1; sp.ph.step_off = (uint32_t)step_base;
    sp.ra = e->rp;
    const bool ring = e->obs.on();                                // an observation latency is set: the one frame of this launch goes to its ring slot
    if (ring) {
        if (n_phys != 1 || r_first != 0 || r_last != 0) return fail(TRS_ERR_STATE, "internal error: a step with an observation latency set is one launch that renders its own frame");
        const int slot = e->obs.slot_of_last(step_base + 1);      // (the step this launch is: counted once it is on the stream)
        sp.img0 = sp.img1 = e->obs.frame(slot);
        sp.dep0 = sp.dep1 = e->cfg.depth ? e->obs.depth(slot) : nullptr;
    } else {
        sp.img0 = e->img[0].get(); sp.img1 = e->img[1].get();
        sp.dep0 = e->depth[0].get(); sp.dep1 = e->depth[1].get();
    }
    sp.n_phys = n_phys; sp.r_first = r_first; sp.r_last = r_last;
    sp.step_base = (unsigned)step_base;
    sp.lds_off_phys = e->lds_off_phys;
    sp.cam_stride = e->pp.envs_per_wg;
    const StepLds lds = step_lds_layout(e->lds_step, sp.cam_stride, e->H, e->W, v, n_phys);   // ring + counters (+ the variant's regions) behind the tables
    sp.lds_off_cam = lds.cam; sp.lds_off_prog = lds.prog;
    // Which frame buffers hold the CURRENT palette's uniform rows for every env (e->uniform_ok, trsim_plan.hpp): the launch skips them there, and the buffers
    // it renders into hold them afterwards — or no longer, after a DYN, LENS or LIGHT frame.
    // A ring slot is never claimed: every step into the ring stores whole frames (the uniform-row skip does not carry over to ring slots).
    sp.skip_uniform = ring ? 0 : (int)e->uniform_ok.skip_mask(v);
    if (!ring && r_first <= r_last) e->uniform_ok.rendered(v, step_base + (uint64_t)(int64_t)r_first, (uint64_t)(r_last - r_first + 1));
    sp.fp = trsim::fparams_of(e, lds.dyn);
    hipLaunchKernelGGL(kernel, dim3(grid_of(e)), dim3(kBlock), lds.total, e->sP, sp);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

// n env steps with a camera, K = steps per launch.  n == 1: one launch, the raster team waits for the physics team
// through the LDS progress counters.  Otherwise a software pipeline over launches: a launch advances K physics steps
// and renders the previous launch's last step plus its own steps 0..K-2; a raster-only launch closes the call, so on
// return state and image both belong to step s0+n-1.  Every launch reads its own slice of the call's controls (Controls::after).
int run_camera_steps(trs_env* e, const Controls& c, int n, int per_launch)
{
    const uint64_t s0 = e->step_count;
    int rc = TRS_OK;
    if (e->obs.on()) {                                       // an observation latency is set: every step is one launch into its ring slot, and trs_obs_kernel behind it
        for (int i = 0; i < n; ++i) {
            if ((rc = launch_step(e, c.after(i), 1, 0, 0, s0 + (uint64_t)i))) return rc;
            e->step_count += 1;
            if ((rc = trsim::launch_obs(e))) return rc;
        }
        return TRS_OK;
    }
    if (n == 1) {
        rc = launch_step(e, c, 1, 0, 0, s0);
    } else {
        const int kmax = std::max(1, std::min(per_launch, steps_that_fit(e, trsim::variant_of(e), e->lds_step)));
        for (int done = 0; done < n && !rc;) {
            const int k = std::min(kmax, n - done);
            rc = launch_step(e, c.after(done), k, done == 0 ? 0 : -1, k - 2, s0 + done);
            done += k;
        }
        if (!rc) rc = launch_step(e, Controls{c.steer, c.thr, c.brk, nullptr, c.synth, c.stride}, 0, -1, -1, s0 + n);   // (no physics step: it reads no controls)
    }
    if (rc) return rc;
    e->step_count += (uint64_t)n;
    return TRS_OK;
}

// one launch of the physics-only kernel: n_steps steps from step index step_off, every step k reading c.after(k) (the kernel strides by itself)
int launch_physics(trs_env* e, const Controls& c, int n_steps, uint64_t step_off)
{
    PParams p = e->pp;
    p.ctl_steer = c.steer; p.ctl_thr = c.thr; p.ctl_brk = c.brk; p.ctl_reset = c.reset; p.ctl_stride = c.stride;
    p.synth = c.synth; p.n_steps = n_steps; p.write_cam = 0; p.step_off = (uint32_t)step_off;
    hipLaunchKernelGGL(trs_physics_kernel, dim3((e->n + kPhysBlock / 64 - 1) / (kPhysBlock / 64)), dim3(kPhysBlock), e->lds_p, e->sP, p);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

// physics-only envs: K steps inside one launch of the physics kernel
int run_physics_steps(trs_env* e, const Controls& c, int n, int per_launch)
{
    if (e->obs.on()) per_launch = 1;                         // an observation latency is set: trs_obs_kernel files every step's telemetry
    for (int done = 0; done < n;) {
        const int now = std::min(per_launch, n - done);
        int rc = launch_physics(e, c.after(done), now, e->step_count);
        if (rc) return rc;
        e->step_count += (uint64_t)now;
        done += now;
        if (e->obs.on() && (rc = trsim::launch_obs(e))) return rc;
    }
    return TRS_OK;
}

// The launch half of every step call, and the whole of the pilot loop's step: n steps by launches on the handle's stream, which the caller has quiesced.
struct PerLaunch { int camera, physics; };                   // steps per launch with a camera / physics-only (trs_step: the whole call / 1)
int launch_steps(trs_env* e, const Controls& c, int n, PerLaunch per) { return e->cfg.render ? run_camera_steps(e, c, n, per.camera) : run_physics_steps(e, c, n, per.physics); }

// The path of every step call behind its argument checks.  In resident mode (tried again when due after a fall-back) the steps are posted to the worker; where
// it falls back in the middle of the call (kResidentFellBack: the first `done` steps are on the stream as launches) the remainder, c.after(done), goes on by launches.
// host (trs_step_host): c holds host arrays; the worker reads them from its pinned staging, launches from the handle's control arrays after an upload.
int step_call(trs_env* e, Controls c, int n_steps, PerLaunch per, bool host = false)
{
    trsim::resident_retry(e);
    if (trsim::resident_on(e)) {
        int done = 0;
        const int rc = host ? trsim::resident_post_host(e, c, n_steps, &done) : trsim::resident_post(e, c, n_steps, &done);
        if (rc != trsim::kResidentFellBack || done == n_steps) return rc < 0 ? rc : TRS_OK;
        c = c.after(done);                                   // the handle went back to launch mode (trs_last_error() says why): the rest of the call by launches
        n_steps -= done;
    }
    { int rq = quiesce(e); if (rq) return rq; }
    if (host) {
        const size_t n = (size_t)e->n;
        e->h2d_bytes += n * 8 + (c.brk ? n * 4 : 0) + (c.reset ? n : 0);
        HIPCHK(hipMemcpyAsync(e->ctl_steer, c.steer, n * 4, hipMemcpyHostToDevice, e->sP));
        HIPCHK(hipMemcpyAsync(e->ctl_thr, c.thr, n * 4, hipMemcpyHostToDevice, e->sP));
        if (c.brk) HIPCHK(hipMemcpyAsync(e->ctl_brk, c.brk, n * 4, hipMemcpyHostToDevice, e->sP));
        if (c.reset) HIPCHK(hipMemcpyAsync(e->ctl_reset, c.reset, n, hipMemcpyHostToDevice, e->sP));
        c = Controls{e->ctl_steer, e->ctl_thr, c.brk ? e->ctl_brk : nullptr, c.reset ? e->ctl_reset : nullptr, 0, 0};
    }
    return launch_steps(e, c, n_steps, per);
}

// The staged fetch behind trs_fetch_outputs and trs_fetch_observation: the items asked for (dst non-null) into the pinned staging by copies on stream
// cs, one synchronisation, then out to the caller's arrays (fetch_layout, trsim_plan.hpp).  fetch_staging comes first: it may have to idle the handle.
struct FetchItem { const void* src; void* dst; size_t bytes; };
int fetch_staging(trs_env* e, size_t img_bytes)
{
    const size_t need = trsim::fetch_reserve(img_bytes, (size_t)e->n);
    if (e->pinned.bytes() >= need) return TRS_OK;
    if (e->pinned.get()) { int rq = sync_all(e); if (rq) return rq; }
    HIPCHK(e->pinned.reserve(need, hipHostMallocDefault));
    return TRS_OK;
}
int staged_fetch(trs_env* e, const FetchItem (&items)[trsim::kFetchItems], hipStream_t cs)
{
    size_t bytes[trsim::kFetchItems];
    for (int i = 0; i < trsim::kFetchItems; ++i) bytes[i] = items[i].dst ? items[i].bytes : 0;
    const trsim::FetchLayout L = trsim::fetch_layout(bytes);
    for (int i = 0; i < trsim::kFetchItems; ++i) {
        if (!bytes[i]) continue;
        HIPCHK(hipMemcpyAsync(e->pinned.get() + L.off[i], items[i].src, bytes[i], hipMemcpyDeviceToHost, cs));
        e->d2h_bytes += bytes[i];
    }
    HIPCHK(hipStreamSynchronize(cs));
    { int rf = trsim::check_fault(e); if (rf) return rf; }
    for (int i = 0; i < trsim::kFetchItems; ++i)
        if (bytes[i]) std::memcpy(items[i].dst, e->pinned.get() + L.off[i], bytes[i]);
    return TRS_OK;
}

}  // namespace

TRS_EXPORT void trs_default_config(trs_config* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->struct_size = (uint32_t)sizeof *c;
    c->n_envs = 1; c->img_h = 120; c->img_w = 160; c->render = 1;
    c->seed = TRS_SYNTH_SEED;
    c->dt = TRS_DEF_DT; c->max_steer = TRS_DEF_MAX_STEER; c->inv_wheelbase = TRS_DEF_INV_WHEELBASE;
    c->accel_max = TRS_DEF_ACCEL_MAX; c->drag_lin = TRS_DEF_DRAG_LIN; c->roll_res = TRS_DEF_ROLL_RES;
    c->brake_max = TRS_DEF_BRAKE_MAX; c->v_max = TRS_DEF_V_MAX; c->v_rev_max = TRS_DEF_V_REV_MAX;
    c->offtrack_cte = TRS_DEF_OFFTRACK_CTE; c->offtrack_penalty = TRS_DEF_OFFTRACK_PENALTY; c->cam_fwd = TRS_DEF_CAM_FWD;
    c->road_half = TRS_DEF_ROAD_HALF; c->edge_half = TRS_DEF_EDGE_HALF; c->centre_half = TRS_DEF_CENTRE_HALF;
    c->dash_period = TRS_DEF_DASH_PERIOD; c->dash_on = TRS_DEF_DASH_ON; c->map_margin = TRS_DEF_MAP_MARGIN;
    c->fov_v_deg = TRS_DEF_FOV_V_DEG; c->cam_h = TRS_DEF_CAM_H; c->cam_pitch_deg = TRS_DEF_CAM_PITCH_DEG; c->z_far = TRS_DEF_Z_FAR;
}

TRS_EXPORT int trs_device_count(int* out)
{
    if (!out) return fail(TRS_ERR_ARG, "null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return TRS_OK;
}

namespace {
// everything trs_create builds; on a failure the caller destroys the half-built handle
int create_impl(const trs_config* cfg, int device, trs_env* e)
{
    e->cfg = *cfg; e->device = device; e->n = cfg->n_envs; e->H = cfg->img_h; e->W = cfg->img_w;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    e->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIPCHK(hipStreamCreateWithFlags(&e->sP, hipStreamNonBlocking));
    for (auto& ev : e->ev) HIPCHK(hipEventCreate(&ev));
    HIPCHK(hipEventCreateWithFlags(&e->ev_order, hipEventDisableTiming));

    // one slab for all per-env arrays: 10 float + 2 int32 state arrays, 3 float + 1 byte control arrays, 2 byte flags
    const size_t n = (size_t)e->n, fa = trsim::align_up(n * 4, 256), ba = trsim::align_up(n, 256);
    const size_t slab_bytes = fa * (10 + 2 + 3) + ba * 3;
    HIPCHK(e->slab.alloc(slab_bytes));
    HIPCHK(hipMemsetAsync(e->slab.get(), 0, slab_bytes, e->sP));
    unsigned char* c = e->slab.get();
    auto takef = [&](float*& ptr) { ptr = reinterpret_cast<float*>(c); c += fa; };
    PParams& k = e->pp;
    takef(k.x); takef(k.y); takef(k.z); takef(k.yaw); takef(k.v); takef(k.speed); takef(k.cte);
    takef(k.ep_return); takef(k.last_return); takef(k.steer_filt);
    k.seg_idx = reinterpret_cast<int32_t*>(c); c += fa;
    k.ep_len = reinterpret_cast<int32_t*>(c); c += fa;
    takef(e->ctl_steer); takef(e->ctl_thr); takef(e->ctl_brk);
    k.done = c; c += ba; k.pending = c; c += ba; e->ctl_reset = c; c += ba;
    HIPCHK(e->stats.alloc(64 * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(e->stats.get(), 0, e->stats.bytes(), e->sP));
    HIPCHK(e->cam.alloc((size_t)kRing * n * sizeof(float4)));
    HIPCHK(hipMemsetAsync(e->cam.get(), 0, e->cam.bytes(), e->sP));
    HIPCHK(e->cam_pitch.alloc((size_t)kRing * n * sizeof(float)));   // the frames' view pitches beside the camera ring (tracks with elevation)
    HIPCHK(hipMemsetAsync(e->cam_pitch.get(), 0, e->cam_pitch.bytes(), e->sP));
    k.stats = e->stats.get(); k.cam = e->cam.get();
    RParams& r = e->rp;
    r.stats = e->stats.get();
    if (cfg->render) {
        e->img_bytes = n * (size_t)e->H * e->W * 3;
        e->uniform_ok.invalidate();                         // fresh buffers hold no frame
        for (int b = 0; b < 2; ++b) {
            HIPCHK(e->img[b].alloc(e->img_bytes));
            HIPCHK(hipMemsetAsync(e->img[b].get(), 0, e->img_bytes, e->sP));
            if (cfg->depth) {
                HIPCHK(e->depth[b].alloc(n * (size_t)e->H * e->W * 4));
                HIPCHK(hipMemsetAsync(e->depth[b].get(), 0, e->depth[b].bytes(), e->sP));
            }
        }
    }
    k.n_envs = e->n; k.env_id_base = cfg->env_id_base;
    k.envs_per_wg = (e->n + e->cu_count - 1) / e->cu_count;
    r.n_envs = e->n; r.envs_per_wg = k.envs_per_wg;
    r.H = e->H; r.W = e->W; r.gpr = e->W / 4; r.gpe = r.gpr * e->H; r.depth = (cfg->render && cfg->depth) ? 1 : 0;
    k.dt = cfg->dt; k.max_steer = cfg->max_steer; k.inv_wheelbase = cfg->inv_wheelbase; k.accel_max = cfg->accel_max;
    k.drag_lin = cfg->drag_lin; k.roll_res = cfg->roll_res; k.brake_max = cfg->brake_max; k.v_max = cfg->v_max;
    k.v_rev_max = cfg->v_rev_max; k.offtrack_cte = cfg->offtrack_cte; k.offtrack_penalty = cfg->offtrack_penalty;
    k.cam_fwd = cfg->cam_fwd; k.auto_reset = cfg->auto_reset; k.seed = cfg->seed;
    if (r.gpr > kBlock) return fail(TRS_ERR_LIMIT, "img_w too large: more 4-pixel groups per row than threads per workgroup");
    if (r.gpr > kRasterThreads) return fail(TRS_ERR_LIMIT, "img_w too large: more 4-pixel groups per row than raster threads");
    r.rows_per_pass = trsim::raster_rows_per_pass(r.gpr);   // raster threads beyond rows_per_pass * gpr idle (32 of 512 at W = 160)
    HIPCHK(e->fault.alloc(64, hipHostMallocMapped | hipHostMallocCoherent));   // kernels report a layout fault here (checked at every synchronisation)
    *e->fault.get() = 0ull;
    k.fault = e->fault.get(); r.fault = e->fault.get();
    HIPCHK(hipStreamSynchronize(e->sP));
    return TRS_OK;
}


}  // namespace

TRS_EXPORT int trs_create(const trs_config* cfg, int device, trs_env** out)
{
    if (!cfg || !out) return fail(TRS_ERR_ARG, "null argument");
    if (cfg->struct_size != sizeof(trs_config)) return fail(TRS_ERR_ARG, "trs_config.struct_size mismatch");
    if (cfg->n_envs < 1 || cfg->img_h < 2 || cfg->img_w < 4 || (cfg->img_w & 3) || cfg->env_id_base < 0)
        return fail(TRS_ERR_ARG, "bad n_envs / image size (img_w must be a multiple of 4)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(TRS_ERR_DEVICE, "no HIP device visible (libtrsim has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(TRS_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    trs_env* e = new (std::nothrow) trs_env();
    if (!e) return fail(TRS_ERR_NOMEM, "out of memory");
    e->device = device;
    const int rc = create_impl(cfg, device, e);
    if (rc) {                                                // keep the message of the failure, not of the clean-up
        const std::string why = g_err;
        (void)trs_destroy(e);
        return fail(rc, why);
    }
    *out = e;
    return TRS_OK;
}

TRS_EXPORT int trs_destroy(trs_env* e)
{
    if (!e) return TRS_OK;
    (void)hipSetDevice(e->device);
    trsim::resident_destroy(e);
    if (e->sP) (void)hipStreamSynchronize(e->sP);
    trsim::comm_destroy(e);
    if (e->ev_order) (void)hipEventDestroy(e->ev_order);
    if (e->pilot) { trs_pilot_free(e->pilot); e->pilot = nullptr; }
    if (e->expert) { trs_expert_free(e->expert); e->expert = nullptr; }
    for (auto& ev : e->ev) if (ev) (void)hipEventDestroy(ev);
    if (e->sP) (void)hipStreamDestroy(e->sP);
    delete e;                                                // the handle's buffers go with it: the stream was idle above
    return TRS_OK;
}

// trs_load_track (trsim_scene.hip) before it commits a track: the kernels may use the LDS the new track needs — and the fused kernel has room for one step
// per launch beside it
int trsim::track_kernel_attributes(const trs_env* e, const trsim::TrackLayout& L, bool hills)
{
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(trs_physics_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, L.p.lds_p));
    // room in the CU's 160 KiB for one step per launch of the camera hand-off ring (on a track with elevation: and the per-env row tables); the frame filter,
    // the lens camera and scene lighting that are set are checked later, each with its own message
    if (e->cfg.render && trsim::handle_fit(e, variant_bits(e->rp.depth != 0, false, hills, false, false), L.lds_step) == trsim::LdsFit::no_launch)
        return fail(TRS_ERR_LIMIT, hills ? "no LDS left for the camera hand-off ring and the per-env row tables of a track with elevation" : "no LDS left for the camera hand-off ring");
    for (const StepKernel sk : kStepKernels)
        if (sk) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(sk), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(trs_locate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, L.p.blob_bytes));
    return TRS_OK;
}

TRS_EXPORT int trs_reset(trs_env* e, const uint8_t* h_mask)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    HIPCHK(hipSetDevice(e->device));
    int rc = sync_all(e);
    if (rc) return rc;
    if (!h_mask) { HIPCHK(hipMemset(e->pp.pending, 1, (size_t)e->n)); return TRS_OK; }
    std::vector<uint8_t> cur((size_t)e->n);
    HIPCHK(hipMemcpy(cur.data(), e->pp.pending, cur.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < e->n; ++i) if (h_mask[i]) cur[i] = 1;
    HIPCHK(hipMemcpy(e->pp.pending, cur.data(), cur.size(), hipMemcpyHostToDevice));
    return TRS_OK;
}

TRS_EXPORT int trs_step(trs_env* e, const float* d_st, const float* d_th, const float* d_br, const uint8_t* d_rs, int n_steps)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    if (n_steps < 1) return fail(TRS_ERR_ARG, "n_steps < 1");
    if (!d_st || !d_th) return fail(TRS_ERR_ARG, "null controls");
    HIPCHK(hipSetDevice(e->device));
    return step_call(e, Controls{d_st, d_th, d_br, d_rs, 0, 0}, n_steps, PerLaunch{n_steps, 1});   // held controls; the reset request applies to the first step only
}

TRS_EXPORT int trs_step_host(trs_env* e, const float* h_st, const float* h_th, const float* h_br, const uint8_t* h_rs, int n_steps)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    if (n_steps < 1) return fail(TRS_ERR_ARG, "n_steps < 1");
    if (!h_st || !h_th) return fail(TRS_ERR_ARG, "null controls");
    HIPCHK(hipSetDevice(e->device));
    return step_call(e, Controls{h_st, h_th, h_br, h_rs, 0, 0}, n_steps, PerLaunch{n_steps, 1}, true);
}

TRS_EXPORT int trs_step_sequence(trs_env* e, const float* d_st, const float* d_th, const float* d_br, const uint8_t* d_rs, int n_steps, int steps_per_launch)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    if (n_steps < 1 || steps_per_launch < 1) return fail(TRS_ERR_ARG, "n_steps / steps_per_launch < 1");
    if (!d_st || !d_th) return fail(TRS_ERR_ARG, "null controls");
    HIPCHK(hipSetDevice(e->device));
    return step_call(e, Controls{d_st, d_th, d_br, d_rs, 0, e->n}, n_steps, PerLaunch{steps_per_launch, steps_per_launch});
}

TRS_EXPORT int trs_step_sequence_host(trs_env* e, const float* h_st, const float* h_th, const float* h_br, const uint8_t* h_rs, int n_steps, int steps_per_launch)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    if (n_steps < 1 || steps_per_launch < 1) return fail(TRS_ERR_ARG, "n_steps / steps_per_launch < 1");
    if (!h_st || !h_th) return fail(TRS_ERR_ARG, "null controls");
    HIPCHK(hipSetDevice(e->device));
    { int rq = quiesce(e); if (rq) return rq; }            // the sequence is copied through the handle's stream
    const size_t cnt = (size_t)n_steps * (size_t)e->n;
    if (e->seq_buf.bytes() < cnt * 3 * sizeof(float)) {
        HIPCHK(hipStreamSynchronize(e->sP));
        HIPCHK(e->seq_buf.reserve(cnt * 3 * sizeof(float)));
    }
    float *ds = e->seq_buf.get(), *dt = ds + cnt, *db = dt + cnt;
    HIPCHK(hipMemcpyAsync(ds, h_st, cnt * 4, hipMemcpyHostToDevice, e->sP));
    HIPCHK(hipMemcpyAsync(dt, h_th, cnt * 4, hipMemcpyHostToDevice, e->sP));
    if (h_br) HIPCHK(hipMemcpyAsync(db, h_br, cnt * 4, hipMemcpyHostToDevice, e->sP));
    if (h_rs) HIPCHK(hipMemcpyAsync(e->ctl_reset, h_rs, (size_t)e->n, hipMemcpyHostToDevice, e->sP));
    return step_call(e, Controls{ds, dt, h_br ? db : nullptr, h_rs ? e->ctl_reset : nullptr, 0, e->n}, n_steps, PerLaunch{steps_per_launch, steps_per_launch});
}

TRS_EXPORT int trs_step_synthetic(trs_env* e, int n_steps, int steps_per_launch)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    if (n_steps < 1 || steps_per_launch < 1) return fail(TRS_ERR_ARG, "n_steps / steps_per_launch < 1");
    HIPCHK(hipSetDevice(e->device));
    return step_call(e, Controls{nullptr, nullptr, nullptr, nullptr, 1, 0}, n_steps, PerLaunch{steps_per_launch, steps_per_launch});
}

TRS_EXPORT int trs_get_state(trs_env* e, trs_state_view* o)
{
    if (!e || !o) return fail(TRS_ERR_ARG, "null argument");
    const PParams& k = e->pp;
    o->n_envs = e->n; o->img_h = e->H; o->img_w = e->W; o->n_points = k.np;
    o->img = latest_frame(e);
    o->pos_x = k.x; o->pos_y = k.y; o->pos_z = k.z; o->speed = k.speed; o->cte = k.cte; o->yaw = k.yaw; o->vel = k.v;
    o->seg_idx = k.seg_idx; o->ep_return = k.ep_return; o->last_return = k.last_return; o->ep_len = k.ep_len; o->done = k.done;
    o->step_count = e->step_count;
    o->depth = latest_depth(e);
    return TRS_OK;
}

TRS_EXPORT int trs_copy_to_host(trs_env* e, int which, void* dst, size_t bytes)
{
    if (!e || !dst) return fail(TRS_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(e->device));
    const PParams& k = e->pp;
    const void* src = nullptr; size_t need = 0; const size_t n = (size_t)e->n;
    bool host_src = false;
    switch (which) {
    case TRS_F_IMG: src = latest_frame(e); need = e->img_bytes; break;
    case TRS_F_POS_X: src = k.x; need = n * 4; break;
    case TRS_F_POS_Y: src = k.y; need = n * 4; break;
    case TRS_F_POS_Z: src = k.z; need = n * 4; break;
    case TRS_F_SPEED: src = k.speed; need = n * 4; break;
    case TRS_F_CTE: src = k.cte; need = n * 4; break;
    case TRS_F_YAW: src = k.yaw; need = n * 4; break;
    case TRS_F_VEL: src = k.v; need = n * 4; break;
    case TRS_F_SEG_IDX: src = k.seg_idx; need = n * 4; break;
    case TRS_F_EP_RETURN: src = k.ep_return; need = n * 4; break;
    case TRS_F_LAST_RETURN: src = k.last_return; need = n * 4; break;
    case TRS_F_EP_LEN: src = k.ep_len; need = n * 4; break;
    case TRS_F_DONE: src = k.done; need = n; break;
    case TRS_F_STEER_FILT: src = k.steer_filt; need = n * 4; break;
    case TRS_F_CTL_STEER: src = e->ctl_steer; need = n * 4; break;
    case TRS_F_CTL_THR: src = e->ctl_thr; need = n * 4; break;
    case TRS_F_CTL_BRK: src = e->ctl_brk; need = n * 4; break;
    case TRS_F_STATS: src = e->stats.get(); need = 64 * sizeof(unsigned long long); break;
    case TRS_F_DEPTH: src = latest_depth(e); need = n * e->H * e->W * 4; break;
    case TRS_F_ROWDEPTH: if (e->track_loaded) { src = e->trk.blob_r.get() + e->rp.off_depth; need = (size_t)e->H * 4; } break;
    // the tables live on the host exactly as built; their LDS images on the device are re-laid-out (pitched map)
    case TRS_F_MAP: if (e->track_loaded) { src = e->tab.map.data(); need = e->tab.map.size() * 4; host_src = true; } break;
    case TRS_F_ROWTAB: if (e->track_loaded) { src = e->trk.blob_r.get() + e->rp.off_rowtab; need = (size_t)e->H * 8; } break;
    case TRS_F_PALETTE: if (e->track_loaded) { src = e->trk.blob_r.get() + e->rp.off_pal; need = (size_t)e->H * 16; } break;
    case TRS_F_TANGENT: if (e->track_loaded) { src = e->trk.tangent.get(); need = (size_t)k.np * 8; } break;
    case TRS_F_DPITCH: if (e->track_loaded) { src = e->tab.dpitch.data(); need = e->tab.dpitch.size() * 4; host_src = true; } break;
    case TRS_F_LENS_TABLE: if (e->track_loaded && e->scene.lens_on) { src = e->lens.T.pix.data(); need = e->lens.T.pix.size() * 4; host_src = true; } break;
    case TRS_F_LENS_PALETTE: if (e->track_loaded && e->scene.lens_on && e->lens.dev.get()) { src = e->lens.dev.get() + e->lens.pal_off; need = (size_t)trsim::kLensPalBytes; } break;
    default: return fail(TRS_ERR_ARG, "unknown field");
    }
    if (!src) return fail(TRS_ERR_STATE, "field not available");
    if (bytes != need) return fail(TRS_ERR_ARG, "byte count mismatch");
    if (host_src) { std::memcpy(dst, src, need); return TRS_OK; }
    if (trsim::resident_on(e) && which != TRS_F_STATS) {
        // the worker keeps the handle's stream: wait for its posted steps (their bytes are written through to memory before
        // the completion flag), then copy on the side stream
        int rw = trsim::resident_wait(e);
        if (rw) return rw;
        hipStream_t sc = trsim::resident_copy_stream(e);
        HIPCHK(hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, sc));
        HIPCHK(hipStreamSynchronize(sc));
        e->d2h_bytes += need;
        return trsim::check_fault(e);
    }
    int rc = sync_all(e);
    if (rc) return rc;
    HIPCHK(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
    e->d2h_bytes += need;
    if (which == TRS_F_STATS && static_cast<unsigned long long*>(dst)[2] != 0)
        return fail(TRS_ERR_DEVICE, "raster kernel found its dynamic LDS segment at a non-zero offset");
    return TRS_OK;
}

TRS_EXPORT int trs_fetch_outputs(trs_env* e, uint8_t* h_img, float* h_x, float* h_y, float* h_z, float* h_speed, float* h_cte,
                                 int32_t* h_seg, uint8_t* h_done)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    if (h_img && !e->cfg.render) return fail(TRS_ERR_STATE, "the env has no camera (cfg.render == 0)");
    HIPCHK(hipSetDevice(e->device));
    const PParams& k = e->pp;
    const size_t n = (size_t)e->n, img_b = h_img ? e->img_bytes : 0;
    { int rs = fetch_staging(e, img_b); if (rs) return rs; }
    const FetchItem items[trsim::kFetchItems] = {
        {h_img ? latest_frame(e) : nullptr, h_img, img_b},
        {k.x, h_x, n * 4}, {k.y, h_y, n * 4}, {k.z, h_z, n * 4}, {k.speed, h_speed, n * 4}, {k.cte, h_cte, n * 4},
        {k.seg_idx, h_seg, n * 4}, {k.done, h_done, n},
    };
    hipStream_t cs = e->sP;
    if (trsim::resident_on(e)) { int rw = trsim::resident_wait(e); if (rw) return rw; cs = trsim::resident_copy_stream(e); }
    else { int rq = quiesce(e); if (rq) return rq; }
    return staged_fetch(e, items, cs);
}

// trs_fetch_outputs as the cars are told it (observation latency: trsim_latency.hip has the rest; this one shares the staging above)
TRS_EXPORT int trs_fetch_observation(trs_env* e, uint8_t* h_img, float* h_x, float* h_y, float* h_z, float* h_speed, float* h_cte,
                                     int32_t* h_seg, uint8_t* h_arrived)
{
    if (!e) return fail(TRS_ERR_ARG, "null handle");
    if (!e->obs.on()) return fail(TRS_ERR_STATE, "no observation latency is set (trs_set_latency): the observation is the state, trs_fetch_outputs");
    if (h_img && !e->cfg.render) return fail(TRS_ERR_STATE, "the env has no camera (cfg.render == 0)");
    HIPCHK(hipSetDevice(e->device));
    const size_t n = (size_t)e->n, img_b = h_img ? e->img_bytes : 0;
    { int rs = fetch_staging(e, img_b); if (rs) return rs; }
    trs_obs_view v;
    trsim::obs_view(e, &v);
    const FetchItem items[trsim::kFetchItems] = {
        {h_img ? v.img : nullptr, h_img, img_b},
        {v.pos_x, h_x, n * 4}, {v.pos_y, h_y, n * 4}, {v.pos_z, h_z, n * 4}, {v.speed, h_speed, n * 4}, {v.cte, h_cte, n * 4},
        {v.seg_idx, h_seg, n * 4}, {v.arrived, h_arrived, n},
    };
    return staged_fetch(e, items, e->sP);
}

TRS_EXPORT int trs_set_pose(trs_env* e, const float* x, const float* y, const float* z, const float* yaw, const float* v)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    HIPCHK(hipSetDevice(e->device));
    int rc = sync_all(e);
    if (rc) return rc;
    const size_t n = (size_t)e->n;
    const PParams& k = e->pp;
    if (x) HIPCHK(hipMemcpy(k.x, x, n * 4, hipMemcpyHostToDevice));
    if (y) HIPCHK(hipMemcpy(k.y, y, n * 4, hipMemcpyHostToDevice));
    if (z) HIPCHK(hipMemcpy(k.z, z, n * 4, hipMemcpyHostToDevice));
    if (yaw) HIPCHK(hipMemcpy(k.yaw, yaw, n * 4, hipMemcpyHostToDevice));
    if (v) HIPCHK(hipMemcpy(k.v, v, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(k.pending, 0, n));
    HIPCHK(hipMemset(k.done, 0, n));
    return TRS_OK;
}

TRS_EXPORT int trs_locate(trs_env* e, const double* h_xyz, int nq, int32_t* h_idx)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    if (nq < 0 || (nq && (!h_xyz || !h_idx))) return fail(TRS_ERR_ARG, "bad query");
    if (nq == 0) return TRS_OK;
    HIPCHK(hipSetDevice(e->device));
    { int rq = quiesce(e); if (rq) return rq; }
    if (nq > e->loc_cap) {
        HIPCHK(hipStreamSynchronize(e->sP));
        e->loc_cap = 0;
        HIPCHK(e->loc_q.alloc((size_t)nq * 24));
        HIPCHK(e->loc_out.alloc((size_t)nq * 4));
        e->loc_cap = nq;
    }
    HIPCHK(hipMemcpyAsync(e->loc_q.get(), h_xyz, (size_t)nq * 24, hipMemcpyHostToDevice, e->sP));
    constexpr int kW = kLocBlock / 64;
    int grid = (nq + kW - 1) / kW;
    grid = std::min(grid, e->cu_count * 2);
    const PParams& pk = e->pp;
    const NearParams near{pk.np, pk.off_py, pk.off_pz, pk.off_gstart, pk.off_gpts, pk.grid_nx, pk.grid_nz, pk.grid_x0, pk.grid_z0};
    hipLaunchKernelGGL(trs_locate_kernel, dim3(grid), dim3(kLocBlock), pk.blob_bytes, e->sP,
                       (const unsigned char*)e->trk.blob_p.get(), pk.blob_bytes, near, (const double*)e->loc_q.get(), nq, e->loc_out.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_idx, e->loc_out.get(), (size_t)nq * 4, hipMemcpyDeviceToHost, e->sP));
    HIPCHK(hipStreamSynchronize(e->sP));
    return TRS_OK;
}

TRS_EXPORT int trs_sync(trs_env* e)
{
    if (!e) return fail(TRS_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(e->device));
    if (trsim::resident_on(e)) { int rw = trsim::resident_wait(e); return rw ? rw : trsim::check_fault(e); }   // posted steps complete; the worker stays
    return sync_all(e);
}

TRS_EXPORT int trs_step_wait(trs_env* e, const float* d_st, const float* d_th, const float* d_br, const uint8_t* d_rs, int n_steps)
{
    const int rc = trs_step(e, d_st, d_th, d_br, d_rs, n_steps);
    return rc ? rc : trs_sync(e);
}

TRS_EXPORT int trs_quiesce(trs_env* e)
{
    if (!e) return fail(TRS_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(e->device));
    return quiesce(e);
}

TRS_EXPORT int trs_event_record(trs_env* e, int slot)
{
    if (!e || slot < 0 || slot >= 8) return fail(TRS_ERR_ARG, "bad event slot");
    HIPCHK(hipSetDevice(e->device));
    { int rq = quiesce(e); if (rq) return rq; }            // an event behind a resident worker would wait for the worker to leave anyway
    HIPCHK(hipEventRecord(e->ev[slot], e->sP));
    return TRS_OK;
}

TRS_EXPORT int trs_event_elapsed_ms(trs_env* e, int a, int b, float* ms)
{
    if (!e || !ms || a < 0 || a >= 8 || b < 0 || b >= 8) return fail(TRS_ERR_ARG, "bad event slot");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipEventSynchronize(e->ev[b]));
    HIPCHK(hipEventElapsedTime(ms, e->ev[a], e->ev[b]));
    return TRS_OK;
}

TRS_EXPORT int trs_scratch(trs_env* e, int slot, size_t bytes, void** d_out)
{
    if (!e || !d_out || slot < 0 || slot >= 32) return fail(TRS_ERR_ARG, "bad scratch slot (0..31) / null argument");
    HIPCHK(hipSetDevice(e->device));
    if (bytes > e->scratch[slot].bytes()) {
        int rc = sync_all(e);                                // nothing in flight may still use the old buffer
        if (rc) return rc;
        (void)e->scratch[slot].reset();
        trsim::DevBuf<void> nb;                              // (the slot takes it once it is zeroed)
        HIPCHK(nb.alloc(trsim::align_up(std::max<size_t>(bytes, 256), 256)));
        HIPCHK(hipMemset(nb.get(), 0, nb.bytes()));
        e->scratch[slot] = std::move(nb);
    }
    *d_out = e->scratch[slot].get();
    return TRS_OK;
}

TRS_EXPORT int trs_upload(trs_env* e, void* d_dst, const void* h_src, size_t bytes)
{
    if (!e || (bytes && (!d_dst || !h_src))) return fail(TRS_ERR_ARG, "null argument");
    if (!bytes) return TRS_OK;
    HIPCHK(hipSetDevice(e->device));
    { int rq = quiesce(e); if (rq) return rq; }
    HIPCHK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, e->sP));   // pageable source: staged before the call returns
    e->h2d_bytes += bytes;
    return TRS_OK;
}

TRS_EXPORT int trs_counters(trs_env* e, uint64_t out[4])
{
    if (!e || !out) return fail(TRS_ERR_ARG, "null argument");
    out[0] = e->d2h_bytes; out[1] = e->h2d_bytes; out[2] = e->step_count; out[3] = 0;
    return TRS_OK;
}

TRS_EXPORT const char* trs_last_error(void) { return g_err.c_str(); }

// ---- internal accessors for the other translation units (trsim_internal.hpp, trsim_env.hpp; not exported) ----------------------------------------------
bool trs_internal_view(trs_env* e, TrsEnvView* v)
{
    if (!e || !v) return false;
    if (quiesce(e)) return false;                            // the pilot's kernels go onto the handle's stream
    v->device = e->device; v->n = e->n; v->H = e->H; v->W = e->W; v->render = e->cfg.render;
    v->stream = e->sP;
    v->latest_frame = e->step_count > 0 ? latest_frame(e) : nullptr;
    v->speed = e->pp.speed; v->seg_idx = e->pp.seg_idx; v->n_points = e->pp.np;
    v->ctl_steer = e->ctl_steer; v->ctl_thr = e->ctl_thr; v->ctl_brk = e->ctl_brk;
    v->step_count = e->step_count;
    v->stats = e->stats.get();
    v->obs_on = e->obs.on();
    v->codec_quality = e->codec_quality;
    v->obs_frame = nullptr; v->obs_speed = nullptr; v->obs_seg_idx = nullptr; v->obs_mode = nullptr;
    if (v->obs_on && e->obs.steps(e->step_count) > 0) {                 // what the car is told (trs_get_observation); before the first step of the history: nothing
        trs_obs_view o;
        trsim::obs_view(e, &o);
        v->obs_frame = o.img; v->obs_speed = o.speed; v->obs_seg_idx = o.seg_idx; v->obs_mode = o.arrived + e->n;
    }
    return true;
}
void** trs_internal_pilot_slot(trs_env* e) { return e ? &e->pilot : nullptr; }
void** trs_internal_expert_slot(trs_env* e) { return e ? &e->expert : nullptr; }
const trs_pilot_tuning* trs_internal_pilot_tuning(trs_env* e) { return e && e->has_pilot_tuning ? &e->pilot_tuning : nullptr; }
void trs_internal_set_pilot_tuning(trs_env* e, const trs_pilot_tuning* t)
{
    if (!e) return;
    e->has_pilot_tuning = t != nullptr;
    if (t) e->pilot_tuning = *t;
}
int trs_internal_fail(int code, const std::string& msg) { return fail(code, msg); }
const uint8_t* trs_internal_latest_frame(const trs_env* e) { return e ? latest_frame(e) : nullptr; }
void trs_internal_count(trs_env* e, uint64_t d2h, uint64_t h2d) { if (e) { e->d2h_bytes += d2h; e->h2d_bytes += h2d; } }
// one env step by LAUNCH whatever the handle's step mode: the pilot loop's kernels need the CUs' LDS, which a resident worker
// would hold, and its controls are produced on the handle's stream right in front of the step
int trs_internal_step_launch(trs_env* e, const float* d_st, const float* d_th, const float* d_br)
{
    if (!e || !e->track_loaded) return fail(TRS_ERR_STATE, "no track loaded");
    { int rq = quiesce(e); if (rq) return rq; }
    // (like every step path: the uniform rows of a frame buffer — sky, beyond the far plane — are written by the first step that renders into it and kept after that:
    // 41 % of a frame's bytes at the default camera, 4.8 of the 16.5 us of this step at 1024 x 120x160, ~20 of 48 us at 512 x 240x320 + depth)
    const int rc = launch_steps(e, Controls{d_st, d_th, d_br, nullptr, 0, 0}, 1, PerLaunch{1, 1});
    if (!rc) trsim::resident_note_launch(e);               // resident mode selected: this step has no completion flag, trs_sync / the copies wait for the stream
    return rc;
}
// a closed loop keeps the frame of a captured tick: in front of the step, the handle recycles the buffer two steps on
int TrsLoopOps::keep_frame(int slot, const uint8_t* frame)
{
    HIPCHK(hipMemcpyAsync(cap->d_frames_or_null + (size_t)slot * e->img_bytes, frame, e->img_bytes, hipMemcpyDeviceToDevice, v.stream));
    return TRS_OK;
}
int trs_internal_replay_launch(trs_env* e, const trsim::Controls& c, uint64_t step)
{
    return e->cfg.render ? launch_step(e, c, 1, 0, 0, step) : launch_physics(e, c, 1, step);
}
void trs_internal_note(const std::string& msg) { g_err = msg; }
int trsim::sync_handle(trs_env* e) { return sync_all(e); }
int trsim::quiesce_handle(trs_env* e) { return quiesce(e); }
int trsim::check_fault(trs_env* e)
{
    if (e->fault.get() && __atomic_load_n(e->fault.get(), __ATOMIC_ACQUIRE) != 0ull)
        return fail(TRS_ERR_DEVICE, "a step kernel found its dynamic LDS segment at a non-zero offset and refused to run: frames and state are stale");
    return TRS_OK;
}

#ifdef TRS_DEBUG_PROBES
// Debug build only (scripts/det_probe.py; never part of libtrsim.so): fill the whole LDS of every CU with a pattern on the
// handle's stream, so that a kernel reading LDS bytes it has not (yet) written shows a wrong result instead of silently
// re-reading what its own previous launch left there.
__global__ __launch_bounds__(1024) void trs_debug_poison_kernel(unsigned pattern, int bytes, int spin)
{
    u4v* d = reinterpret_cast<u4v*>(smem);
    for (int i = threadIdx.x; i < bytes / 16; i += blockDim.x) d[i] = (u4v)(pattern);
    __syncthreads();
    const long long t0 = clock64();
    while (clock64() - t0 < spin) __builtin_amdgcn_s_sleep(8);            // stay resident so that every CU gets a workgroup
}

TRS_EXPORT int trs_debug_poison_lds(trs_env* e, unsigned pattern, int bytes)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(trs_debug_poison_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    hipLaunchKernelGGL(trs_debug_poison_kernel, dim3(512), dim3(1024), bytes, e->sP, pattern, bytes, 20000);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}

// ... and: occupy a slice of every CU's LDS from another stream for `cycles` clocks (touch = 1: keep rewriting that slice), so
// that workgroups launched meanwhile get an LDS allocation that does not start at the CU's LDS address 0.
__global__ __launch_bounds__(64) void trs_debug_spin_kernel(int bytes, long long cycles, int touch)
{
    u4v* d = reinterpret_cast<u4v*>(smem);
    const long long t0 = clock64();
    unsigned k = 0;
    while (clock64() - t0 < cycles) {
        if (touch) for (int i = threadIdx.x; i < bytes / 16; i += 64) d[i] = (u4v)(0xDEAD0000u + k++);
        __builtin_amdgcn_s_sleep(8);
    }
}

TRS_EXPORT int trs_debug_spin(trs_env* e, int wgs, int bytes, long long cycles, int touch)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    static hipStream_t side = nullptr;
    HIPCHK(hipSetDevice(e->device));
    if (!side) HIPCHK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(trs_debug_spin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    hipLaunchKernelGGL(trs_debug_spin_kernel, dim3(wgs), dim3(64), bytes, side, bytes, cycles, touch);
    HIPCHK(hipGetLastError());
    return TRS_OK;
}
#endif
