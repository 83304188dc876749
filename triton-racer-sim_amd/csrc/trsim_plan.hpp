// trsim_plan.hpp — what a handle is allowed to become and how a call is cut up, as integer arithmetic and string selection a host compiler builds without HIP:
// the kernel variants and which of them exist, the LDS the kernels keep behind a track's tables (the layouts the hosts size their launches by
// and the kernels take their offsets from), the layout of a track's two LDS images, the refusals that follow from all three, the frame buffers that hold their
// uniform rows (UniformRows), the observation ring and its bytes (ObsRing, obs_bytes), the controls of a step call and their slices (Controls) and a fetch's staging (fetch_layout).
// Functions that the kernels call as well carry TRS_HD (trsim_tables.hpp).  tests/plan_driver.cpp and tests/host_tables_driver.cpp run it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "trsim_tables.hpp"

#ifndef TRS_RASTER_WAVES
#define TRS_RASTER_WAVES 8    /* raster waves per workgroup: 512 threads = 12 full rows of 40 groups per pass, 10 passes exactly at 120x160, and 12 waves balance over the 4 SIMDs (10 + 5 waves: 72.5 M env-steps/s, 8 + 4: 77.0 M; profiles/r01_step_kernel_waves_ab.txt) */
#endif

namespace trsim {

constexpr int kRasterThreads = 64 * TRS_RASTER_WAVES;
constexpr int kPhysBlock = 256;             // threads of the physics-only kernel
constexpr int kCamDepth = 4;                // resident worker: steps the physics team may run ahead of the raster team
constexpr int kSlotWords = 20;              // resident worker, one hand-off slot: camera parameters (4) | x y z yaw v speed cte seg epr epl sf last_return (12) | done | view pitch (a track with elevation) | 2 spare
constexpr int kLensPalBytes = 513 * 16;
constexpr int kDynTabWords = 512 + 768 + 4 + 256;   // ... | cnt[256]: the class counts of a row's 4-pixel pack (n0 | n1 << 8 | n2 << 16 | n3 << 24; round 4, see raster_dyn_batch phase A)

// A raster thread owns one 4-pixel column group (gpr = W / 4 of them per row) of every rows_per_pass-th row: the threads beyond rows_per_pass * gpr idle
// (32 of 512 at W = 160), and a frame takes ceil(H / rows_per_pass) passes, the last of them ragged where H is no multiple.
TRS_HD inline int raster_rows_per_pass(int gpr) { return kRasterThreads / (gpr > 0 ? gpr : 1); }
// the dynamic-brightness filter's brightness window: image rows [lo, hi) = img[40:119] (img_preprocessing.py:88), cut to the frame; empty for H <= 40
TRS_HD inline int dyn_window_lo(int H) { return H < 40 ? H : 40; }
TRS_HD inline int dyn_window_hi(int H) { return H < 119 ? H : 119; }

// Which instantiation of trs_step_kernel / trs_worker_kernel <DEPTH, DYN, HILLS, LENS, LIGHT> renders: one bit per template flag (variant_of in
// trsim_env.hpp).  14 of the 32 are built, DEPTH x {plain, DYN, HILLS, LENS, LIGHT, LIGHT + HILLS, LIGHT + DYN}: the setters refuse the others first
// (variant_clash).
using Variant = unsigned;
constexpr Variant kVDepth = 1, kVDyn = 2, kVHills = 4, kVLens = 8, kVLight = 16, kVariants = 32;
constexpr Variant variant_bits(bool depth, bool dyn, bool hills, bool lens, bool light)
{
    return (depth ? kVDepth : 0u) | (dyn ? kVDyn : 0u) | (hills ? kVHills : 0u) | (lens ? kVLens : 0u) | (light ? kVLight : 0u);
}
constexpr bool variant_built(Variant v) { return !((v & kVDyn) && (v & kVHills)) && !((v & kVLens) && (v & (kVDyn | kVHills | kVLight))); }

// ---- may this handle run variant v: the one owner of the refusals by policy ------------------------------------------------------
// A setter forms what the handle would run after its change, state | add, and asks here.  The answer is the feature bit of `state` that is not built
// together with `add` (0: the combination is built); where two set bits clash with `add` the first in the order HILLS, DYN, LENS, LIGHT is named.
inline Variant variant_clash(Variant state, Variant add)
{
    if (variant_built(state | add)) return 0;
    for (const Variant b : {kVHills, kVDyn, kVLens, kVLight})
        if ((state & b) && !variant_built(add | b)) return b;
    return 0;
}
// what the caller is told (TRS_ERR_STATE) when `add` meets `set`; trs_load_track adds HILLS with the track it loads
inline const char* variant_refusal(Variant add, Variant set)
{
    struct Text { Variant add, set; const char* text; };
    static const Text kTexts[] = {
        {kVHills, kVLens, "this track has elevation and a lens camera is set: the lens camera is built for flat tracks only (trs_set_camera(NULL) first); the handle keeps its track"},
        {kVHills, kVDyn, "this track has elevation: the dynamic-brightness frame filter that was set has been removed (a frame's palette is evaluated per env inside the kernels there; "
                         "the static filter works, or use trs_preprocess on the rendered frames)"},
        {kVDyn, kVHills, "the loaded track has elevation: a frame's palette is evaluated per env inside the kernels there, and the dynamic-brightness filter behind the "
                         "rasteriser is not built for that; the static filter works, or use trs_preprocess on the rendered frames"},
        {kVDyn, kVLens, "a lens camera is set: the dynamic-brightness filter behind the rasteriser is not built for the lens camera (trs_set_camera(NULL) first); "
                        "the static filter works, or use trs_preprocess on the rendered frames"},
        {kVLens, kVHills, "the loaded track has elevation: the lens camera is built for flat tracks only (the ground plane of a hilly track tilts per env and frame)"},
        {kVLens, kVDyn, "the dynamic-brightness frame filter is set: it is not built for the lens camera (trs_set_frame_filter without dynamic brightness, or NULL, first)"},
        {kVLens, kVLight, "scene lighting is set: it is not built for the lens camera (trs_set_lighting(NULL) first)"},
        {kVLight, kVLens, "a lens camera is set: scene lighting is not built for the lens camera (trs_set_camera(NULL) first)"},
    };
    for (const Text& t : kTexts)
        if (t.add == add && t.set == set) return t.text;
    return "";
}

// ---- the LDS of the kernels' variants behind a track's tables ---------------------------------------------------------------
// tracks with elevation: the batch's row tables (trsim_device.hpp, hill_batch_build)
constexpr int kHillRowBytes = 28;
constexpr int kHillBatchMax = 4;
// One row table: float2 rowtab[H] | (16-aligned) uint32 palette[H][4] | float depth[H].  The palette plane is written and read 16 bytes at a time, so it starts
// on a multiple of 16 for every H: behind an odd H's rowtab come 8 bytes of padding (an even H has none: 8 H | 16 H | 4 H = kHillRowBytes * H as before).
// hill_row_build, raster_use_table and hill_table_bytes all take the plane offsets from here.
TRS_HD inline int hill_table_pal_off(int H) { return (8 * H + 15) & ~15; }
TRS_HD inline int hill_table_depth_off(int H) { return hill_table_pal_off(H) + 16 * H; }
TRS_HD inline int hill_table_bytes(int H) { return (hill_table_depth_off(H) + 4 * H + 15) & ~15; }
TRS_HD inline int hill_batch(int H) { const int b = kRasterThreads / (H > 0 ? H : 1); return b < 1 ? 1 : (b > kHillBatchMax ? kHillBatchMax : b); }
TRS_HD inline int hill_lds_bytes(int H) { return hill_batch(H) * hill_table_bytes(H) + 48; }   // the batch's tables + the team-barrier counter (4 B) + 12 B spare + int first_ground[2][4]: an env's first row that sees the ground, by batch parity

constexpr int kDynBatch = 4;                  // envs per batch of the dynamic-brightness filter behind the rasteriser (raster_dyn_batch)
TRS_HD inline int light_copies(int gpr) { return (gpr + 63 + 63) / 64; }
TRS_HD inline int light_pal_bytes(int H, int gpr) { return light_copies(gpr) * H * 16; }
// The LDS of scene lighting behind the row tables (or where they would sit): the parameters of `slots` envs (the step kernel: the workgroup's envs; the
// worker: a ring of kCamDepth steps of them), then on a flat track the waves' lit palettes — or, with the dynamic-brightness filter, the batch's lit
// palettes by channel (raster_dyn_batch)
TRS_HD inline int light_lds_extra(int H, int W, int slots, bool hilly, bool dyn)
{
    return slots * 32 + (hilly ? 0 : (dyn ? kDynBatch * H * 16 : light_pal_bytes(H, W / 4)));
}
TRS_HD inline int dyn_lds_bytes(int H) { return kDynBatch * H * 16 + 128 + ((kDynTabWords * 4 + 15) & ~15) + H * 16; }   // ... + rowch[H]: the raw palette by channel

// The step kernel's dynamic LDS behind its tables (lds_step bytes: raster image, physics image) for variant v and n_phys physics steps per launch: the one
// layout launch_step sizes the launch and fills SParams / FParams from, and the kernel takes lds_off_pitch, lds_off_hill and lds_off_light from
// (step_lds_behind, from SParams::lds_off_prog: the same arithmetic the kernels always did; the layout's size comes on top of it).
//   cam:   float4 lcam[max(n_phys, 1) + 1][epw]   (the last row: the poses of the step before the launch)
//   prog:  int pprog[epw] + 16 spare bytes
//   pitch: float lpitch[max(n_phys, 1) + 1][epw]  (HILLS; LENS and LIGHT keep the region)
//   hill:  (16-aligned) the batch's row tables and the raster team's barrier counter (HILLS) or the lens palette (LENS)
//   light: (16-aligned, LIGHT) the workgroup's lighting parameters, then the lit palettes
//   dyn:   (16-aligned, DYN) the dynamic-brightness filter's palettes, sums and tables (FParams::lds_off)
TRS_HD inline int imax(int a, int b) { return (a > b) ? a : b; }   // (the device compiler's max(int, int), for both compilers: written out in place, the HILLS step kernels allocate registers differently)
struct StepLds { int cam, prog, pitch, hill, light, dyn, total; };
// the region at `hill` of both kernels' layouts: the batch's row tables (HILLS) or the lens palette (LENS)
TRS_HD inline int tabs_lds_bytes(int H, Variant v) { return (v & kVHills) ? hill_lds_bytes(H) : ((v & kVLens) ? kLensPalBytes : 0); }
TRS_HD inline StepLds step_lds_behind(int prog, int epw, int H, Variant v, int n_phys)
{
    const int rows = imax(n_phys, 1) + 1;
    StepLds L;
    L.prog = prog;
    L.cam = prog - rows * epw * 16;
    L.pitch = L.prog + epw * 4 + 16;
    L.hill = (L.pitch + rows * epw * 4 + 15) & ~15;
    L.light = (L.hill + tabs_lds_bytes(H, v) + 15) & ~15;
    return L;
}
TRS_HD inline StepLds step_lds_layout(int lds_step, int epw, int H, int W, Variant v, int n_phys)
{
    StepLds L = step_lds_behind(lds_step + (imax(n_phys, 1) + 1) * epw * 16, epw, H, v, n_phys);
    int end = L.pitch;
    if (v & (kVHills | kVLens | kVLight)) end = L.hill + tabs_lds_bytes(H, v);
    if (v & kVLight) end = L.light + light_lds_extra(H, W, epw, (v & kVHills) != 0, (v & kVDyn) != 0);
    L.dyn = (end + 15) & ~15;
    L.total = (v & kVDyn) ? L.dyn + dyn_lds_bytes(H) : end;
    return L;
}

// what a workgroup of the resident worker shares in LDS (behind the tables): WLds in trsim_resident.hip
TRS_HD inline size_t wlds_slot_off(int epw) { return (64 + (size_t)epw * 8 + 15) & ~(size_t)15; }
TRS_HD inline size_t wlds_bytes(int epw)
{
    return wlds_slot_off(epw) + (size_t)kCamDepth * epw * kSlotWords * 4 + (size_t)epw * 64;
}

// The render worker's dynamic LDS behind the tables (lds_step bytes) for variant v: the one layout worker_fits sizes the launch by and fills WParams
// from; the kernel takes lds_off_light from its last step (worker_lds_light, from WParams::lds_off_hill).
//   ctl:   the control block (WLds) + 16 spare bytes
//   dyn:   (16-aligned, DYN) the dynamic-brightness filter's palettes, sums and tables (FParams::lds_off)
//   hill:  (16-aligned) the batch's row tables and the raster team's barrier counter (HILLS) or the lens palette (LENS)
//   light: (16-aligned, LIGHT) the ring of lighting parameters float[kCamDepth][epw][8], then the lit palettes
struct WorkerLds { int ctl, dyn, hill, light, total; };
TRS_HD inline int worker_lds_light(int hill, int H, Variant v) { return (hill + tabs_lds_bytes(H, v) + 15) & ~15; }
TRS_HD inline WorkerLds worker_lds_layout(int lds_step, int epw, int H, int W, Variant v)
{
    WorkerLds L;
    L.ctl = (lds_step + 15) & ~15;
    int end = (int)(L.ctl + wlds_bytes(epw) + 16);
    L.dyn = (end + 15) & ~15;
    if (v & kVDyn) end = L.dyn + dyn_lds_bytes(H);
    L.hill = (end + 15) & ~15;
    if (v & (kVHills | kVLens)) end = L.hill + tabs_lds_bytes(H, v);
    L.light = worker_lds_light(L.hill, H, v);
    L.total = (v & kVLight) ? L.light + light_lds_extra(H, W, kCamDepth * epw, (v & kVHills) != 0, (v & kVDyn) != 0) : end;
    return L;
}

// Physics steps per launch of variant v beside lds_step bytes of tables: the largest n <= 16 whose step_lds_layout fits a CU's 160 KiB (0: not even one).
inline int steps_that_fit(int lds_step, int epw, int H, int W, Variant v)
{
    int n = 0;
    while (n < 16 && step_lds_layout(lds_step, epw, H, W, v, n + 1).total <= 160 * 1024) ++n;
    return n;
}
// the render worker's LDS layout of variant v fits a CU beside lds_step bytes of tables
inline bool resident_fits(int lds_step, int epw, int H, int W, Variant v) { return worker_lds_layout(lds_step, epw, H, W, v).total <= 160 * 1024; }
// The one LDS question of every setter, about the variant the handle would run after the change: v fits by launches beside lds_step bytes of tables and,
// when resident mode is on, the worker fits.  The caller attaches its own message to whichever failed.
enum class LdsFit { ok, no_launch, no_worker };
inline LdsFit lds_fit(int lds_step, int epw, int H, int W, Variant v, bool resident)
{
    if (steps_that_fit(lds_step, epw, H, W, v) < 1) return LdsFit::no_launch;
    return resident && !resident_fits(lds_step, epw, H, W, v) ? LdsFit::no_worker : LdsFit::ok;
}

// ---- uniform rows: which frame buffers already hold them, and what a raster wave of the worker then stores ---------------------------
// The leading RParams::uni_rows rows of a frame (sky, ground beyond the far plane) are the palette's rows: they depend on neither the pose, the env
// nor the step.  A frame buffer that a step has rendered into with the present palette holds them for every env, and later steps into that buffer
// store only the rows that see the track; the consumer still finds a whole frame.  This is the one owner of "does buffer b hold them":
//   launch_step, worker_launch ask skip_mask();  launch_step and the worker's exit (handle_exit) report what was rendered with rendered();
//   upload_palette (track, frame filter, camera, lens, lighting), the buffers' allocation, trs_set_latency (on and off: the handle's ObsHistory, trsim_latency.hpp,
//   takes the steps' frames meanwhile) and a worker that ended by its abort bit call invalidate().
// DYN, LENS and LIGHT frames have no such rows (the filter follows each frame's mean, the lens decides per pixel, the palette is lit per env): a step
// of those variants skips nothing and leaves its buffer without them.  HILLS has uni_rows == 0: skipping is a no-op there.
constexpr bool variant_keeps_uniform(Variant v) { return !(v & (kVDyn | kVLens | kVLight)); }
struct UniformRows {
    bool ok[2] = {false, false};                // frame buffer b (= step index & 1) holds the present palette's uniform rows of every env
    void invalidate() { ok[0] = ok[1] = false; }
    // bit b: steps of variant v that render into buffer b need not store their uniform rows
    unsigned skip_mask(Variant v) const { return variant_keeps_uniform(v) ? (ok[0] ? 1u : 0u) | (ok[1] ? 2u : 0u) : 0u; }
    // steps [first, first + n) of variant v have rendered (whole frames, or all but rows the buffer held already)
    void rendered(Variant v, unsigned long long first, unsigned long long n)
    {
        for (unsigned long long k = 0; k < n && k < 2; ++k) ok[(first + k) & 1ull] = variant_keeps_uniform(v);
    }
};

// The resident worker's raster waves (trs_worker_kernel, the plain path) skip the uniform rows of step s when the host's mask says buffer s & 1 holds them,
// or when this launch of the worker (it began at step `start`) has itself rendered step s - 2: every thread then skips exactly the bytes it stored two steps ago.
TRS_HD inline bool worker_skips_uniform(unsigned mask, unsigned long long start, unsigned long long s) { return ((mask >> (s & 1ull)) & 1u) != 0 || s - start >= 2; }
// Store instructions a raster wave issues for one step: nstep with its uniform rows (nuni of them), nstep - nuni without.
TRS_HD inline int worker_step_stores(int nstep, int nuni, bool skips) { return skips ? nstep - nuni : nstep; }
// The count of the lagged arrival for step `owed`, taken inside step s (owed < s) behind `uni_now` store instructions of step s's uniform rows: exactly what
// the wave has issued since the end of step `owed` — the whole steps between, each with or without its uniform rows, and uni_now.  (A count that is too
// small only waits longer; one that is too large would publish a frame before it is in memory.)
TRS_HD inline int worker_wait_count(unsigned mask, unsigned long long start, unsigned long long owed, unsigned long long s, int nstep, int nuni, int uni_now)
{
    int n = uni_now;
    for (unsigned long long q = owed + 1; q < s; ++q) n += worker_step_stores(nstep, nuni, worker_skips_uniform(mask, start, q));
    return n;
}
// Steps of lag between a wave's stores and its arrival: two always, three where two whole steps and the uniform rows in front of the wait still fit the
// 6-bit counter — sized by the steps a launch of the worker spends its life on: without their uniform rows where the variant skips them (from its third
// step on; the first two may be longer, their counts are then clamped to 63, which only waits for more).
TRS_HD inline int worker_lag(int nstep, int nuni, bool skipping) { return (2 * worker_step_stores(nstep, nuni, skipping) + (skipping ? 0 : nuni) <= 63) ? 3 : 2; }

// ---- observation latency: the ring of truth records and where an env's observation lies in it ----------------------------------------
// With a latency set (trs_set_latency; include/trsim_spec.h, "observation latency") step T of the history (T = 1 for the first step since the history
// began) renders into ring slot slot_of_step(T) and trs_obs_kernel files its telemetry there.  The observation of an env with delay L after step T is
// the record of step T - L; it must stay intact while step T + 1 renders, so the ring has max_ticks + 2 slots: the records T - max_ticks .. T that
// observations after T may point into, and the one step T + 1 writes.  A step index <= 0 names a slot that no step of the history has written yet
// (T - L > -slots()): the ring is zeroed when the history begins, so such a slot holds the constructor's state, all zeros.
// The one owner of this arithmetic: launch_step, trs_obs_kernel's parameters and the views (trs_get_state, trs_get_observation) ask here.
constexpr int kMaxLatencyTicks = 30;
struct ObsRing {
    int max_ticks = 0;                                       // 0: latency is off
    bool on() const { return max_ticks > 0; }
    int slots() const { return max_ticks + 2; }
    int slot_of_step(long long T) const { const int S = slots(); return (int)(((T % S) + S) % S); }
    static bool arrived(long long T, int L) { return T - L >= 1; }
    int slot_of_obs(long long T, int L) const { return slot_of_step(T - (long long)L); }
    // the gathered observation (telemetry always; frames when the envs' delays differ) is double buffered like the frames of a handle without latency
    static int gather_buf(long long T) { return (int)(T & 1ll); }
};
// The bytes behind a ring: a slot's frames (and depth frames) of all envs lie *_stride bytes apart, a multiple of 256; 0 without a camera / without depth.
// trs_set_latency allocates by it, launch_obs takes an env's frame bytes from it; tests/latency_driver.cpp prints it.  All in size_t.
struct ObsBytes {
    size_t img_env, dep_env;                                 // one env's frame, depth frame
    size_t img_stride, dep_stride, ring_img, ring_dep;       // a slot of every env's frames; all slots
    size_t ring_tel, tel, flag, ticks;                       // [slots][6][n] | [6][n] | arrived[n], mode[n] | int32[n]
};
inline ObsBytes obs_bytes(const ObsRing& r, int n_envs, int H, int W, bool render, bool depth)
{
    const size_t n = (size_t)n_envs, slots = (size_t)r.slots(), px = (size_t)H * (size_t)W;
    auto up256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    ObsBytes b{};
    b.img_env = render ? px * 3 : 0; b.dep_env = render && depth ? px * 4 : 0;
    b.img_stride = up256(n * b.img_env); b.dep_stride = up256(n * b.dep_env);
    b.ring_img = slots * b.img_stride; b.ring_dep = slots * b.dep_stride;
    b.tel = 6 * n * 4; b.ring_tel = slots * b.tel; b.flag = 2 * n; b.ticks = n * 4;
    return b;
}

// ---- the controls of a step call, and the slice of them a launch or a post reads ----------------------------------------------------------
// Control arrays (device pointers, or host arrays on their way to the device; brk and reset optional), or synth: the spec's generator and no arrays.
// stride: floats between the control sets of consecutive steps, 0 = held controls, n_envs = a sequence.  The reset mask belongs to the first step alone.
// The one owner of "which controls does step k of the call read": the launch loops (run_camera_steps, run_physics_steps), the worker's post loop
// (resident_post) and the remainder of a call whose worker fell back to launches all ask after().  after(a).after(b) == after(a + b).
struct Controls {
    const float *steer = nullptr, *thr = nullptr, *brk = nullptr;
    const uint8_t* reset = nullptr;
    int synth = 0, stride = 0;
    Controls after(int k) const                              // the controls of the call's remainder after k steps
    {
        const size_t off = (size_t)k * (size_t)stride;
        return {steer ? steer + off : nullptr, thr ? thr + off : nullptr, brk ? brk + off : nullptr, k == 0 ? reset : nullptr, synth, stride};
    }
};

// ---- the pinned staging of a fetch (trs_fetch_outputs, trs_fetch_observation) ----------------------------------------------------------------
// Up to eight optional items (the frame, six words per env, a byte per env) go through one pinned block behind one synchronisation; bytes[i] == 0: item i is
// not asked for.  Every present item starts 16-byte aligned, in table order.  The block is reserved for the frame asked for and all seven per-env items.
constexpr int kFetchItems = 8;
constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
constexpr size_t fetch_reserve(size_t img_bytes, size_t n_envs) { return align16(img_bytes) + 7 * align16(n_envs * 4) + 16; }
struct FetchLayout { size_t off[kFetchItems], end; };
inline FetchLayout fetch_layout(const size_t (&bytes)[kFetchItems])
{
    FetchLayout L{};
    for (int i = 0; i < kFetchItems; ++i) { L.off[i] = L.end; L.end += align16(bytes[i]); }
    return L;
}

// ---- the two LDS images of a track ------------------------------------------------------------------------------------------
// physics image:  px | py | pz | tangent (tan_in_lds) | grid starts | grid points, and behind it the physics-only kernel's scratch (lds_p bytes of LDS)
// raster image:   map (rows pitched to an odd number of words) @0 | rowtab | palette | depth | sky (a track with elevation)
// The fused kernels stage the raster image at 0 and the physics image at lds_off_phys: lds_step bytes of tables, behind which the layouts above begin.
struct TrackLayout {
    struct Phys { int off_py, off_pz, off_tan, tan_in_lds, off_gstart, off_gpts, blob_bytes, off_scratch, pts_bytes, lds_p; } p;
    struct Raster { int map_pitch_b, off_rowtab, off_pal, off_depth, off_sky, blob_bytes, lds_r; } r;
    int lds_off_phys, lds_step;
};
// TRS_OK, or TRS_ERR_LIMIT with the message in `err`: a track whose images the kernels cannot hold
int track_layout(const TrackTables& T, int H, bool render, int envs_per_wg, TrackLayout& L, std::string& err);
// the two host byte images (blob_bytes each) of a layout that track_layout accepted
void pack_track_images(const TrackTables& T, int H, const TrackLayout& L, std::vector<unsigned char>& phys, std::vector<unsigned char>& raster);

}  // namespace trsim
