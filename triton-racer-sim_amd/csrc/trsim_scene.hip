// trsim_scene.hip — the scene of a handle on the device: the entry points of include/trsim.h that change what a handle renders — trs_load_track,
// trs_set_frame_filter, trs_set_camera (+ trs_default_camera, trs_get_camera), trs_set_lighting / trs_set_lighting_host — and trs_map_info_get.  No kernel
// lives here.  What is uploaded is decided and laid out in trsim_scene.hpp (host-only: tests/scene_driver.cpp runs it on the CPU); every upload below is
// three steps: ask that header for the bytes, allocate, copy.  The handle itself, its stream and its kernels are trsim_hip.hip's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/trsim.h"
#include "../../include/trsim_spec.h"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"
#include "trsim_scene.hpp"
#include "trsim_tables.hpp"

// OpenCV's reciprocal tables (hsv_reciprocals, trsim_filter.hpp) on the device, uploaded once per handle: trs_preprocess (trsim_image.hip) and the
// in-kernel static filter of a track with elevation / scene lighting (upload_palette) read them from there
int trsim::ensure_hsv_table(trs_env* e)
{
    if (e->hsv_tab.get()) return TRS_OK;
    int tab[512];
    trsim::hsv_reciprocals(tab);
    HIPCHK(e->hsv_tab.alloc(sizeof tab));
    HIPCHK(hipMemcpy(e->hsv_tab.get(), tab, sizeof tab, hipMemcpyHostToDevice));
    return TRS_OK;
}

namespace {
using trsim::handle_fit; using trsim::variant_now; using trsim::variant_of; using trsim::sync_handle;
using trsim::LensStage; using trsim::TrackStage;           // what the handle holds as e->lens and e->trk (trsim_env.hpp)

// ---- the palette and the tables: what trs_load_track and the setters below (frame filter, camera, lighting) upload ----

// the tables the DYN step kernels stage into LDS (FParams::tabs) for filter c
int upload_dyn_tables(trs_env* e, const trs_pre_config& c)
{
    int rc = trsim::ensure_hsv_table(e);
    if (rc) return rc;
    const std::vector<unsigned> t = trsim::dyn_table(c);
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; HIPCHK(hipStreamSynchronize(e->sP)); }   // a running kernel may still be staging the old tables
    HIPCHK(e->dyn_tab.reserve(t.size() * sizeof(unsigned)));   // (allocated once: the size is fixed)
    HIPCHK(hipMemcpy(e->dyn_tab.get(), t.data(), t.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    return TRS_OK;
}

// (re)write every colour of the scene: the palette of the raster LDS image, the lens palette, and the colour half of the block behind the image
int upload_palette(trs_env* e)
{
    if (!e->track_loaded || !e->cfg.render) return TRS_OK;
    const trsim::Scene& s = e->scene;
    const trsim::FlatPalette fp = trsim::flat_palette(s, e->tab, e->H);
    { int rq = sync_handle(e); if (rq) return rq; }            // frames in flight keep the palette they were launched with (a resident worker leaves here and reports what it rendered)
    e->rp.uni_rows = fp.uni_rows;
    e->uniform_ok.invalidate();                                // (steps skip uniform rows an earlier step wrote: not across a palette change)
    HIPCHK(hipMemcpy(e->trk.blob_r.get() + e->rp.off_pal, fp.pal.data(), fp.pal.size() * 4, hipMemcpyHostToDevice));
    if (s.lens_on && e->lens.dev.get()) {
        const std::vector<uint32_t> lp = trsim::lens_palette(s, e->lens.T);
        HIPCHK(hipMemcpy(e->lens.dev.get() + e->lens.pal_off, lp.data(), lp.size() * 4, hipMemcpyHostToDevice));
    }
    if (s.hilly || s.light_on) {                               // (the kernels that read the block's colour half)
        trsim::HillBlock hb = s.hill;
        const std::vector<uint32_t> sky = trsim::hill_colours(s, e->tab, hb);
        if (hb.filt) {
            int rc = trsim::ensure_hsv_table(e);
            if (rc) return rc;
            hb.hsv_tab = e->hsv_tab.get();
        }
        hb.light = s.light_on ? e->light : nullptr;
        if (s.hilly) HIPCHK(hipMemcpy(e->trk.blob_r.get() + hb.off_sky, sky.data(), sky.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->trk.blob_r.get() + trsim::hill_block_offset(e->rp.blob_bytes), &hb, sizeof hb, hipMemcpyHostToDevice));
    }
    return TRS_OK;
}

// The lens tables of a map for a camera (include/trsim_spec.h, "lens camera"), STAGED: host tables in binary64, their device image (lens_image: the half-width
// planes and the palette) in a buffer of its own, and the LensBlock written into the raster image `blob_r` (the new track's, not yet committed,
// in trs_load_track; the handle's own, with nothing in flight, in trs_set_camera).  Nothing of the handle changes here: the caller moves S into e->lens.
// `lds_step` / `cell`: the step kernel's LDS image and the map cell of the track the tables are for.  *block_written (optional): the copy into blob_r was begun.
int lens_stage(const trs_env* e, const trs_camera& cam, int lds_step, double cell, unsigned char* blob_r, int blob_bytes, LensStage& S, bool* block_written = nullptr)
{
    if (handle_fit(e, variant_bits(e->rp.depth != 0, false, false, true, false), lds_step) == trsim::LdsFit::no_launch)   // (a lens excludes the other variants)
        return trs_internal_fail(TRS_ERR_LIMIT, "no LDS left beside this track's tables for the lens camera's palette (" + std::to_string(lds_step) + " B of tables at " +
                                   std::to_string(e->pp.envs_per_wg) + " envs per workgroup): the lens camera needs a shorter track or fewer envs per GPU");
    std::string err;
    int rc = trsim::build_lens_tables(e->cfg, cell, cam.fish_eye_x, cam.fish_eye_y, S.T, err);
    if (rc) return trs_internal_fail(rc, err);
    const trsim::LensImage im = trsim::lens_image(e->scene, S.T);
    HIPCHK(S.dev.alloc(im.bytes.size()));
    HIPCHK(hipMemcpy(S.dev.get(), im.bytes.data(), im.bytes.size(), hipMemcpyHostToDevice));
    trsim::LensBlock lb{};
    unsigned char* const d = S.dev.get();
    lb.F = reinterpret_cast<const float*>(d); lb.L = reinterpret_cast<const float*>(d + im.off_L); lb.D = reinterpret_cast<const float*>(d + im.off_D);
    lb.M = reinterpret_cast<const uint16_t*>(d + im.off_M); lb.pal = reinterpret_cast<const uint32_t*>(d + im.off_pal);
    lb.oc = (float)(cam.offset_x / cell);
    lb.wh = e->W / 2;
    if (block_written) *block_written = true;                // (from here on the slot in blob_r may hold a partial block when the copy fails)
    HIPCHK(hipMemcpy(blob_r + trsim::lens_block_offset(blob_bytes), &lb, sizeof lb, hipMemcpyHostToDevice));
    S.pal_off = im.off_pal;
    return TRS_OK;
}

// ---- trs_load_track, step by step.  Transactional: everything is built into copies (tables, layout, parameter blocks, device buffers: a TrackStage, released
// unless moved into the handle) and committed only after every check, allocation and copy has succeeded — a failed reload leaves the handle with the track it
// had (or with none), never with new offsets against old blobs.

int track_upload(const trsim::TrackTables& T, const std::vector<unsigned char>& hp, const std::vector<unsigned char>& hr, TrackStage& S)
{
    const size_t n_points = (size_t)T.n_points;
    HIPCHK(S.blob_p.alloc(hp.size()));
    HIPCHK(S.blob_r.alloc(trsim::lens_block_offset((int)hr.size()) + sizeof(trsim::LensBlock)));   // (+ the constants of a track with elevation and of the lens camera, behind the image)
    HIPCHK(S.tangent.alloc(n_points * 8));
    HIPCHK(S.start_yaw.alloc(n_points * 4));
    HIPCHK(hipMemcpy(S.blob_p.get(), hp.data(), hp.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.blob_r.get(), hr.data(), hr.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.tangent.get(), T.tangent.data(), n_points * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.start_yaw.get(), T.start_yaw.data(), n_points * 4, hipMemcpyHostToDevice));
    HIPCHK(S.dpitch.alloc(n_points * 4));
    // the view pitch of a frame whose nearest raw track point is idx: pitch_f + dpitch[idx], ONE binary32 addition as the spec has it
    std::vector<float> vp(n_points);
    for (size_t i = 0; i < n_points; ++i) vp[i] = T.pitch_f + T.dpitch[i];
    HIPCHK(hipMemcpy(S.dpitch.get(), vp.data(), n_points * 4, hipMemcpyHostToDevice));
    return TRS_OK;
}

// the kernels' parameter blocks for the new track: copies of the handle's with the layout, the tables' constants and the staged buffers
void track_params(const trsim::TrackTables& T, const trsim::TrackLayout& L, const TrackStage& S, PParams& k, RParams& r)
{
    k.off_py = L.p.off_py; k.off_pz = L.p.off_pz; k.off_tan = L.p.off_tan; k.tan_in_lds = L.p.tan_in_lds;
    k.grid_nx = T.grid_nx; k.grid_nz = T.grid_nz; k.grid_x0 = T.grid_x0; k.grid_z0 = T.grid_z0;
    k.off_gstart = L.p.off_gstart; k.off_gpts = L.p.off_gpts; k.blob_bytes = L.p.blob_bytes; k.off_scratch = L.p.off_scratch;
    r.map_pitch_b = L.r.map_pitch_b; r.off_rowtab = L.r.off_rowtab; r.off_pal = L.r.off_pal; r.off_depth = L.r.off_depth; r.blob_bytes = L.r.blob_bytes;
    k.blob = S.blob_p.get(); k.start_yaw = S.start_yaw.get(); k.tangent_g = S.tangent.get();
    r.blob = S.blob_r.get();
    k.np = T.n_points; r.map_w = T.info.map_w; r.map_h = T.info.map_h;
    k.map_x0f = T.map_x0f; k.map_z0f = T.map_z0f; k.inv_cellf = T.inv_cellf;
}

// the lens camera, when one is set: its tables for the new map (its cell size) and its LensBlock behind the NEW raster image, before anything is committed —
// a track that leaves no LDS for the lens palette is refused like any other, and the handle keeps its track and its lens
int track_lens_stage(const trs_env* e, const trsim::TrackTables& T, const trsim::TrackLayout& L, TrackStage& S, LensStage& ls)
{
    trsim::LensBlock none{};                                 // (the slot is never read while no lens is set; defined contents all the same)
    HIPCHK(hipMemcpy(S.blob_r.get() + trsim::lens_block_offset(L.r.blob_bytes), &none, sizeof none, hipMemcpyHostToDevice));
    return e->scene.lens_on ? lens_stage(e, e->scene.camera, L.lds_step, T.info.cell, S.blob_r.get(), L.r.blob_bytes, ls) : TRS_OK;
}

// ---- commit: nothing before this has touched the handle ----
int track_commit(trs_env* e, trsim::TrackTables& T, const trsim::TrackLayout& L, TrackStage& S, const PParams& k, const RParams& r, LensStage& ls)
{
    e->track_loaded = false;                                 // (until the state arrays are in place: track_start_poses)
    e->trk = std::move(S);                                   // (the old track's buffers are released)
    trsim::HillBlock& hb = e->scene.hill;                    // the geometry half of the block behind the raster image; upload_palette sends it again with the colours
    hb = trsim::hill_geometry(T, L.r.off_sky);
    hb.vpitch = e->trk.dpitch.get(); hb.cam_pitch = e->cam_pitch.get();
    e->scene.hilly = T.hills;
    HIPCHK(hipMemcpy(e->trk.blob_r.get() + trsim::hill_block_offset(r.blob_bytes), &hb, sizeof hb, hipMemcpyHostToDevice));
    if (e->scene.lens_on) e->lens = std::move(ls);           // (the old map's tables are released)
    e->tab = std::move(T);
    e->pp = k; e->rp = r;
    e->lds_r = L.r.lds_r; e->lds_p = L.p.lds_p; e->lds_step = L.lds_step; e->lds_off_phys = L.lds_off_phys; e->pts_bytes = L.p.pts_bytes;
    return TRS_OK;
}

// start poses (host mirror of the reset branch so that telemetry is meaningful before the first step)
int track_start_poses(trs_env* e)
{
    const trsim::TrackTables& TT = e->tab;
    const PParams& k = e->pp;
    const size_t n = (size_t)e->n;
    std::vector<float> sx(n), sy(n), sz(n), syaw(n);
    std::vector<int32_t> sidx(n);
    for (size_t i = 0; i < n; ++i) {
        const int gid = e->cfg.env_id_base + (int)i;
        const int si = (int)(((long long)TRS_START_STRIDE * gid) % TT.n_points);
        sx[i] = (float)TT.px[si]; sy[i] = (float)TT.py[si]; sz[i] = (float)TT.pz[si]; syaw[i] = TT.start_yaw[si]; sidx[i] = si;
    }
    HIPCHK(hipMemcpy(k.x, sx.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(k.y, sy.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(k.z, sz.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(k.yaw, syaw.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(k.seg_idx, sidx.data(), n * 4, hipMemcpyHostToDevice));
    for (float* a : {k.v, k.speed, k.cte, k.ep_return, k.last_return, k.steer_filt}) HIPCHK(hipMemset(a, 0, n * 4));
    HIPCHK(hipMemset(k.ep_len, 0, n * 4));
    HIPCHK(hipMemset(k.done, 0, n));
    HIPCHK(hipMemset(k.pending, 1, n));
    HIPCHK(hipMemset(e->stats.get(), 0, 64 * sizeof(unsigned long long)));
    e->step_count = 0;
    e->track_loaded = true;
    trsim::resident_clear_fault(e);
    return TRS_OK;
}

// The features that were set and that the committed track has no kernel (`clash`: the dynamic-brightness filter on a track with elevation, see
// variant_refusal) or no LDS for are removed, with an error return; otherwise the palette of the new track goes up
int track_drop_misfits(trs_env* e, Variant clash)
{
    auto drop_filter = [&](int code, const char* why) {
        e->scene.drop_filter();
        (void)upload_palette(e);
        return trs_internal_fail(code, why);
    };
    const Variant v = variant_of(e);                  // (HILLS, e->lds_step: the new track's)
    if (clash == kVDyn) return drop_filter(TRS_ERR_STATE, trsim::variant_refusal(kVHills, kVDyn));
    if ((v & kVDyn) && handle_fit(e, v & ~kVLight, e->lds_step) == trsim::LdsFit::no_launch)   // (the filter alone; with lighting: below)
        return drop_filter(TRS_ERR_LIMIT, "this track leaves no LDS for the dynamic-brightness frame filter that was set: the filter has been removed");
    if ((v & kVLight) && handle_fit(e, v, e->lds_step) == trsim::LdsFit::no_launch) {
        e->scene.light_on = false; e->light = nullptr;
        (void)upload_palette(e);
        return trs_internal_fail(TRS_ERR_LIMIT, "this track leaves no LDS for the scene lighting that was set: lighting has been removed");
    }
    return upload_palette(e);                 // also sets rp.uni_rows (and applies a frame filter that was set earlier)
}
}  // namespace

TRS_EXPORT int trs_load_track(trs_env* e, const double* h_xyz, int n_points)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(e->device));
    int rc = sync_handle(e);
    if (rc) return rc;
    std::string err;
    trsim::TrackTables T;
    rc = trsim::build_tables(e->cfg, h_xyz, n_points, T, err);
    if (rc) return trs_internal_fail(rc, err);
    // the new track's HILLS bit against what is set: a lens camera refuses the track now, the dynamic-brightness filter is removed after the commit
    const Variant clash = trsim::variant_clash(variant_of(e) & ~kVHills, T.hills ? kVHills : 0u);
    if (clash == kVLens) return trs_internal_fail(TRS_ERR_STATE, trsim::variant_refusal(kVHills, clash));
    trsim::TrackLayout L;
    rc = trsim::track_layout(T, e->H, e->cfg.render != 0, e->pp.envs_per_wg, L, err);
    if (rc) return trs_internal_fail(rc, err);
    std::vector<unsigned char> hp, hr;
    trsim::pack_track_images(T, e->H, L, hp, hr);
    TrackStage S;
    if ((rc = track_upload(T, hp, hr, S))) return rc;
    PParams k = e->pp;
    RParams r = e->rp;
    track_params(T, L, S, k, r);
    if ((rc = trsim::track_kernel_attributes(e, L, T.hills))) return rc;
    LensStage ls;
    if ((rc = track_lens_stage(e, T, L, S, ls))) return rc;
    if ((rc = track_commit(e, T, L, S, k, r, ls))) return rc;
    if (e->expert) { trs_expert_free(e->expert); e->expert = nullptr; }   // the scripted expert's tables were the old track's (the handle is idle: sync_handle above)
    if ((rc = track_start_poses(e))) return rc;
    if (e->obs.on() && (rc = trsim::latency_restart(e))) return rc;  // the observations of the old track's steps do not reach the new one
    return track_drop_misfits(e, clash);
}

TRS_EXPORT int trs_map_info_get(trs_env* e, trs_map_info* o)
{
    if (!e || !o || !e->track_loaded) return trs_internal_fail(TRS_ERR_STATE, "no track loaded");
    *o = e->tab.info;
    o->lds_bytes = e->cfg.render ? e->lds_step : e->lds_p;
    return TRS_OK;
}

// ---- frame filter, camera, lighting -----------------------------------------------------------------------

TRS_EXPORT int trs_set_frame_filter(trs_env* e, const trs_pre_config* c)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (!e->cfg.render) return trs_internal_fail(TRS_ERR_STATE, "the env has no camera (cfg.render == 0)");
    if (c) {
        const char* why = nullptr;
        int rc = trsim::check_pre(c, &why);
        if (rc) return trs_internal_fail(rc, why);
        if (e->codec_quality)
            return trs_internal_fail(TRS_ERR_STATE, "a camera codec is set (trs_set_camera_codec): the fused filter would run in front of it, the reference filters the decoded frame: "
                                       "use trs_preprocess on the codec's frames");
        if (c->edge_detection_enabled) return trs_internal_fail(TRS_ERR_ARG, "the Canny layer is a neighbourhood operator: not a palette filter, use trs_preprocess");
        if (c->dynamic_brightness)
            if (const Variant set = trsim::variant_clash(variant_now(e), kVDyn)) return trs_internal_fail(TRS_ERR_STATE, trsim::variant_refusal(kVDyn, set));
        if (c->dynamic_brightness) {
            if (!trsim::dyn_filter_width_ok(e->W)) return trs_internal_fail(TRS_ERR_LIMIT, "image too wide for the in-kernel dynamic-brightness filter (class bits of the brightness rows live in 4 registers), use trs_preprocess");
            const Variant v = variant_of(e) | kVDyn;       // what the handle runs with this filter: checked without, then with, its scene lighting
            if (e->track_loaded && handle_fit(e, v & ~kVLight, e->lds_step) == trsim::LdsFit::no_launch)
                return trs_internal_fail(TRS_ERR_LIMIT, "no LDS left beside this track's tables for the in-kernel dynamic-brightness palette, use trs_preprocess");
            const trsim::LdsFit fit = e->track_loaded ? handle_fit(e, v, e->lds_step) : trsim::LdsFit::ok;
            if (fit == trsim::LdsFit::no_launch)             // (only with scene lighting: the filter alone fits)
                return trs_internal_fail(TRS_ERR_LIMIT, "no LDS left beside this track's tables for the dynamic-brightness palettes with scene lighting, use trs_preprocess");
            // resident mode: the worker keeps its env state and hand-off ring in LDS as well — refuse HERE, with the reason, what every later
            // trs_step would otherwise refuse as "too many envs per workgroup" 
            if (fit == trsim::LdsFit::no_worker)
                return trs_internal_fail(TRS_ERR_LIMIT, "the resident worker's LDS (tables + env state + hand-off ring) leaves no room for the dynamic-brightness palettes of a batch: "
                                           "select TRS_STEP_LAUNCH for this filter, or use trs_preprocess");
        }
        if (c->dynamic_brightness) { HIPCHK(hipSetDevice(e->device)); rc = upload_dyn_tables(e, *c); if (rc) return rc; }
        e->scene.filter = *c; e->scene.has_filter = true;
    } else {
        e->scene.drop_filter();
    }
    HIPCHK(hipSetDevice(e->device));
    return upload_palette(e);
}

TRS_EXPORT void trs_default_camera(trs_camera* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->struct_size = (uint32_t)sizeof *c;
}

TRS_EXPORT int trs_set_camera(trs_env* e, const trs_camera* c)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    trs_camera nc;
    trs_default_camera(&nc);
    if (c) {
        if (c->struct_size != sizeof(trs_camera)) return trs_internal_fail(TRS_ERR_ARG, "trs_camera.struct_size mismatch");
        if (!(c->fish_eye_x >= 0.0 && c->fish_eye_x <= 2.0)) return trs_internal_fail(TRS_ERR_ARG, "fish_eye_x must lie in [0, 2]");
        if (!(c->fish_eye_y >= 0.0 && c->fish_eye_y <= 2.0)) return trs_internal_fail(TRS_ERR_ARG, "fish_eye_y must lie in [0, 2]");
        if (!(c->offset_x >= -2.0 && c->offset_x <= 2.0)) return trs_internal_fail(TRS_ERR_ARG, "offset_x must lie in [-2, 2] world units");
        nc.fish_eye_x = c->fish_eye_x; nc.fish_eye_y = c->fish_eye_y; nc.offset_x = c->offset_x;
    }
    const bool on = nc.fish_eye_x != 0.0 || nc.fish_eye_y != 0.0 || nc.offset_x != 0.0;
    if (on) {
        if (!e->cfg.render) return trs_internal_fail(TRS_ERR_STATE, "the env has no camera (cfg.render == 0)");
        if (e->W % 8) return trs_internal_fail(TRS_ERR_LIMIT, "the lens camera needs an image width that is a multiple of 8 (the kernels store half of the mirror-symmetric table)");
        if (const Variant set = trsim::variant_clash(variant_now(e), kVLens)) return trs_internal_fail(TRS_ERR_STATE, trsim::variant_refusal(kVLens, set));
    }
    HIPCHK(hipSetDevice(e->device));
    // nothing may be in flight, and a resident worker leaves, BEFORE anything of the camera changes (the worker's quiesce can still launch for steps
    // posted earlier: they run with the camera they were posted under)
    { int rq = sync_handle(e); if (rq) return rq; }
    trsim::Scene& s = e->scene;
    if (on && e->track_loaded) {
        LensStage ls;
        bool block_written = false;
        int rc = lens_stage(e, nc, e->lds_step, e->tab.info.cell, e->trk.blob_r.get(), e->rp.blob_bytes, ls, &block_written);
        if (rc) {
            if (s.lens_on && block_written) {                // the copy of the block failed: the handle's LensBlock may be half written, the old lens cannot stay
                const std::string why = trs_last_error();
                e->lens = {}; s.lens_on = false; trs_default_camera(&s.camera);
                (void)upload_palette(e);
                return trs_internal_fail(rc, why + " (the lens camera that was set has been removed: the pinhole camera renders)");
            }
            return rc;                                       // (the handle is unchanged: no lens before, whose block slot is never read, or the old block untouched)
        }
        e->lens = std::move(ls);                             // (the old tables are released: nothing is in flight)
    }
    s.camera = nc; s.lens_on = on;
    if (!on) e->lens = {};                                   // back to the pinhole: the tables are not kept
    return upload_palette(e);                                // uni_rows, the lens palette with the frame filter
}

TRS_EXPORT int trs_get_camera(trs_env* e, trs_camera* out)
{
    if (!e || !out) return trs_internal_fail(TRS_ERR_ARG, "null argument");
    *out = e->scene.camera;
    out->struct_size = (uint32_t)sizeof *out;
    return TRS_OK;
}

// scene lighting (include/trsim_spec.h, "scene lighting"): register the caller's float[n_envs][8] (NULL: back to the unlit kernels)
namespace {
int set_lighting_impl(trs_env* e, const float* d_params, trsim::DevBuf<float> own = {})   // own: the host entry point's copy behind d_params, released on a refusal
{
    const bool on = d_params != nullptr;
    if (on) {
        if (!e->cfg.render) return trs_internal_fail(TRS_ERR_STATE, "the env has no camera (cfg.render == 0)");
        if (const Variant set = trsim::variant_clash(variant_now(e), kVLight)) return trs_internal_fail(TRS_ERR_STATE, trsim::variant_refusal(kVLight, set));
        const trsim::LdsFit fit = e->track_loaded ? handle_fit(e, variant_of(e) | kVLight, e->lds_step) : trsim::LdsFit::ok;   // what the handle runs with lighting
        if (fit == trsim::LdsFit::no_launch)
            return trs_internal_fail(TRS_ERR_LIMIT, "no LDS left beside this track's tables for the lit palettes");
        if (fit == trsim::LdsFit::no_worker)
            return trs_internal_fail(TRS_ERR_LIMIT, "the resident worker's LDS (tables + env state + hand-off ring) leaves no room for the lighting parameters and lit palettes: select TRS_STEP_LAUNCH");
    }
    // nothing may be in flight and a resident worker leaves before the kernels change (upload_palette quiesces too; the old host copy is freed after that)
    { int rq = sync_handle(e); if (rq) return rq; }
    e->light_own = std::move(own);                         // (the old host copy is released here, after the wait)
    e->light = d_params; e->scene.light_on = on;
    return upload_palette(e);                              // raw palette + the filter for the kernels, the parameters' address in the block behind the raster image
}
}  // namespace

TRS_EXPORT int trs_set_lighting(trs_env* e, const float* d_params)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(e->device));
    return set_lighting_impl(e, d_params);
}

TRS_EXPORT int trs_set_lighting_host(trs_env* e, const float* h_params)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(e->device));
    if (!h_params) return set_lighting_impl(e, nullptr);
    if (!e->cfg.render) return trs_internal_fail(TRS_ERR_STATE, "the env has no camera (cfg.render == 0)");
    trsim::DevBuf<float> own;
    const size_t bytes = (size_t)e->n * 8 * sizeof(float);
    HIPCHK(own.alloc(bytes));
    if (hipMemcpy(own.get(), h_params, bytes, hipMemcpyHostToDevice) != hipSuccess) return trs_internal_fail(TRS_ERR_DEVICE, "hipMemcpy of the lighting parameters failed");
    const float* d_params = own.get();
    return set_lighting_impl(e, d_params, std::move(own));
}
