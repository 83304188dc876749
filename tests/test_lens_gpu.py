"""The lens camera on the GPU (include/trsim_spec.h, "lens camera"; trs_set_camera): frames bit-exact against a restatement of the kernel formula
evaluated on the step's own poses, the physics unchanged (the oracle), every step path byte-equal to launch mode, the pinhole path untouched by an
all-zero camera, the refusals, a reload, and the gym interface's string keys.

The checker is C (a correctly rounded binary32 fmaf, -ffp-contract=off), compiled here; it reads the per-pixel table and palette of the numpy
restatement in tests/test_lens_tables_cpu.py (which checks the host builder against it bit for bit)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import track_points
from test_lens_tables_cpu import LENSES, SIZES, spec_lens_palette, spec_lens_table

pytestmark = pytest.mark.gpu

CHECKER_SRC = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>
static void spec_sincos(float a, float* so, float* co)
{
    const float q = rintf(a * 0.636619746685028076f);
    float r = fmaf(q, -1.5707963705062866211f, a);
    r = fmaf(q, 4.3711388286737928865e-08f, r);
    const float z = r * r;
    const float ps = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    const float s = fmaf(r * z, ps, r);
    const float pc = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    const float c = fmaf(z * z, pc, fmaf(z, -0.5f, 1.0f));
    switch (((int)q) & 3) { case 0: *so = s; *co = c; break; case 1: *so = c; *co = -s; break; case 2: *so = -s; *co = -c; break; default: *so = -c; *co = s; }
}
static int clampi(float g, int n) { return g < 0.0f ? 0 : (g >= (float)(n - 1) ? n - 1 : (int)g); }   /* clamp((int)floor(g), 0, n-1) */
void lens_render(int n, int H, int W, const float* x, const float* z, const float* yaw, float cam_fwd, float x0f, float z0f, float inv_cell, float oc,
                 const float* tab, const uint32_t* pal, const uint32_t* map, int gw, int gh, int mw, uint8_t* img, float* dep)
{
    for (int e = 0; e < n; ++e) {
        float s, c;
        spec_sincos(yaw[e], &s, &c);
        const float camx = ((x[e] + cam_fwd * s) - x0f) * inv_cell, camz = ((z[e] + cam_fwd * c) - z0f) * inv_cell;
        const float cx = fmaf(oc, c, camx), cz = fmaf(oc, -s, camz);
        for (int p = 0; p < H * W; ++p) {
            const float F = tab[4 * p], L = tab[4 * p + 1];
            uint32_t row;
            memcpy(&row, &tab[4 * p + 3], 4);
            const float gx = fmaf(L, c, fmaf(F, s, cx)), gz = fmaf(L, -s, fmaf(F, c, cz));
            const int ix = clampi(gx, gw), iz = clampi(gz, gh);
            const uint32_t cls = (map[(size_t)iz * mw + (ix >> 4)] >> (2 * (ix & 15))) & 3u;
            const uint32_t rgb = pal[4 * row + cls];
            uint8_t* o = img + ((size_t)e * H * W + p) * 3;
            o[0] = rgb & 255u; o[1] = (rgb >> 8) & 255u; o[2] = (rgb >> 16) & 255u;
            dep[(size_t)e * H * W + p] = tab[4 * p + 2];
        }
    }
}
"""


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    d = tmp_path_factory.mktemp("lens_checker")
    (d / "checker.c").write_text(CHECKER_SRC)
    so = d / "checker.so"
    subprocess.check_call([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so), str(d / "checker.c"), "-lm"])
    lib = C.CDLL(str(so))
    fp = C.c_float
    lib.lens_render.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, fp, fp, fp, fp, fp,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.lens_render.restype = None
    return lib


_TABLES = {}


def expected_frames(checker, env, lens, filt=None):
    """(img, depth) the checker renders from the env's CURRENT poses (x, z, yaw) and map with the spec's tables for `lens`."""
    mi = env.map_info
    key = (env.H, env.W, mi.cell, lens[0], lens[1])
    if key not in _TABLES:
        _TABLES[key] = np.ascontiguousarray(spec_lens_table(env.H, env.W, mi.cell, lens[0], lens[1]))
    tab = _TABLES[key]
    pal = np.ascontiguousarray(spec_lens_palette() if filt is None else filt)
    x, z, yaw = (np.ascontiguousarray(env.fetch(k)) for k in ("pos_x", "pos_z", "yaw"))
    mp = np.ascontiguousarray(env.fetch("map"))
    img = np.zeros((env.n, env.H, env.W, 3), np.uint8)
    dep = np.zeros((env.n, env.H, env.W), np.float32)
    f32 = np.float32
    checker.lens_render(env.n, env.H, env.W, x.ctypes.data, z.ctypes.data, yaw.ctypes.data, f32(env.cfg.cam_fwd), f32(mi.x0), f32(mi.z0),
                        f32(1.0 / mi.cell), f32(lens[2] / mi.cell), tab.ctypes.data, pal.ctypes.data, mp.ctypes.data, mi.map_w, mi.map_h, mi.map_words,
                        img.ctypes.data, dep.ctypes.data)
    return img, dep


def assert_frames(checker, env, lens, depth=True):
    img, dep = expected_frames(checker, env, lens)
    got = env.fetch("img")
    bad = np.argwhere((got != img).any(-1))
    assert bad.size == 0, f"{len(bad)} pixels differ from the checker, first {bad[:4].tolist()}"
    if depth:
        assert np.array_equal(env.fetch("depth").view(np.uint32), dep.view(np.uint32))


def controls(n, t):
    return np.sin(np.linspace(0, 3, n, dtype=np.float32) + 0.3 * t).astype(np.float32) * 0.6, np.full(n, 0.7, np.float32)


@pytest.mark.parametrize("lens", LENSES)
@pytest.mark.parametrize("shape", SIZES)
def test_launch_frames_and_physics(make_env, checker, shape, lens):
    H, W = shape
    n = 8
    env = make_env("hip", n_envs=n, img_h=H, img_w=W, depth=True, auto_reset=True)
    ref = make_env("oracle", n_envs=n, img_h=H, img_w=W, depth=True, auto_reset=True)
    env.set_camera(*lens)
    assert env.camera() == tuple(float(v) for v in lens)
    tab = env.fetch("lens_table")
    want = spec_lens_table(H, W, env.map_info.cell, lens[0], lens[1])
    assert np.array_equal(tab.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(env.fetch("lens_palette"), spec_lens_palette())
    for t in range(3):
        st, th = controls(n, t)
        for e in (env, ref):
            e.step(st, th)
        assert_frames(checker, env, lens)
    for e in (env, ref):
        e.step_synthetic(5, 1)
    assert_frames(checker, env, lens)
    for name in ("seg_idx", "done", "ep_len"):
        assert np.array_equal(env.fetch(name), ref.fetch(name)), name
    for name in ("pos_x", "pos_y", "pos_z", "speed", "cte", "yaw"):
        assert np.max(np.abs(env.fetch(name) - ref.fetch(name))) <= 1e-5, name


def frames(env):
    return env.fetch("img"), env.fetch("depth")


@pytest.mark.parametrize("shape", [(120, 160), (240, 320)])
def test_resident_sequence_synthetic_equal_launch(make_env, shape):
    H, W = shape
    n = 16
    lens = (1.5, 0.3, 0.4)
    a = make_env("hip", n_envs=n, img_h=H, img_w=W, depth=True, auto_reset=True, camera=lens)
    b = make_env("hip", n_envs=n, img_h=H, img_w=W, depth=True, auto_reset=True, camera=dict(fish_eye_x=1.5, fish_eye_y=0.3, offset_x=0.4))
    b.set_step_mode(True)
    for t in range(6):                                                 # resident posts vs launches
        st, th = controls(n, t)
        a.step(st, th); b.step(st, th)
        fa, fb = frames(a), frames(b)
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1].view(np.uint32), fb[1].view(np.uint32)), t
    b.set_step_mode(False)
    seq_st = np.stack([controls(n, t)[0] for t in range(6, 16)])
    seq_th = np.stack([controls(n, t)[1] for t in range(6, 16)])
    a.step_sequence(seq_st, seq_th, steps_per_launch=4)                # several steps per launch (the raster team one step behind)
    for k in range(10):
        b.step(seq_st[k], seq_th[k])
    assert np.array_equal(a.fetch("img"), b.fetch("img")) and np.array_equal(a.fetch("depth"), b.fetch("depth"))
    a.step_synthetic(12, 4)
    b.step_synthetic(12, 1)
    assert np.array_equal(a.fetch("img"), b.fetch("img")) and np.array_equal(a.fetch("depth"), b.fetch("depth"))
    b.set_step_mode(True)                                              # synthetic controls through the worker
    a.step_synthetic(3, 1); b.step_synthetic(3, 1)
    assert np.array_equal(a.fetch("img"), b.fetch("img")) and np.array_equal(a.fetch("depth"), b.fetch("depth"))


def test_pilot_loop_through_a_lens(make_env, checker):
    from test_pilot_trained import trained_weights
    n = 32
    lens = (0.8, 0.4, 0.3)
    env = make_env("hip", n_envs=n, img_h=120, img_w=160, auto_reset=True, camera=lens)
    env.pilot_load(trained_weights())
    env.step_pilot(20, {"spd_ctl_threshold": 1.1, "spd_ctl_reverse_multiplier": 1.0})
    assert float(env.fetch("speed").mean()) > 0.5                      # the pilot drives (it sees frames)
    assert_frames(checker, env, lens, depth=False)


def test_static_filter_on_lens_frames_equals_the_oracle_preprocess(make_env):
    n, H, W = 8, 120, 160
    lens = (1.5, 0.3, 0.4)
    filt = {"preprocessing_contrast_enhancement_ratio": 1.4, "preprocessing_contrast_enhancement_offset": 110.0, "preprocessing_color_filter_enabled": True}
    raw = make_env("hip", n_envs=n, img_h=H, img_w=W, camera=lens)
    flt = make_env("hip", n_envs=n, img_h=H, img_w=W, camera=lens)
    flt.set_frame_filter(filt)
    ora = make_env("oracle", n_envs=n, img_h=H, img_w=W, track=None, render=True)
    for t in range(4):
        st, th = controls(n, t)
        raw.step(st, th); flt.step(st, th)
    want = ora.preprocess_host(raw.fetch("img"), filt)
    assert np.array_equal(flt.fetch("img"), want)
    flt.set_step_mode(True)
    raw.set_step_mode(True)
    st, th = controls(n, 9)
    raw.step(st, th); flt.step(st, th)
    assert np.array_equal(flt.fetch("img"), ora.preprocess_host(raw.fetch("img"), filt))


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("off", [None, (0.0, 0.0, 0.0)])
def test_pinhole_camera_is_byte_identical(make_env, resident, off):
    n = 16
    a = make_env("hip", n_envs=n, depth=True, auto_reset=True)
    b = make_env("hip", n_envs=n, depth=True, auto_reset=True)
    b.set_camera(1.0, 1.0, 0.5)
    b.step_synthetic(2, 1)
    if off is None:
        b.set_camera(None)
    else:
        b.set_camera(*off)
    b.reset(np.ones(n, np.uint8)); a.reset(np.ones(n, np.uint8))
    if resident:
        a.set_step_mode(True); b.set_step_mode(True)
    for t in range(32):
        st, th = controls(n, t)
        a.step(st, th); b.step(st, th)
        assert np.array_equal(a.fetch("img"), b.fetch("img")), t
        assert np.array_equal(a.fetch("depth").view(np.uint32), b.fetch("depth").view(np.uint32)), t
    assert b.camera() == (0.0, 0.0, 0.0)


def test_refusals_leave_the_handle_working(make_env, checker):
    from triton_racer_sim_amd import _ffi
    n = 8
    lens = (0.5, 0.5, 0.0)
    env = make_env("hip", n_envs=n, auto_reset=True, camera=lens)
    for bad in [(2.5, 0.0, 0.0), (0.0, -0.1, 0.0), (0.0, 0.0, 2.5), (float("nan"), 0.0, 0.0)]:
        with pytest.raises(RuntimeError, match="must lie in"):
            env.set_camera(*bad)
        assert env.camera() == lens
    with pytest.raises(RuntimeError, match="elevation"):               # a hilly track while a lens is set: refused, the old track stays
        env.load_track(track_points("mountain"))
    with pytest.raises(RuntimeError, match="dynamic-brightness"):
        env.set_frame_filter({"preprocessing_dynamic_brightness_enabled": True})
    env.step(*controls(n, 0))
    assert_frames(checker, env, lens, depth=False)
    # the other order: a hilly track first, then a lens; the dynamic-brightness filter first, then a lens
    hilly = make_env("hip", n_envs=n, track=track_points("mountain"), depth=True)
    fresh = make_env("hip", n_envs=n, track=track_points("mountain"), depth=True)
    with pytest.raises(RuntimeError, match="elevation"):
        hilly.set_camera(*lens)
    assert hilly.camera() == (0.0, 0.0, 0.0)
    for t in range(3):                                                 # the refused call changed nothing: the same frames and state as a handle never asked
        hilly.step(*controls(n, t)); fresh.step(*controls(n, t))
        for name in ("img", "depth", "pos_x", "pos_z", "yaw", "seg_idx"):
            assert np.array_equal(hilly.fetch(name), fresh.fetch(name)), (t, name)
    dyn = make_env("hip", n_envs=n, auto_reset=True)
    dyn.set_frame_filter({"preprocessing_dynamic_brightness_enabled": True})
    with pytest.raises(RuntimeError, match="dynamic-brightness"):
        dyn.set_camera(*lens)
    dyn.set_frame_filter(None)
    dyn.set_camera(*lens)
    dyn.step(*controls(n, 1))
    assert_frames(checker, dyn, lens, depth=False)
    cam = _ffi.TrsCamera()
    cam.struct_size = 4
    assert env.api.set_camera(env._h, C.byref(cam)) == -1


def test_reload_of_a_flat_track_rebuilds_the_lens_tables(make_env, checker):
    n = 8
    lens = (1.5, 0.3, 0.4)
    env = make_env("hip", n_envs=n, depth=True, auto_reset=True, camera=lens)
    env.step(*controls(n, 0))
    assert_frames(checker, env, lens)
    pts = track_points("generated").copy()
    pts[:, 0] = pts[:, 0] * 1.25 + 7.0                                 # another flat track: a different map and corner
    pts[:, 2] = pts[:, 2] * 1.25 - 3.0
    env.load_track(pts)
    for t in range(3):
        env.step(*controls(n, t))
        assert_frames(checker, env, lens)


def test_gym_interface_string_keys(make_env):
    from triton_racer_sim_amd.components import HipGymInterface
    gym = HipGymInterface(gym_config={"fish_eye_x": "0.8", "fish_eye_y": "0.4", "offset_x": "0.3"})
    env = make_env("hip", n_envs=1, camera=(0.8, 0.4, 0.3))
    assert gym.env.camera() == (0.8, 0.4, 0.3)
    for t in range(3):
        out = gym.step(0.2, 0.6, 0.0, False)
        env.step(0.2, 0.6)
    assert np.array_equal(np.asarray(out[0]), env.fetch("img")[0])
    gym.onShutdown()
    plain = HipGymInterface(gym_config={"fish_eye_x": 0, "offset_x": "0"})
    assert plain.env.camera() == (0.0, 0.0, 0.0)
    plain.onShutdown()


def long_flat_track():
    """The mountain track's 2664 points with their height removed: a flat track whose tables leave a 1024-env step kernel room for the pinhole
    camera's hand-off ring but none for the lens camera's palette."""
    pts = track_points("mountain").copy()
    pts[:, 1] = 0.0
    return pts


def test_reload_onto_a_track_without_room_for_the_lens(make_env, checker):
    n = 1024
    lens = (0.8, 0.4, 0.3)
    env = make_env("hip", n_envs=n, auto_reset=True, camera=lens)
    twin = make_env("hip", n_envs=n, auto_reset=True, camera=lens)
    env.step(*controls(n, 0)); twin.step(*controls(n, 0))
    mi = (env.map_info.map_w, env.map_info.map_h, env.map_info.cell)
    with pytest.raises(RuntimeError, match="lens camera"):
        env.load_track(long_flat_track())
    # refused as a whole: the old track, map and lens tables stay, and the handle steps as its twin does
    info = env.api.map_info_get
    from triton_racer_sim_amd import _ffi
    got = _ffi.TrsMapInfo()
    env.api.check(info(env._h, C.byref(got)), "map_info_get")
    assert (got.map_w, got.map_h, got.cell, got.n_points) == mi + (len(track_points("generated")),)
    assert env.camera() == lens
    assert np.array_equal(env.fetch("lens_table").view(np.uint32), spec_lens_table(env.H, env.W, mi[2], lens[0], lens[1]).view(np.uint32))
    for t in range(1, 4):
        env.step(*controls(n, t)); twin.step(*controls(n, t))
        assert np.array_equal(env.fetch("img"), twin.fetch("img")), t
        for name in ("pos_x", "pos_z", "yaw", "seg_idx", "done"):
            assert np.array_equal(env.fetch(name), twin.fetch(name)), (t, name)
    assert_frames(checker, env, lens, depth=False)


def test_lens_refused_where_its_palette_does_not_fit(make_env):
    n = 1024
    env = make_env("hip", n_envs=n, auto_reset=True, track=long_flat_track())
    twin = make_env("hip", n_envs=n, auto_reset=True, track=long_flat_track())
    with pytest.raises(RuntimeError, match="no LDS left"):
        env.set_camera(0.8, 0.4, 0.3)
    assert env.camera() == (0.0, 0.0, 0.0)
    for t in range(3):
        env.step(*controls(n, t)); twin.step(*controls(n, t))
        assert np.array_equal(env.fetch("img"), twin.fetch("img")), t


def test_camera_changes_reach_a_running_resident_worker(make_env, checker):
    """One handle in resident mode: pinhole steps, then a lens set while the worker runs (frames = the checker), then the pinhole again (frames
    byte-equal to a handle that never had a lens).  The worker is relaunched with each camera; its register-held table rows with it."""
    n = 16
    lens = (1.5, 0.3, 0.4)
    ref = make_env("hip", n_envs=n, depth=True, auto_reset=True)
    env = make_env("hip", n_envs=n, depth=True, auto_reset=True)
    env.set_step_mode(True)
    t = 0
    for _ in range(3):
        ref.step(*controls(n, t)); env.step(*controls(n, t)); t += 1
        assert np.array_equal(env.fetch("img"), ref.fetch("img"))
    env.set_camera(*lens)
    for _ in range(4):
        ref.step(*controls(n, t)); env.step(*controls(n, t)); t += 1
        assert_frames(checker, env, lens)
        for name in ("pos_x", "pos_z", "yaw", "seg_idx"):
            assert np.array_equal(env.fetch(name), ref.fetch(name)), name
    assert env.step_mode()[0] == "resident"
    env.set_camera(None)
    for _ in range(4):
        ref.step(*controls(n, t)); env.step(*controls(n, t)); t += 1
        assert np.array_equal(env.fetch("img"), ref.fetch("img"))
        assert np.array_equal(env.fetch("depth").view(np.uint32), ref.fetch("depth").view(np.uint32))
    with pytest.raises(RuntimeError, match="field not available"):
        env.fetch("lens_table")                                        # back to the pinhole: the lens tables are freed
    assert env.step_mode()[0] == "resident"


def test_a_lens_set_over_a_lens_renders_like_a_handle_that_set_only_that_camera(make_env):
    """lens A -> lens B (another offset_x) -> pinhole -> lens A -> a reload with lens A set, two steps each: after every step the frames are those of a twin
    that took the same steps under the pinhole camera and set only the stage's camera where the stage begins (the camera does not enter the physics),
    and while a lens is on both handles hold the same table and palette.  Every stage replaces or releases the tables of the one before."""
    n, H, W = 3, 30, 48
    pts = track_points("generated")
    A, B = (1.5, 0.3, 0.4), (0.6, 1.1, -0.7)
    kw = dict(n_envs=n, img_h=H, img_w=W, depth=True, track=pts, auto_reset=True)
    env = make_env("hip", **kw)

    def same(a, b, where, lens):
        for name in ("img", "depth", "pos_x", "pos_z", "yaw", "seg_idx"):
            assert np.array_equal(a.fetch(name), b.fetch(name)), (where, name)
        if lens:
            for name in ("lens_table", "lens_palette"):
                assert np.array_equal(a.fetch(name).view(np.uint32), b.fetch(name).view(np.uint32)), (where, name)

    t = 0
    for stage, lens in enumerate((A, B, None, A)):
        twin = make_env("hip", **kw)
        for k in range(t):
            twin.step(*controls(n, k))
        for e in (env, twin):
            e.set_camera(*lens) if lens else e.set_camera(None)
        assert env.camera() == (lens or (0.0, 0.0, 0.0))
        for _ in range(2):
            env.step(*controls(n, t)); twin.step(*controls(n, t)); t += 1
            same(env, twin, (stage, t), lens)
    env.load_track(pts)                                                # lens A is set: its tables are staged for the new map and replace the old ones
    twin = make_env("hip", camera=A, **kw)
    assert env.camera() == A
    for k in range(2):
        env.step(*controls(n, k)); twin.step(*controls(n, k))
        same(env, twin, ("reload", k), A)
