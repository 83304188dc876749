"""Every HIP step path on all branches of "one env step" (include/trsim_spec.h) and with the camera outside the class map.

Two kinds of input are legal through the public API and reached a kernel in no other GPU test: reverse driving, stopping by drag or brake, the two
speed clamps, both yaw wraps, both reward wraps across the start line and `lost` (part A); and frames whose ground lookups fall outside the grid and
clamp onto the grass border, with the nearest-point block search at fx = -1 / nx, its fall back to the full scan, and the lost result (part B).

Part A runs the scenario of test_independent_spec.py::test_physics_steps_against_a_numpy_restatement (the same start poses and controls, drawn in the
same order) through the physics-only kernels (the SEL form of env_advance), the step kernels, the resident workers and the HILLS instantiation, beside
the oracle, and counts on the ORACLE's states, with that test's numpy_step, that all twelve branch keys were really hit.  Part B places 32 cars on four
rings around the track's bounding box and compares every raster implementation's frames with its reference.  The two coverage tests carry no gpu mark:
they pin, on the oracle alone, that the inputs are what they claim to be.

Any change to env_advance, wave_nearest or a raster lookup (its clamps included) has to pass this file."""
import math

import numpy as np
import pytest

from conftest import track_points
from test_gpu_parity import FLOATS, assert_state_equal
from test_image_path import DYNAMIC, FUSED
from test_independent_spec import fetch_state, numpy_step, spec_tangents
from test_lens_gpu import checker, expected_frames  # noqa: F401  (checker is a fixture)
from test_lens_tables_cpu import LENSES
from test_lighting_gpu import light_frames

gpu = pytest.mark.gpu
F = np.float32

NEED = ("reverse", "stopped_by_drag", "brake", "clamp_vmax", "clamp_vrev", "yaw_wrap_down", "yaw_wrap_up", "reward_wrap_fwd", "reward_wrap_back",
        "lost", "done", "reset")
# With the default parameters each speed clamp is reachable from the start pose only (v drawn beyond it); the tight set reaches both every few steps.
PARAM_SETS = {"defaults": {}, "tight": dict(v_max=6.0, v_rev_max=1.0, drag_lin=0.1)}
SEED, N_ENVS, STEPS = 8, 64, 30
SEQ_K = 7                                      # steps per launch of the sequence paths: 30 steps = four full launches and a ragged one
_TANGENTS = {}


def tangents(track):
    if track not in _TANGENTS:
        _TANGENTS[track] = spec_tangents(track_points(track))
    return _TANGENTS[track]


# ---------------------------------------------------------------------------------------------------------------- A: the branch scenario

def branch_scenario(track, seed=SEED, n=N_ENVS, steps=STEPS):
    """Start poses and controls of test_independent_spec.py::test_physics_steps_against_a_numpy_restatement, drawn in that test's order: cars near
    random track points (eight at the first and last points), headings along or against the track +- 0.3 rad, eight headings at +- 3.14, v in -6 .. 27,
    four cars at x + 500 (lost); steer in +- 1.3, thr in +- 1.2, brk > 0 on 30 % of the envs, full throttle / full reverse for envs 0-15 / 16-23 in the
    steps t % 10 < 3, a 4 % user reset.  Controls and resets are [steps, n]."""
    pts = track_points(track)
    tang = tangents(track)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(pts), n)
    k[:8] = [0, 1, 2, len(pts) - 1, len(pts) - 2, len(pts) - 3, 3, len(pts) - 4]
    x = (pts[k, 0] + rng.uniform(-1.0, 1.0, n)).astype(F); z = (pts[k, 2] + rng.uniform(-1.0, 1.0, n)).astype(F)
    tz_yaw = np.arctan2(tang[k, 0], tang[k, 1])
    yaw = (tz_yaw + rng.choice([0.0, math.pi], n) + rng.uniform(-0.3, 0.3, n)).astype(np.float64)
    yaw = ((yaw + math.pi) % (2 * math.pi) - math.pi).astype(F)
    yaw[8:16] = F(3.14) * rng.choice([-1, 1], 8).astype(F)
    v = rng.uniform(-6.0, 27.0, n).astype(F)
    x[n - 4:] += F(500.0)
    steer, thr, brk = (np.zeros((steps, n), F) for _ in range(3))
    reset = np.zeros((steps, n), np.uint8)
    for t in range(steps):
        steer[t] = rng.uniform(-1.3, 1.3, n)
        thr[t] = rng.uniform(-1.2, 1.2, n)
        brk[t] = np.where(rng.random(n) < 0.3, rng.uniform(0.0, 1.2, n), 0.0)
        if t % 10 < 3:
            thr[t, :16] = 1.0; brk[t, :16] = 0.0
            thr[t, 16:24] = -1.0; brk[t, 16:24] = 0.0
        reset[t] = rng.random(n) < 0.04
    return dict(track=track, pts=pts, tang=tang, n=n, steps=steps, x=x, z=z, yaw=yaw, v=v, steer=steer, thr=thr, brk=brk, reset=reset)


def place(env, sc):
    env.step(0.0, 0.0)                                                  # consumes the pending reset: every env on its start pose (y, seg_idx)
    env.set_pose(x=sc["x"], z=sc["z"], yaw=sc["yaw"], v=sc["v"])


def count_step(seen, ora, sc, t, reset):
    """Hits of the branch keys in the step the oracle is about to take (numpy_step on the oracle's own state)."""
    _, hit = numpy_step(ora.cfg, sc["pts"], sc["tang"], fetch_state(ora), sc["steer"][t], sc["thr"][t], sc["brk"][t], reset.astype(bool))
    for key, mask in hit.items():
        seen[key] = seen.get(key, 0) + int(np.count_nonzero(mask))


def resets_of(sc, t, sequence):
    """A step sequence takes ONE reset mask, applied at its first step (trs_step_sequence): the scenario's first, and none after it."""
    return sc["reset"][t] if (not sequence or t == 0) else np.zeros(sc["n"], np.uint8)


def assert_all_keys(seen, where):
    missing = [k for k in NEED if seen.get(k, 0) == 0]
    assert not missing, (where, missing, seen)


_MAXDIFF = {}


def compare(g, o, where, path, frames=False, depth=False):
    """Integers, flags and frame bytes bit for bit; the float fields at the project's 1e-5 (a yaw off by 2 pi is far outside it).  Records the largest
    float difference per path."""
    d = max(float(np.max(np.abs(g.fetch(k).astype(np.float64) - o.fetch(k).astype(np.float64)))) for k in FLOATS)
    _MAXDIFF[path] = max(_MAXDIFF.get(path, 0.0), d)
    assert_state_equal(g, o, where)
    if frames:
        a, b = g.fetch("img"), o.fetch("img")
        bad = np.argwhere((a != b).any(-1))
        assert bad.size == 0, f"{where}: {len(bad)} pixels differ, first (env, v, u) {bad[:4].tolist()}"
    if depth:
        a, b = g.fetch("depth").view(np.uint32), o.fetch("depth").view(np.uint32)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{where}: {len(bad)} depth words differ, first (env, v, u) {bad[:4].tolist()}"


def run_branch_path(make_env, track, params, auto_reset, mode, render, depth=False):
    """One step path beside the oracle on the branch scenario.  mode: 'step' (one trs_step per call), 'sequence' (one trs_step_sequence call,
    SEQ_K steps per launch) or 'resident' (posted to the worker kernel)."""
    sc = branch_scenario(track)
    path = f"{'rendered' if render else 'physics'}{'+depth' if depth else ''}/{mode}/{track}"
    kw = dict(n_envs=sc["n"], track=sc["pts"], render=render, depth=depth, auto_reset=auto_reset, **PARAM_SETS[params])
    g, o = make_env("hip", **kw), make_env("oracle", **kw)
    for env in (g, o):
        place(env, sc)
    seen = {}
    if mode == "sequence":
        walk = make_env("oracle", **kw)                                 # the same steps one at a time, to count on: it must end where the sequence call does
        place(walk, sc)
        for t in range(sc["steps"]):
            rs = resets_of(sc, t, True)
            count_step(seen, walk, sc, t, rs)
            walk.step(sc["steer"][t], sc["thr"][t], sc["brk"][t], reset=rs)
        for env in (g, o):
            env.step_sequence(sc["steer"], sc["thr"], sc["brk"], reset=sc["reset"][0], steps_per_launch=SEQ_K)
        for name in ("pos_x", "pos_y", "pos_z", "yaw", "vel", "cte", "ep_return", "last_return", "seg_idx", "done", "ep_len") + (("img",) if render else ()):
            assert np.array_equal(walk.fetch(name), o.fetch(name)), f"oracle: sequence call != single steps ({name})"
        compare(g, o, f"{path} after {sc['steps']} steps", path, render, depth)
    else:
        if mode == "resident":
            g.set_step_mode(True)
        for t in range(sc["steps"]):
            count_step(seen, o, sc, t, sc["reset"][t])
            for env in (g, o):
                env.step(sc["steer"][t], sc["thr"][t], sc["brk"][t], reset=sc["reset"][t])
            compare(g, o, f"{path} step {t}", path, render, depth)
        if mode == "resident":
            assert int(g.fetch("stats")[2]) == 0                        # no layout fault: the worker really ran
    assert_all_keys(seen, path)
    print(f"[step branches] {path} {params} auto_reset={auto_reset}: largest float difference {_MAXDIFF[path]:.3g}; hits {seen}")


@pytest.mark.parametrize("sequence", [False, True])
@pytest.mark.parametrize("params", list(PARAM_SETS))
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("track", ["generated", "mountain"])
def test_scenario_covers_every_branch_on_the_oracle(make_env, track, auto_reset, params, sequence):
    """The scenario hits what it claims, on the oracle alone, fed as single steps and as a step sequence (resets at the first step only).  Counts with
    seed 8, 30 steps, 64 envs, single steps — defaults: clamp_vmax 1, clamp_vrev 2 (start poses only), every other key >= 8; tight: clamp_vmax 103-122,
    clamp_vrev 55, every other key >= 4.  The test prints what it counts."""
    sc = branch_scenario(track)
    env = make_env("oracle", n_envs=sc["n"], track=sc["pts"], render=False, auto_reset=auto_reset, **PARAM_SETS[params])
    place(env, sc)
    seen = {}
    for t in range(sc["steps"]):
        rs = resets_of(sc, t, sequence)
        count_step(seen, env, sc, t, rs)
        env.step(sc["steer"][t], sc["thr"][t], sc["brk"][t], reset=rs)
    print(f"[step branches] {track} auto_reset={auto_reset} {params} sequence={sequence}: {seen}")
    assert_all_keys(seen, (track, auto_reset, params, sequence))
    if params == "tight":
        assert seen["clamp_vmax"] >= 50 and seen["clamp_vrev"] >= 20, seen


@gpu
@pytest.mark.parametrize("mode", ["step", "sequence", "resident"])
@pytest.mark.parametrize("params", list(PARAM_SETS))
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("track", ["generated", "mountain"])
def test_physics_only_paths_on_every_branch(make_env, track, auto_reset, params, mode):
    """render=False: trs_physics_kernel (one step per call, and SEQ_K steps per launch) and trs_physics_worker_kernel — the SEL form of env_advance,
    spec_sincos_sel and wave_nearest<true>."""
    run_branch_path(make_env, track, params, auto_reset, mode, render=False)


@gpu
@pytest.mark.parametrize("mode", ["step", "sequence", "resident"])
@pytest.mark.parametrize("params", list(PARAM_SETS))
@pytest.mark.parametrize("auto_reset", [False, True])
def test_rendered_paths_on_every_branch(make_env, auto_reset, params, mode):
    """120x160 frames: trs_step_kernel (one step per call, and SEQ_K steps per launch) and trs_worker_kernel — the branchy env_advance, every frame byte."""
    run_branch_path(make_env, "generated", params, auto_reset, mode, render=True)


@gpu
@pytest.mark.parametrize("mode", ["step", "resident"])
def test_hills_paths_on_every_branch(make_env, mode):
    """The HILLS instantiations: the view pitch follows idx — idx = 0 of a lost car included — and the depth frame differs from env to env."""
    run_branch_path(make_env, "mountain", "tight", True, mode, render=True, depth=True)


# ---------------------------------------------------------------------------------------------------------------- B: off-map poses

RING_OUTSIDE = (2.0, 6.0, 60.0)                # rings 1-3: world units outside the bounding box of the raw points, looking at its centre
RING_FAR = 1500.0                              # ring 4: world units from the centre, looking away
COMPASS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))   # N, NE, E, ... as (x, z) signs
OFFMAP_STEPS = 4


def ring_poses(pts):
    """32 poses: env 8 r + j is on ring r + 1 in compass direction j.  All within +- 2000 world units: the oracle's (int)floor(g) is defined while
    |g| < 2^31 cells, and the smallest cell is 0.125."""
    xmin, xmax, zmin, zmax = pts[:, 0].min(), pts[:, 0].max(), pts[:, 2].min(), pts[:, 2].max()
    cx, cz, hx, hz = 0.5 * (xmin + xmax), 0.5 * (zmin + zmax), 0.5 * (xmax - xmin), 0.5 * (zmax - zmin)
    x, z, yaw = [], [], []
    for d in RING_OUTSIDE:
        for sx, sz in COMPASS:
            px, pz = cx + sx * (hx + d), cz + sz * (hz + d)
            x.append(px); z.append(pz); yaw.append(math.atan2(cx - px, cz - pz))       # forward = (sin yaw, cos yaw) in (x, z)
    for sx, sz in COMPASS:
        r = RING_FAR / math.hypot(sx, sz)
        x.append(cx + sx * r); z.append(cz + sz * r); yaw.append(math.atan2(sx, sz))
    x, z, yaw = np.asarray(x, F), np.asarray(z, F), np.asarray(yaw, F)
    assert max(np.abs(x).max(), np.abs(z).max()) < 2000.0
    return x, z, yaw


def offmap_controls(t, n):
    """Step 0: the cars reverse; then steer and throttle alternate +- 1."""
    if t == 0:
        return np.zeros(n, F), np.full(n, -1.0, F)
    s = F(1.0 if t % 2 else -1.0)
    return np.full(n, s, F), np.full(n, s, F)


def place_rings(env, pts):
    x, z, yaw = ring_poses(pts)
    env.step(0.0, 0.0)
    env.set_pose(x=x, z=z, yaw=yaw, v=np.zeros(len(x), F))


@pytest.mark.parametrize("track", ["generated", "mountain"])
def test_ring_poses_are_what_they_claim_on_the_oracle(make_env, track):
    """Rings 3 and 4 see nothing but the clamped border (every image row one colour); rings 1 and 2 see the map from outside; ring 4 is lost, ring 3
    is half lost and half found by the full scan (far from every point, but under 100 L1), rings 1 and 2 are found."""
    pts = track_points(track)
    env = make_env("oracle", n_envs=32, track=pts, auto_reset=False)
    place_rings(env, pts)
    env.step(*offmap_controls(0, 32))
    img = env.fetch("img")
    mixed = (img != img[:, :, :1]).any((2, 3)).any(1)                   # per env: some row holds more than one colour
    seg, done = env.fetch("seg_idx"), env.fetch("done")
    lost = [int(((seg[8 * r:8 * r + 8] == 0) & (done[8 * r:8 * r + 8] != 0)).sum()) for r in range(4)]
    print(f"[off-map rings] {track}: envs with a mixed row per ring {[int(mixed[8 * r:8 * r + 8].sum()) for r in range(4)]}, lost per ring {lost}")
    assert not mixed[16:].any(), np.flatnonzero(mixed[16:]) + 16
    assert mixed[0:8].sum() >= 5 and mixed[8:16].sum() >= 5
    assert lost == [0, 0, 4, 8]
    assert [int((seg[8 * r:8 * r + 8] == 0).sum()) for r in range(4)] == [0, 0, 4, 8]
    # the nearest-point search of ring 3's found cars is the full scan: no point within one TRS_NEAR_GRID_CELL
    x, y, z = env.fetch("pos_x").astype(np.float64), env.fetch("pos_y").astype(np.float64), env.fetch("pos_z").astype(np.float64)
    best = (np.abs(x[:, None] - pts[None, :, 0]) + np.abs(y[:, None] - pts[None, :, 1]) + np.abs(z[:, None] - pts[None, :, 2])).min(1)
    assert (best[16:24] >= 4.0).all() and ((best[16:24] < 100.0).sum() == 4) and (best[24:] >= 100.0).all()


OFFMAP_VARIANTS = {
    "rgb": dict(),
    "depth": dict(depth=True),
    "240x320+depth": dict(img_h=240, img_w=320, depth=True),
    "64x64": dict(img_h=64, img_w=64),
    "static filter": dict(filt=FUSED[1]),
    "dynamic brightness": dict(filt=DYNAMIC[0]),
    "lighting": dict(light=True),
    "lens": dict(lens=next(l for l in LENSES if l[2] != 0.0), depth=True),
    "hills+depth": dict(track="mountain", depth=True),
}


@gpu
@pytest.mark.parametrize("resident", [False, True], ids=["launches", "resident"])
@pytest.mark.parametrize("variant", list(OFFMAP_VARIANTS))
def test_offmap_frames(make_env, request, variant, resident):
    """Every raster implementation with the camera outside the class map: raster_ground_rows (plain and the UNI_CHECK / HILLS form), raster_dyn_batch
    and raster_lens_frame clamp each in their own code; the spec's ix = clamp((int)floor(gx), 0, GW-1) onto the GRASS border decides."""
    from triton_racer_sim_amd.env import lighting_params
    v = dict(OFFMAP_VARIANTS[variant])
    track, filt, light, lens = v.pop("track", "generated"), v.pop("filt", None), v.pop("light", False), v.pop("lens", None)
    depth = v.get("depth", False)
    pts = track_points(track)
    n = 32
    g = make_env("hip", n_envs=n, track=pts, auto_reset=False, **v)
    o = make_env("oracle", n_envs=n, track=pts, auto_reset=False, **v)
    p = lighting_params(n, seed=11) if light else None
    chk = request.getfixturevalue("checker") if lens else None
    if filt:
        g.set_frame_filter(filt); o.set_frame_filter(filt)
    if light:
        g.set_lighting(p)
    if lens:
        g.set_camera(*lens)
    for env in (g, o):
        place_rings(env, pts)
    if resident:
        g.set_step_mode(True)
    path = f"off-map/{variant}/{'resident' if resident else 'launches'}"
    for t in range(OFFMAP_STEPS):
        st, th = offmap_controls(t, n)
        for env in (g, o):
            env.step(st, th)
        where = f"{path} step {t}"
        compare(g, o, where, path)
        if lens:
            want, want_depth = expected_frames(chk, g, lens)            # rendered from the env's own poses (equal to the oracle's: compare above)
        else:
            want, want_depth = (light_frames(o.fetch("img"), p) if light else o.fetch("img")), (o.fetch("depth") if depth else None)
        got = g.fetch("img")
        bad = np.argwhere((got != want).any(-1))
        assert bad.size == 0, f"{where}: {len(bad)} pixels differ, first (env, v, u) {bad[:4].tolist()}"
        if depth:
            assert np.array_equal(g.fetch("depth").view(np.uint32), want_depth.view(np.uint32)), where
    if resident:
        assert int(g.fetch("stats")[2]) == 0
    print(f"[step branches] {path}: largest float difference {_MAXDIFF[path]:.3g}")


@gpu
@pytest.mark.parametrize("resident", [False, True], ids=["launches", "resident"])
@pytest.mark.parametrize("track", ["generated", "mountain"])
def test_offmap_physics_only(make_env, track, resident):
    """render=False on the rings: wave_nearest<true> at fx = -1 and fx = nx, the full-scan fall back with a real result, and lost."""
    pts = track_points(track)
    n = 32
    g, o = make_env("hip", n_envs=n, track=pts, render=False), make_env("oracle", n_envs=n, track=pts, render=False)
    for env in (g, o):
        place_rings(env, pts)
    if resident:
        g.set_step_mode(True)
    path = f"off-map/physics/{track}/{'resident' if resident else 'launches'}"
    for t in range(OFFMAP_STEPS):
        st, th = offmap_controls(t, n)
        for env in (g, o):
            env.step(st, th)
        compare(g, o, f"{path} step {t}", path)
    seg = o.fetch("seg_idx")
    assert [int((seg[8 * r:8 * r + 8] == 0).sum()) for r in range(4)] == [0, 0, 4, 8]
    print(f"[step branches] {path}: largest float difference {_MAXDIFF[path]:.3g}")
