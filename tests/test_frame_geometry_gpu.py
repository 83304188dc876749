"""Every raster variant at frame sizes and env counts where its indexing is hard.

The rasteriser is built as DEPTH x {plain, DYN, HILLS, LENS, LIGHT, LIGHT + HILLS, LIGHT + DYN}, in trs_step_kernel and trs_worker_kernel.  Its indexing
follows the frame (rows_per_pass = 512 / (W / 4) and the threads that division leaves idle, hill_batch(H) row tables per batch, light_copies(W / 4) lit
palettes, the lens cache rows and the rows behind them, the worker's store counts per step) and the envs a workgroup owns (envs_per_wg = ceil(n_envs / CUs):
batches of kDynBatch = 4 and of hill_batch(H), the LIGHT parameter ring of kCamDepth x envs_per_wg slots).  The other files pin every variant bit for bit
at 60x80, 64x64, 120x160 and 240x320 with mostly one env per workgroup; this one runs them all at the seven sizes of GEOMETRY, each the smallest frame that
reaches the property its row names, with env counts taken from the device's CU count, through three step paths each (PATHS).

References are the project's own: the oracle for plain, DYN, static-filter and HILLS frames; light_frames(oracle raw) and preprocess_host for LIGHT
(tests/test_lighting_gpu.py::assert_lit); the lens checker on the handle's own poses (tests/test_lens_gpu.py).  Frames, depth words and integer fields
bit for bit, float state at 1e-5 (tests/test_gpu_parity.py::assert_state_equal).  The tests without a gpu mark pin, on the CPU, that the sizes are what
the table claims (through the plan header), that the substituted heights are the nearest that fit, and that the oracle's frames at these sizes
really differ from env to env."""
import numpy as np
import pytest

from conftest import track_points
from test_host_tables import LDS_BYTES, driver, plan_driver, run_layout, run_plan  # noqa: F401  (driver and plan_driver are fixtures)
from test_image_path import DYNAMIC, FUSED
from test_lens_gpu import checker, expected_frames  # noqa: F401  (checker is a fixture)
from test_lens_tables_cpu import LENSES
from test_lighting_gpu import assert_lit, params_for
from test_step_branches_gpu import _MAXDIFF, compare

gpu = pytest.mark.gpu
F = np.float32
MI355X_CUS = 256                                # the CPU tests size their workgroups like the device the kernels are built for

# id: (H, W, n_envs(CUs), and what plan_driver must say: rows per pass, idle raster threads, passes, rows of the last pass, hill_batch, light_copies,
#      the dynamic filter's brightness window is empty)
#   A  odd H; one partial pass, so threads with vstart >= H idle; three row tables per batch; lens: one cached row per thread
#   B  the narrowest frame; two row tables per batch; one lit palette; W % 8 != 0
#   C  a row's groups straddle wave boundaries; the second pass is ragged (87 rows); one row table per batch
#   D  odd H and an odd group count; 6 idle threads; passes of 46 + 15 rows; four row tables per batch; W % 8 != 0
#   E  H > 512: the palette build and DYN's row loop take several rounds; passes of 256 + 256 + 3 rows
#   F  a row spans three waves; 122 idle threads; 11 passes; four lit palettes; DYN's window rows [40, 119) are empty; lens rows beyond the register cache
#   G  the widest frame; one row per pass; nine lit palettes (and, three rows high, an empty window as F)
# A, B and D run 4 CUs + 70 envs: five envs per workgroup (a full batch of four plus one, or 3 + 2, or 2 + 2 + 1) and a ragged last workgroup.
GEOMETRY = {
    "A": (131, 8, lambda cus: 4 * cus + 70, dict(rows_per_pass=256, idle=0, passes=1, last=131, hill_batch=3, light_copies=2, empty_window=False)),
    "B": (171, 4, lambda cus: 4 * cus + 70, dict(rows_per_pass=512, idle=0, passes=1, last=171, hill_batch=2, light_copies=1, empty_window=False)),
    "C": (257, 12, lambda cus: 300, dict(rows_per_pass=170, idle=2, passes=2, last=87, hill_batch=1, light_copies=2, empty_window=False)),
    "D": (61, 44, lambda cus: 4 * cus + 70, dict(rows_per_pass=46, idle=6, passes=2, last=15, hill_batch=4, light_copies=2, empty_window=False)),
    "E": (515, 8, lambda cus: 2 * cus + 3, dict(rows_per_pass=256, idle=0, passes=3, last=3, hill_batch=1, light_copies=2, empty_window=False)),
    "F": (33, 520, lambda cus: 9, dict(rows_per_pass=3, idle=122, passes=11, last=3, hill_batch=4, light_copies=4, empty_window=True)),
    "G": (3, 2048, lambda cus: 5, dict(rows_per_pass=1, idle=0, passes=3, last=1, hill_batch=4, light_copies=9, empty_window=True)),
}
LENS_SIZES = {"A": (131, 8), "C'": (257, 16), "E": (515, 8), "F": (33, 520), "G": (3, 2048)}   # (C': C with a width the lens takes)
LENS_ENVS = {"C'": "C"}

# Heights replaced because the variant does not fit a CU's 160 KiB beside the track's tables at the table's H (test_substituted_heights_are_the_nearest_that_fit
# proves each on the CPU: the table's H does not fit, this one does, H + 2 does not).  No hilly or DYN variant fits at any H > 512, so E's "several rounds" is
# reached by the plain, static-filter, LIGHT and LENS cases only; what the substitutes keep:
#   E dyn 391: passes of 256 + 135 rows, so DYN's row loop still takes two rounds and its palette build (4 x 391 items over 512 threads) four
#   E hills 401 / light+hills 395: passes of 256 + 145 / 139 rows, one row table per batch, three envs per workgroup
#   E light+dyn 243: a single partial pass (as A) with three envs per workgroup: a ragged batch of three lit palettes by channel
#   C light+dyn 247: C's properties unchanged (passes of 170 + 77 rows)
SUBSTITUTED_H = {("E", "dyn"): 391, ("E", "hills+depth"): 401, ("E", "hills+static"): 401, ("E", "light+hills"): 395, ("E", "light+dyn"): 243, ("C", "light+dyn"): 247}
# Widths replaced because of a refusal by policy that exists: trs_set_frame_filter takes dynamic brightness only where a thread walks at most 16 rows of the
# window img[40:119] (their class bits live in four registers), which is rows_per_pass >= 5, W <= 408.  F and G are wider
# (test_dynamic_brightness_is_refused_where_a_thread_walks_too_many_rows pins the refusal there); their DYN cases run at the widest frame that is taken:
# 102 groups per row, 5 rows per pass, 2 idle threads, a row spans two waves, and at both heights the window is empty.
DYN_MAX_W = 408
SUBSTITUTED_W = {(size, case): DYN_MAX_W for size in "FG" for case in ("dyn", "light+dyn")}

V_DEPTH, V_DYN, V_HILLS, V_LENS, V_LIGHT = 1, 2, 4, 8, 16
# case: the handle's settings, and the kernel variant they select (trsim_plan.hpp, variant_bits)
CASES = {
    "rgb": (dict(), 0),
    "depth": (dict(depth=True), V_DEPTH),
    "static": (dict(filt=FUSED[2]), 0),
    "dyn": (dict(filt=DYNAMIC[1]), V_DYN),
    "hills+depth": (dict(track="mountain", depth=True), V_HILLS | V_DEPTH),
    "hills+static": (dict(track="mountain", filt=FUSED[2]), V_HILLS),
    "light": (dict(light=True), V_LIGHT),
    "light+static": (dict(light=True, filt=FUSED[1]), V_LIGHT),
    "light+dyn": (dict(light=True, filt=DYNAMIC[1]), V_LIGHT | V_DYN),
    "light+hills": (dict(track="mountain", light=True), V_LIGHT | V_HILLS),
}
PATHS = ("launches", "sequence", "resident")
LENS = next(l for l in LENSES if l[2] != 0.0)


def height_of(size, case):
    return SUBSTITUTED_H.get((size, case), GEOMETRY[size][0])


def width_of(size, case):
    return SUBSTITUTED_W.get((size, case), GEOMETRY[size][1])


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def controls(n, steps, seed):
    """Per-env host controls [steps, n] and a reset mask over a tenth of the envs."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (steps, n)).astype(F), rng.uniform(0.2, 1, (steps, n)).astype(F), (rng.uniform(0, 1, n) < 0.1).astype(np.uint8)


def drive(envs, g, path, n, check):
    """The three step paths: `envs` all take the same steps (g, the HIP handle, by `path`); check(where) compares after each."""
    st, th, rs = controls(n, 5, 17)
    if path == "launches":                      # single trs_step launches with per-env host controls, a reset mask on the second
        for t in range(3):
            for env in envs:
                env.step(st[t], th[t], 0.0, reset=rs if t == 1 else None)
            check(f"{path} step {t}")
    elif path == "sequence":                    # 5 steps, 3 per launch: the last launch is ragged
        for env in envs:
            env.step_sequence(st, th, reset=rs, steps_per_launch=3)
        check(f"{path} 5 steps, 3 per launch")
    else:                                       # posted to the resident worker, then a lock-step tick
        g.set_step_mode(True)
        for env in envs:
            env.step_synthetic(4, 1)
        check(f"{path} 4 posts")
        for env in envs:
            env.step(st[0], th[0], 0.0)
        g.sync()
        check(f"{path} lock-step tick")
        assert g.step_mode()[0] == "resident"
        assert int(g.fetch("stats")[2]) == 0    # no layout fault: the worker really ran


# ---------------------------------------------------------------------------------------------------------------- the GPU table

@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("size", list(GEOMETRY))
def test_variant_at_geometry(make_env, size, case, path):
    n_of = GEOMETRY[size][2]
    H, W, n = height_of(size, case), width_of(size, case), n_of(device_cus())
    settings, _ = CASES[case]
    pts = track_points(settings.get("track", "generated"))
    depth, filt, light = settings.get("depth", False), settings.get("filt"), settings.get("light", False)
    kw = dict(n_envs=n, track=pts, img_h=H, img_w=W, depth=depth, auto_reset=True)
    g, o = make_env("hip", **kw), make_env("oracle", **kw)
    p = params_for(n, 21) if light else None
    if filt:
        g.set_frame_filter(filt)
        if not light:
            o.set_frame_filter(filt)            # (a lit handle's reference filters the LIT oracle frames: assert_lit)
    if light:
        g.set_lighting(p)
    tag = f"geometry/{size} {H}x{W} n={n}/{case}/{path}"

    def check(where):
        if light:
            compare(g, o, f"{tag}: {where}", tag)
            assert_lit(g, o, p, f"{tag}: {where}", depth, cfg=filt)
        else:
            compare(g, o, f"{tag}: {where}", tag, frames=True, depth=depth)

    drive((g, o), g, path, n, check)
    print(f"[frame geometry] {tag}: largest float difference {_MAXDIFF[tag]:.3g}")


@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("size", list(LENS_SIZES))
def test_lens_at_geometry(make_env, checker, size, path):
    H, W = LENS_SIZES[size]
    n = GEOMETRY[LENS_ENVS.get(size, size)][2](device_cus())
    kw = dict(n_envs=n, img_h=H, img_w=W, depth=True, auto_reset=True)
    g, o = make_env("hip", **kw), make_env("oracle", **kw)
    g.set_camera(*LENS)
    tag = f"geometry/{size} {H}x{W} n={n}/lens+depth/{path}"

    def check(where):
        compare(g, o, f"{tag}: {where}", tag)                              # the lens changes no physics
        want, want_depth = expected_frames(checker, g, LENS)                # rendered from the handle's own poses
        got = g.fetch("img")
        bad = np.argwhere((got != want).any(-1))
        assert bad.size == 0, f"{tag}: {where}: {len(bad)} pixels differ from the checker, first (env, v, u) {bad[:4].tolist()}"
        bad = np.argwhere(g.fetch("depth").view(np.uint32) != want_depth.view(np.uint32))
        assert bad.size == 0, f"{tag}: {where}: {len(bad)} depth words differ, first (env, v, u) {bad[:4].tolist()}"

    drive((g, o), g, path, n, check)
    print(f"[frame geometry] {tag}: largest float difference {_MAXDIFF[tag]:.3g}")


DEEP_POSTS = 19                                 # posts without a sync: more than 2 x kSlots (8 posts in flight) and more than 4 x kCamDepth (4 hand-off slots per env)
DEEP_LENS_W = 48                                # D's 44 is no multiple of 8 (the lens is refused there, below): the next width it takes, as C' is to C


@gpu
@pytest.mark.parametrize("case", list(CASES) + ["lens+depth"])
def test_variant_resident_deep_queue(make_env, checker, case):
    """The worker's hand-off where the other tests hardly reach it: size D (five envs per workgroup in batches of 4 + 1, a ragged last workgroup), 19 steps
    posted without a sync — the slot ring wraps (r >= kCamDepth), the physics team runs into the back-pressure of rread, the deferred rread bump of the
    LIGHT variants is what frees a slot, and arrivals lag a full `keep` — then three lock-step ticks with per-env host controls and a reset mask on the second.
    The references and tolerances are test_variant_at_geometry's (test_lens_at_geometry's for the lens), after the posts and after every tick."""
    lens = case == "lens+depth"
    H, W = (GEOMETRY["D"][0], DEEP_LENS_W) if lens else (height_of("D", case), width_of("D", case))
    n = GEOMETRY["D"][2](device_cus())
    settings, _ = (dict(depth=True), V_LENS | V_DEPTH) if lens else CASES[case]
    depth, filt, light = settings.get("depth", False), settings.get("filt"), settings.get("light", False)
    kw = dict(n_envs=n, track=track_points(settings.get("track", "generated")), img_h=H, img_w=W, depth=depth, auto_reset=True)
    g, o = make_env("hip", **kw), make_env("oracle", **kw)
    p = params_for(n, 21) if light else None
    if filt:
        g.set_frame_filter(filt)
        if not light:
            o.set_frame_filter(filt)
    if light:
        g.set_lighting(p)
    if lens:
        g.set_camera(*LENS)
    tag = f"geometry/D {H}x{W} n={n}/{case}/deep queue"

    def check(where):
        if lens:
            compare(g, o, f"{tag}: {where}", tag)
            want, want_depth = expected_frames(checker, g, LENS)
            bad = np.argwhere((g.fetch("img") != want).any(-1))
            assert bad.size == 0, f"{tag}: {where}: {len(bad)} pixels differ from the checker, first (env, v, u) {bad[:4].tolist()}"
            bad = np.argwhere(g.fetch("depth").view(np.uint32) != want_depth.view(np.uint32))
            assert bad.size == 0, f"{tag}: {where}: {len(bad)} depth words differ, first (env, v, u) {bad[:4].tolist()}"
        elif light:
            compare(g, o, f"{tag}: {where}", tag)
            assert_lit(g, o, p, f"{tag}: {where}", depth, cfg=filt)
        else:
            compare(g, o, f"{tag}: {where}", tag, frames=True, depth=depth)

    st, th, rs = controls(n, 3, 17)
    g.set_step_mode(True)
    for env in (g, o):
        env.step_synthetic(DEEP_POSTS, 1)
    check(f"{DEEP_POSTS} posts")
    for t in range(3):
        for env in (g, o):
            env.step(st[t], th[t], 0.0, reset=rs if t == 1 else None)
        g.sync()
        check(f"lock-step tick {t}")
    assert g.step_mode()[0] == "resident"
    assert int(g.fetch("stats")[2]) == 0        # no layout fault: the worker really ran
    print(f"[frame geometry] {tag}: largest float difference {_MAXDIFF[tag]:.3g}")


@gpu
@pytest.mark.parametrize("size", ["B", "D"])
def test_lens_is_refused_where_the_width_is_no_multiple_of_8(make_env, size):
    """trs_set_camera fails with its reason, and the handle steps exactly like a twin that never asked, in all three paths (the twin always by launches:
    two resident workers of one process would take turns on the GPU)."""
    H, W, n_of, _ = GEOMETRY[size]
    n = n_of(device_cus())
    for path in PATHS:
        kw = dict(n_envs=n, img_h=H, img_w=W, depth=True, auto_reset=True)
        g, twin = make_env("hip", **kw), make_env("hip", **kw)
        with pytest.raises(RuntimeError, match="multiple of 8"):
            g.set_camera(*LENS)
        assert g.camera() == (0.0, 0.0, 0.0)

        def check(where):
            for k in ("pos_x", "pos_y", "pos_z", "speed", "cte", "yaw", "vel", "ep_return", "last_return", "seg_idx", "done", "ep_len", "img"):
                assert np.array_equal(g.fetch(k), twin.fetch(k)), (size, path, where, k)
            assert np.array_equal(g.fetch("depth").view(np.uint32), twin.fetch("depth").view(np.uint32)), (size, path, where)

        drive((g, twin), g, path, n, check)
        g.close(); twin.close()


@gpu
@pytest.mark.parametrize("light", [False, True], ids=["dyn", "light+dyn"])
@pytest.mark.parametrize("size", ["F", "G"])
def test_dynamic_brightness_is_refused_where_a_thread_walks_too_many_rows(make_env, size, light):
    """At F and G a thread would walk more than 16 window rows: trs_set_frame_filter says so, and the handle goes on rendering what it rendered before
    (raw frames, or lit ones) in all three paths."""
    H, W, n_of, _ = GEOMETRY[size]
    n = n_of(device_cus())
    p = params_for(n, 22)
    for path in PATHS:
        kw = dict(n_envs=n, img_h=H, img_w=W, auto_reset=True)
        g, o = make_env("hip", **kw), make_env("oracle", **kw)
        if light:
            g.set_lighting(p)
        with pytest.raises(RuntimeError, match="image too wide for the in-kernel dynamic-brightness filter"):
            g.set_frame_filter(DYNAMIC[1])
        tag = f"geometry/{size} {H}x{W} n={n}/{'light+' if light else ''}dyn refused/{path}"

        def check(where):
            if light:
                compare(g, o, f"{tag}: {where}", tag)
                assert_lit(g, o, p, f"{tag}: {where}")
            else:
                compare(g, o, f"{tag}: {where}", tag, frames=True)

        drive((g, o), g, path, n, check)
        g.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------- the inputs are what they claim (CPU)

def test_dyn_width_is_the_widest_the_filter_takes(plan_driver):
    """rows_per_pass >= 5 (16 window rows per thread at most: ceil(79 / 5)) holds at DYN_MAX_W and no further; F and G are beyond it."""
    def rpp(W):
        (row,) = run_plan(plan_driver, "geometry", 33, W)
        return int(row[4])
    assert rpp(DYN_MAX_W) == 5 and -(-79 // 5) == 16 and rpp(DYN_MAX_W + 4) == 4 and -(-79 // 4) > 16
    assert rpp(GEOMETRY["F"][1]) < 5 and rpp(GEOMETRY["G"][1]) < 5
    for H in (33, 3):
        (row,) = run_plan(plan_driver, "geometry", H, DYN_MAX_W)
        assert int(row[10]) >= int(row[11])                                  # the window is empty there as well

@pytest.mark.parametrize("size", list(GEOMETRY))
def test_sizes_reach_what_the_table_claims(plan_driver, size):
    H, W, _, claim = GEOMETRY[size]
    (row,) = run_plan(plan_driver, "geometry", H, W)
    tag, h, w, gpr, rpp, idle, passes, last, hb, lc, w0, w1 = [row[0]] + [int(x) for x in row[1:]]
    assert (tag, h, w, gpr) == ("geometry", H, W, W // 4)
    got = dict(rows_per_pass=rpp, idle=idle, passes=passes, last=last, hill_batch=hb, light_copies=lc, empty_window=w0 >= w1)
    assert got == claim
    assert rpp * (passes - 1) + last == H and 0 < last <= rpp                # the passes cover the frame; the last one is the ragged one


def test_env_counts_fill_workgroups_as_claimed():
    """At the device the kernels are built for: five envs per workgroup at A, B and D with a ragged last workgroup, three at E, two at C, one at F and G."""
    epw = {s: -(-GEOMETRY[s][2](MI355X_CUS) // MI355X_CUS) for s in GEOMETRY}
    assert epw == {"A": 5, "B": 5, "C": 2, "D": 5, "E": 3, "F": 1, "G": 1}
    for s in "ABDE":
        assert GEOMETRY[s][2](MI355X_CUS) % epw[s] != 0                      # the last workgroup that has envs has fewer
    assert [(4, 1), (3, 2), (2, 2, 1)] == [tuple(min(b, 5 - k) for k in range(0, 5, b)) for b in (4, 3, 2)]   # batches of kDynBatch / hill_batch in five envs


def fits(plan_driver, lds_step, H, W, variant, epw):
    """(one step per launch and three fit, the resident worker fits) for `variant` beside lds_step bytes of tables."""
    for tag, ls, v, e, total1, fit_steps, worker_total, fit_launch, fit_resident in run_plan(plan_driver, "fit", H, W, lds_step):
        if int(v) == variant and int(e) == epw:
            return int(fit_steps) >= 3, int(fit_resident) == 0
    raise AssertionError((H, W, variant, epw))


def lds_step_of(driver, oracle_api, tmp_path, track, H, W, epw):
    lines = run_layout(driver, oracle_api, tmp_path, track_points(track), H, W, epw)
    assert lines[1].startswith("layout "), lines[1]
    return {k: int(v) for k, v in (kv.split("=") for kv in lines[1].split()[1:])}["lds_step"]


@pytest.mark.parametrize("size", list(GEOMETRY))
def test_every_case_fits_in_lds(driver, plan_driver, oracle_api, tmp_path, size):
    """Every case of the GPU table fits beside its track's tables at the height it runs at, by launches (three steps per launch) and resident."""
    _, W, n_of, _ = GEOMETRY[size]
    epw = -(-n_of(MI355X_CUS) // MI355X_CUS)
    for case, (settings, variant) in CASES.items():
        H, Wc = height_of(size, case), width_of(size, case)
        lds_step = lds_step_of(driver, oracle_api, tmp_path, settings.get("track", "generated"), H, Wc, epw)
        assert fits(plan_driver, lds_step, H, Wc, variant, epw) == (True, True), (size, case, H, Wc)
    if size in "ACEFG":
        H, W = LENS_SIZES["C'" if size == "C" else size]
        assert fits(plan_driver, lds_step_of(driver, oracle_api, tmp_path, "generated", H, W, epw), H, W, V_LENS | V_DEPTH, epw) == (True, True)


@pytest.mark.parametrize("key", list(SUBSTITUTED_H), ids=lambda k: f"{k[0]}-{k[1]}")
def test_substituted_heights_are_the_nearest_that_fit(driver, plan_driver, oracle_api, tmp_path, key):
    size, case = key
    H0, W, n_of, _ = GEOMETRY[size]
    epw = -(-n_of(MI355X_CUS) // MI355X_CUS)
    settings, variant = CASES[case]
    track = settings.get("track", "generated")

    def ok(H):
        return fits(plan_driver, lds_step_of(driver, oracle_api, tmp_path, track, H, W, epw), H, W, variant, epw) == (True, True)

    H = SUBSTITUTED_H[key]
    assert H % 2 == 1 and H < H0 and not ok(H0) and ok(H) and not ok(H + 2)
    if variant & (V_HILLS | V_DYN):                                          # no H > 512 fits these: E's property is out of their reach
        assert not ok(513)


def oracle_frames(make_env, track, H, W, filt=None, depth=False, n=40):
    env = make_env("oracle", n_envs=n, track=track_points(track), img_h=H, img_w=W, depth=depth, auto_reset=True)
    if filt:
        env.set_frame_filter(filt)
    env.step_synthetic(6, 1)
    return env.fetch("img"), (env.fetch("depth") if depth else None)


def distinct(img):
    return len({f.tobytes() for f in img})


@pytest.mark.parametrize("size", list(GEOMETRY))
def test_oracle_frames_differ_between_envs(make_env, size):
    """40 envs, six synthetic steps, on the oracle alone: a kernel that rendered every env of a workgroup, batch or ring slot from one env's pose,
    palette or row table could not pass the GPU table.  Every frame is distinct at A to F (G, three rows high: at least 36 of 40); the dynamic filter
    changes the frames at A to E and leaves F's (empty window) distinct per env; on the mountain track the first ground row differs between envs at A to E."""
    H, W, _, claim = GEOMETRY[size]
    raw, _ = oracle_frames(make_env, "generated", H, W)
    print(f"[frame geometry] {size} {H}x{W}: {distinct(raw)} distinct frames of 40")
    assert distinct(raw) >= (36 if size == "G" else 40)
    Hd, Wd = height_of(size, "dyn"), width_of(size, "dyn")
    raw_d = raw if (Hd, Wd) == (H, W) else oracle_frames(make_env, "generated", Hd, Wd)[0]
    dyn, _ = oracle_frames(make_env, "generated", Hd, Wd, filt=DYNAMIC[1])
    assert distinct(dyn) >= (36 if size == "G" else 40)
    if size in "ABCDE":
        assert not claim["empty_window"] and (dyn != raw_d).any(axis=(1, 2, 3)).all()
        for case in ("hills+depth", "light+hills"):
            Hh = height_of(size, case)
            _, dep = oracle_frames(make_env, "mountain", Hh, W, depth=True)
            ground = dep[:, :, 0] < F(40.0)
            assert ground.any(axis=1).all()
            first_ground = ground.argmax(axis=1)
            print(f"[frame geometry] {size} {Hh}x{W} mountain: first ground rows {first_ground.min()}-{first_ground.max()}")
            assert first_ground.max() > first_ground.min()
