"""The product's host-side table builder (csrc/trsim_tables.cpp: class map, row table, palette, tangents) on the CPU, built
with AddressSanitizer + UBSan, against the oracle's tables bit for bit; the layout and packing of a track's two LDS images, the refusals by policy and the LDS fit arithmetic
(csrc/trsim_plan.hpp) against fixtures computed with the arithmetic `trs_load_track` and the setters had — their host logic without a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_golden, track_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("host_tables") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "host_tables_driver.cpp"),
                           os.path.join(ROOT, "triton-racer-sim_amd", "csrc", "trsim_tables.cpp")])
    return str(exe)


@pytest.mark.parametrize("track,shape", [("generated", (120, 160)), ("mountain", (120, 160)), ("generated", (240, 320)), ("generated", (64, 64))])
def test_host_tables_equal_the_oracle(driver, make_env, oracle_api, tmp_path, track, shape):
    from triton_racer_sim_amd import _ffi
    h, w = shape
    pts = track_points(track)
    env = make_env("oracle", n_envs=2, img_h=h, img_w=w, track=pts)
    cfg = _ffi.TrsConfig()
    oracle_api.default_config(C.byref(cfg))
    cfg.n_envs, cfg.img_h, cfg.img_w = 2, h, w
    (tmp_path / "cfg.bin").write_bytes(bytes(cfg))
    (tmp_path / "pts.bin").write_bytes(np.ascontiguousarray(pts, dtype=np.float64).tobytes())
    out = subprocess.run([driver, str(tmp_path / "cfg.bin"), str(tmp_path / "pts.bin"), str(tmp_path / "t")], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    for name, dtype in (("map", np.uint32), ("rowtab", np.float32), ("palette", np.uint32), ("tangent", np.float32), ("rowdepth", np.float32)):
        got = np.fromfile(tmp_path / f"t.{name}", dtype=dtype)
        want = env.fetch(name).reshape(-1)
        assert got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


# ---- the layout of a track's two LDS images and the refusals (csrc/trsim_plan.hpp), on the CPU ---------------------------------------------

LDS_BYTES = 160 * 1024
V_DEPTH, V_DYN, V_HILLS, V_LENS, V_LIGHT = 1, 2, 4, 8, 16
FEATURE_BITS = {"DYN": V_DYN, "HILLS": V_HILLS, "LENS": V_LENS, "LIGHT": V_LIGHT}


def built(v):
    """variant_built as DESIGN.md states it: no DYN with HILLS, no LENS with DYN, HILLS or LIGHT."""
    return not (v & V_DYN and v & V_HILLS) and not (v & V_LENS and v & (V_DYN | V_HILLS | V_LIGHT))


def layout_track(name, resampled_to=None, scaled_by=None):
    """The fixture's tracks: the two golden tracks, the mountain track without its heights (`long_flat_track` of tests/test_lens_gpu.py), a
    track resampled to n points (point i at arc index i * len / n of the closed lap, linear between its two neighbours) or scaled about the origin."""
    pts = track_points("mountain" if name == "long_flat" else name).copy()
    if name == "long_flat":
        pts[:, 1] = 0.0
    if resampled_to:
        t = np.arange(resampled_to) * (len(pts) / resampled_to)
        i0 = np.floor(t).astype(int)
        f = (t - i0)[:, None]
        pts = pts[i0] * (1.0 - f) + pts[(i0 + 1) % len(pts)] * f
    return pts if scaled_by is None else pts * scaled_by


def run_layout(driver, oracle_api, tmp_path, pts, h, w, envs_per_wg):
    from triton_racer_sim_amd import _ffi
    cfg = _ffi.TrsConfig()
    oracle_api.default_config(C.byref(cfg))
    cfg.n_envs, cfg.img_h, cfg.img_w = 2, h, w
    (tmp_path / "cfg.bin").write_bytes(bytes(cfg))
    (tmp_path / "pts.bin").write_bytes(np.ascontiguousarray(pts, dtype=np.float64).tobytes())
    out = subprocess.run([driver, str(tmp_path / "cfg.bin"), str(tmp_path / "pts.bin"), str(tmp_path / "t"), str(envs_per_wg)], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


LAYOUT_CASES = load_golden("track_layouts.json")


@pytest.mark.parametrize("case", LAYOUT_CASES["cases"], ids=lambda c: f"{c['track']}-{c['img_h']}x{c['img_w']}-{c['envs_per_wg']}")
def test_track_layout_and_packed_images(driver, oracle_api, tmp_path, case):
    h, w = case["img_h"], case["img_w"]
    lines = run_layout(driver, oracle_api, tmp_path, layout_track(case["track"]), h, w, case["envs_per_wg"])
    n_points, map_w, map_h, map_words = (int(x) for x in lines[0].split())
    assert lines[1].startswith("layout "), lines[1]
    L = {k: int(v) for k, v in (kv.split("=") for kv in lines[1].split()[1:])}
    hills = lines[2] == "hills 1"
    # (a) every field is what the arithmetic of trs_load_track gave before it moved (the fixture was computed with those lines)
    assert L == case["layout"]
    # (b) regions: 16-byte aligned, in order, disjoint, inside the image; the map pitch is an odd number of words
    pts_b, grid_start_b, grid_pts_b = n_points * 8, os.path.getsize(tmp_path / "t.grid_start"), os.path.getsize(tmp_path / "t.grid_pts")
    phys = [("px", 0, pts_b), ("py", L["p.off_py"], pts_b), ("pz", L["p.off_pz"], pts_b)]
    if L["p.tan_in_lds"]:
        phys.append(("tangent", L["p.off_tan"], n_points * 8))
    phys += [("grid_start", L["p.off_gstart"], grid_start_b), ("grid_pts", L["p.off_gpts"], grid_pts_b)]
    raster = [("map", 0, L["r.map_pitch_b"] * map_h), ("rowtab", L["r.off_rowtab"], h * 8), ("palette", L["r.off_pal"], h * 16), ("rowdepth", L["r.off_depth"], h * 4)]
    if hills:
        raster.append(("sky", L["r.off_sky"], h * 4))
    for regions, blob_bytes in ((phys, L["p.blob_bytes"]), (raster, L["r.blob_bytes"])):
        end = 0
        for name, off, size in regions:
            assert off % 16 == 0 and off >= end, (name, off, end)
            end = off + size
        assert end <= blob_bytes, (regions[-1][0], end, blob_bytes)
    assert L["r.map_pitch_b"] % 4 == 0 and (L["r.map_pitch_b"] // 4) % 2 == 1 and L["r.map_pitch_b"] // 4 >= map_words
    assert L["p.pts_bytes"] == L["p.off_tan"] and L["p.off_scratch"] == L["p.blob_bytes"] and L["p.lds_p"] >= L["p.blob_bytes"] and L["p.lds_p"] % 16 == 0
    assert L["lds_off_phys"] == L["r.lds_r"] >= L["r.blob_bytes"] and L["lds_off_phys"] % 16 == 0
    assert L["lds_step"] == L["lds_off_phys"] + L["p.blob_bytes"] <= LDS_BYTES and L["p.lds_p"] <= LDS_BYTES
    # (c) every region of a packed image is, byte for byte, the table it holds; the map rows are the unpitched map's
    img_p, img_r = (tmp_path / "t.phys").read_bytes(), (tmp_path / "t.raster").read_bytes()
    assert len(img_p) == L["p.blob_bytes"] and len(img_r) == L["r.blob_bytes"]
    for name, off, size in phys:
        assert img_p[off:off + size] == (tmp_path / f"t.{name}").read_bytes(), name
    for name, off, size in raster[1:]:
        assert img_r[off:off + size] == (tmp_path / f"t.{name}").read_bytes(), name
    unpitched = (tmp_path / "t.map").read_bytes()
    assert len(unpitched) == map_words * 4 * map_h
    for row in range(map_h):
        assert img_r[row * L["r.map_pitch_b"]:row * L["r.map_pitch_b"] + map_words * 4] == unpitched[row * map_words * 4:(row + 1) * map_words * 4], row


@pytest.mark.parametrize("case", LAYOUT_CASES["refusals"], ids=lambda c: f"{c['track']}-{c['resampled_to'] or c['scaled_by']}-{c['img_h']}x{c['img_w']}")
def test_track_layout_refusals(driver, oracle_api, tmp_path, case):
    lines = run_layout(driver, oracle_api, tmp_path, layout_track(case["track"], case["resampled_to"], case["scaled_by"]), case["img_h"], case["img_w"], case["envs_per_wg"])
    assert lines[1] == f"refused {case['code']} {case['text']}"


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("plan") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "plan_driver.cpp")])
    return str(exe)


def run_plan(plan_driver, *args):
    out = subprocess.run([plan_driver, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return [line.split(" ") for line in out.stdout.splitlines()]


def test_refusal_policy_is_variant_built(plan_driver):
    """For each of the 14 built variants as the handle's state and each feature bit a caller can add: refused exactly when the result is not built,
    naming a set bit that is not built together with the added one, with a message; the eight messages are the ones the setters had."""
    rows = run_plan(plan_driver, "policy")
    states = [v for v in range(32) if built(v)]
    assert len(states) == 14 and len(rows) == 14 * 4
    seen = {}
    for (tag, state, add, result_built, set_bit, pair_built, *text), (want_state, want_add) in zip(rows, [(s, a) for s in states for a in FEATURE_BITS.values()]):
        state, add, set_bit, text = int(state), int(add), int(set_bit), " ".join(text)
        assert tag == "clash" and (state, add) == (want_state, want_add)
        assert int(result_built) == built(state | add)
        if built(state | add):
            assert set_bit == 0 and text == ""
        else:
            assert set_bit in FEATURE_BITS.values() and state & set_bit and not built(add | set_bit) and int(pair_built) == 0 and text != ""
            assert seen.setdefault((add, set_bit), text) == text
    want = {(FEATURE_BITS[r["added"]], FEATURE_BITS[r["set"]]): r["text"] for r in load_golden("variant_refusals.json")}
    assert len(want) == 8 and seen == want
    # a lens camera asked for while two set features clash with it: the order of the setter's checks (HILLS, DYN, LIGHT) picks the message
    by_case = {(int(r[1]), int(r[2])): int(r[4]) for r in rows}
    assert by_case[(V_DYN | V_LIGHT, V_LENS)] == V_DYN and by_case[(V_HILLS | V_LIGHT, V_LENS)] == V_HILLS


def test_lds_fit_is_the_two_layouts(plan_driver):
    """lds_fit over the fixture's lds_step values, every built variant and 1 to 64 envs per workgroup: 'one step per launch fits' and 'the worker fits'
    as the two layout functions give them; each feature must be seen fitting and not fitting."""
    by_size = {}
    for c in LAYOUT_CASES["cases"]:
        by_size.setdefault((c["img_h"], c["img_w"]), set()).add(c["layout"]["lds_step"])
    answers = {(name, mode): set() for name in FEATURE_BITS for mode in ("launch", "resident")}
    n = 0
    for (h, w), steps in sorted(by_size.items()):
        for tag, lds_step, v, epw, total1, fit_steps, worker_total, fit_launch, fit_resident in run_plan(plan_driver, "fit", h, w, *sorted(steps)):
            v, launch_ok, worker_ok = int(v), int(total1) <= LDS_BYTES, int(worker_total) <= LDS_BYTES
            assert tag == "fit" and built(v) and (int(fit_steps) >= 1) == launch_ok
            assert int(fit_launch) == (0 if launch_ok else 1)                                # LdsFit: ok, no_launch, no_worker
            assert int(fit_resident) == (1 if not launch_ok else (0 if worker_ok else 2))
            for name, bit in FEATURE_BITS.items():
                if v & bit:
                    answers[(name, "launch")].add(int(fit_launch) == 0)
                    answers[(name, "resident")].add(int(fit_resident) == 0)
            n += 1
    assert n == sum(len(s) for s in by_size.values()) * 14 * 64
    assert all(a == {True, False} for a in answers.values()), answers


def test_control_slices_of_a_step_call(plan_driver):
    """Controls::after, the one owner of 'which controls does step k of a call read' (launch loops, the worker's post loop, the remainder after a
    fall-back): strides 0 and n_envs, brk / reset given or not, the synthetic call, k = 0..16, against a three-line model; and after(a).after(b) is
    after(a + b), which a fall-back followed by launch slices relies on."""
    n = 70

    def model(present, stride, k):                             # offsets in floats of steer, thr, brk (-1: null) and whether the reset mask survives
        return [k * stride if p else -1 for p in present], k == 0

    rows = [[r[0]] + [int(x) for x in r[1:]] for r in run_plan(plan_driver, "slices", n)]
    calls = set()
    for tag, stride, has_brk, has_reset, synth, a, b, o_st, o_th, o_br, reset_kept, synth_out, stride_out in rows:
        assert tag in ("slice", "compose") and stride in (0, n) and (b == 0 or tag == "compose")
        calls.add((stride, has_brk, has_reset, synth))
        offs, keeps = model([not synth, not synth, bool(has_brk)], stride, a + b)
        where = (tag, stride, has_brk, has_reset, synth, a, b)
        assert [o_st, o_th, o_br] == offs, where
        assert reset_kept == (1 if has_reset and keeps else 0), where          # (-1: a reset pointer that is not the call's)
        assert (synth_out, stride_out) == (synth, stride), where
    assert calls == {(s, br, rs, 0) for s in (0, n) for br in (0, 1) for rs in (0, 1)} | {(0, 0, 0, 1), (n, 0, 0, 1)}
    assert len(rows) == len(calls) * (17 + 81)


def test_fetch_layout_every_subset(plan_driver):
    """fetch_layout / fetch_reserve (the pinned staging of trs_fetch_outputs and trs_fetch_observation): for every subset of the eight items, n_envs in
    {1, 5, 70}, with and without a 64 x 64 frame: the items asked for start 16-byte aligned, in table order, without overlap, inside the reserve;
    and the reserve is the formula the staging has always been sized by."""
    rows = run_plan(plan_driver, "fetch")
    assert len(rows) == 3 * 2 * 256
    seen = set()
    for tag, n, img, mask, reserve, end, *items in rows:
        n, img, mask, reserve, end = int(n), int(img), int(mask), int(reserve), int(end)
        assert tag == "fetch" and n in (1, 5, 70) and img in (0, 64 * 64 * 3 * n) and len(items) == 8
        seen.add((n, img, mask))
        items = [tuple(int(x) for x in it.split(":")) for it in items]
        want = [(img if i == 0 else (n if i == 7 else 4 * n)) if mask >> i & 1 else 0 for i in range(8)]
        assert [b for _, b in items] == want
        assert reserve == ((want[0] + 15) & ~15) + 7 * ((4 * n + 15) & ~15) + 16
        at = 0
        for off, size in items:
            if not size:
                continue
            assert off % 16 == 0 and off >= at, (n, img, mask, items)        # aligned, ascending, behind the end of the item before
            at = off + size
        assert at <= end <= reserve, (n, img, mask, at, end, reserve)
    assert len(seen) == len(rows)


# ---- every LDS region and row-table plane over H = 2..600 (csrc/trsim_plan.hpp), on the CPU ------------------------------------------------

K_CAM_DEPTH, K_DYN_BATCH, K_SLOT_WORDS, K_LENS_PAL_BYTES, K_DYN_TAB_WORDS, K_RASTER_THREADS = 4, 4, 20, 513 * 16, 512 + 768 + 4 + 256, 512


def a16(x):
    return (x + 15) & ~15


def old_layouts(H, W, lds_step, epw, n_phys, v):
    """step_lds_layout, worker_lds_layout and the row tables' planes as the header computed them while a row table was 8 H | 16 H | 4 H without padding."""
    hilly, dyn, lens, light = bool(v & V_HILLS), bool(v & V_DYN), bool(v & V_LENS), bool(v & V_LIGHT)
    hb = max(1, min(4, K_RASTER_THREADS // H))
    tab = a16(28 * H)
    tabs = hb * tab + 48 if hilly else (K_LENS_PAL_BYTES if lens else 0)
    dyn_b = K_DYN_BATCH * H * 16 + 128 + a16(K_DYN_TAB_WORDS * 4) + H * 16

    def light_extra(slots):
        return slots * 32 + (0 if hilly else (K_DYN_BATCH * H * 16 if dyn else ((W // 4 + 126) // 64) * H * 16))

    rows = max(n_phys, 1) + 1
    cam = lds_step
    prog = cam + rows * epw * 16
    pitch = prog + epw * 4 + 16
    hill = a16(pitch + rows * epw * 4)
    lightoff = a16(hill + tabs)
    end = pitch
    if hilly or lens or light:
        end = hill + tabs
    if light:
        end = lightoff + light_extra(epw)
    dynoff = a16(end)
    step = dict(cam=cam, prog=prog, pitch=pitch, hill=hill, light=lightoff, lit=lightoff + epw * 32, dyn=dynoff, total=dynoff + dyn_b if dyn else end)
    ctl = a16(lds_step)
    slot = a16(64 + epw * 8)
    end = ctl + slot + K_CAM_DEPTH * epw * K_SLOT_WORDS * 4 + epw * 64 + 16
    wdyn = a16(end)
    if dyn:
        end = wdyn + dyn_b
    whill = a16(end)
    if hilly or lens:
        end = whill + tabs
    wlight = a16(whill + tabs)
    worker = dict(ctl=ctl, slots=ctl + slot, dyn=wdyn, hill=whill, light=wlight, lit=wlight + K_CAM_DEPTH * epw * 32,
                  total=wlight + light_extra(K_CAM_DEPTH * epw) if light else end)
    tables = {(k, name): (base + k * tab, base + k * tab + 8 * H, base + k * tab + 24 * H, base + (k + 1) * tab)
              for k in range(hb) for name, base in (("step", hill), ("worker", whill))} if hilly else {}
    return step, worker, tables, hb


@pytest.mark.parametrize("W,lds_step,epw,n_phys", [(160, 142240, 1, 1), (8, 117616, 5, 3), (12, 146656, 2, 16), (520, 114880, 3, 1), (2048, 159824, 64, 2)])
def test_lds_regions_and_row_table_planes_are_aligned(plan_driver, W, lds_step, epw, n_phys):
    """For H = 2..600 and every built variant, both kernels' layouts and each of the hill_batch(H) row tables.  What the kernels access 16 bytes at a
    time starts on a multiple of 16: the camera rows (float4), the tables' region, each row table and its palette plane (hill_row_build stores uint4,
    the row loops load them), the lighting parameters and the lit palettes behind them, the dynamic filter's region, the worker's control block and its
    hand-off slots (float4 camera parameters, 80 bytes each).  The rowtab plane (float2) needs 8, the depth plane, prog and pitch 4.  Planes and tables
    lie in order without overlap inside their region.  For even H every value is what the unpadded layout gave."""
    rows = run_plan(plan_driver, "lds", W, lds_step, epw, n_phys)
    n_rows = {"step": 0, "worker": 0, "table": 0}
    seen_odd_hilly = False
    got = {}
    for r in rows:
        got.setdefault((int(r[1]), int(r[2])), []).append(r)
    assert sorted(got) == [(H, v) for H in range(2, 601) for v in range(32) if built(v)]
    for (H, v), group in got.items():
        step_old, worker_old, tables_old, hb = old_layouts(H, W, lds_step, epw, n_phys, v)
        tables = {}
        for r in group:
            tag, vals = r[0], r[3:]
            if tag == "step":
                step = dict(zip(("cam", "prog", "pitch", "hill", "light", "lit", "dyn", "total"), map(int, vals)))
            elif tag == "worker":
                worker = dict(zip(("ctl", "slots", "dyn", "hill", "light", "lit", "total"), map(int, vals)))
            elif tag == "sizes":
                tabs_b, light_b, light_ring_b, dyn_b = map(int, vals)
            elif tag == "table":
                tables[(int(vals[0]), vals[1])] = tuple(int(x) for x in vals[2:])
            else:
                assert tag == "hbar" and int(vals[0]) == hb
                hbar = (int(vals[1]), int(vals[2]))
        for name in ("cam", "hill", "light", "lit", "dyn"):
            assert step[name] % 16 == 0, (H, v, name, step)
        for name in ("ctl", "slots", "dyn", "hill", "light", "lit"):
            assert worker[name] % 16 == 0, (H, v, name, worker)
        assert step["prog"] % 4 == 0 and step["pitch"] % 4 == 0 and dyn_b % 16 == 0
        assert lds_step == step["cam"] < step["prog"] < step["pitch"] <= step["hill"] <= step["light"] <= step["lit"] and step["hill"] + tabs_b <= step["light"]
        assert worker["ctl"] < worker["slots"] < worker["dyn"] <= worker["hill"] <= worker["light"] <= worker["lit"] and worker["hill"] + tabs_b <= worker["light"]
        if v & V_LIGHT:
            assert step["light"] + light_b <= step["dyn"] and step["light"] + light_b <= step["total"] and worker["light"] + light_ring_b == worker["total"]
        if v & V_DYN:
            assert step["dyn"] + dyn_b == step["total"] and worker["dyn"] + dyn_b <= worker["hill"]
        assert set(tables) == ({(k, name) for k in range(hb) for name in ("step", "worker")} if v & V_HILLS else set())
        for name, base, bar in (("step", step["hill"], 0), ("worker", worker["hill"], 1)):
            at = base
            for k in range(hb if v & V_HILLS else 0):
                tab, pal, dep, end = tables[(k, name)]
                assert tab == at and tab % 16 == 0 and pal % 16 == 0 and dep % 4 == 0, (H, v, k, name, tables[(k, name)])
                assert tab + 8 * H <= pal and pal + 16 * H == dep and dep + 4 * H <= end and end % 16 == 0, (H, v, k, name, tables[(k, name)])
                at = end
                n_rows["table"] += 1
                seen_odd_hilly |= H % 2 == 1
            if v & V_HILLS:
                assert hbar[bar] == at and at + 48 == base + tabs_b               # the barrier counter and the first-ground rows behind the last table
        if H % 2 == 0:
            assert (step, worker, tables) == (step_old, worker_old, tables_old), (H, v)
        n_rows["step"] += 1; n_rows["worker"] += 1
    assert n_rows["step"] == n_rows["worker"] == 599 * 14 and n_rows["table"] > 0 and seen_odd_hilly
