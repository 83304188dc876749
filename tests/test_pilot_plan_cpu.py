"""The pilot's plan and weight packing (csrc/trsim_pilot_plan.hpp) on the CPU: tests/pilot_plan_driver.cpp built with AddressSanitizer + UBSan and run as
a subprocess.  (a) Which kernel serves which layer, and with what LDS, at the sizes the GPU tests and the benchmark use — the table of DESIGN.md, computed
with the arithmetic trs_pilot_load had before it moved here (256 CUs, default tuning).  (b) Properties of every plan over a sweep of frame sizes and batch
capacities.  (c) The packing of the Keras arrays into fp16 granules against a numpy restatement written here."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BYTES = 160 * 1024
REFUSALS = ("image too small for Keras_2D_CNN", "dense1's shape does not suit trs_pilot_dense_kernel", "a convolution's weight slice does not fit LDS")
SPEC = [(5, 2, 3, 24), (5, 2, 24, 32), (5, 2, 32, 64), (3, 1, 64, 64), (3, 1, 64, 64), (3, 1, 64, 128), (3, 1, 128, 128)]


def build_driver(directory, sanitize=True):
    """The driver's executable, or None where there is no host compiler.  tests/test_pilot.py asks the same program for the plan of its cases, without the sanitizers."""
    if not shutil.which("g++"):
        return None
    exe = os.path.join(str(directory), "pilot_plan_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else [])
                          + ["-o", exe, os.path.join(ROOT, "tests", "pilot_plan_driver.cpp")])
    return exe


def run_driver(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (args, out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


def parse(line):
    """'kind a=1 b=x text=the rest' -> (kind, {a: 1, b: 'x', text: 'the rest'})"""
    kind, _, rest = line.partition(" ")
    rest, _, text = rest.partition(" text=")
    rec = {k: (int(v) if re.fullmatch(r"-?\d+", v) else v) for k, v in (kv.split("=", 1) for kv in rest.split())}
    if text:
        rec["text"] = text
    return kind, rec


def plan_of(exe, h, w, n_cap, cus=256, arrays=22, **tuning):
    """{'layers': [...], 'head': {...}, 'chain': {...}} or {'refuse': {...}} for one frame size."""
    plan = {"layers": []}
    for kind, rec in map(parse, run_driver(exe, "plan", h, w, n_cap, cus, arrays, *[f"{k}={v}" for k, v in tuning.items()])):
        if kind == "layer":
            plan["layers"].append(rec)
        else:
            plan[kind] = rec
    return plan


def call_of(exe, h, w, n_cap, n, cus=256, arrays=22, **tuning):
    """The call line of one batch: dense1's slices, the head's roll and grid, every layer's own grid (the launches and blocks behind it: tests/test_pilot_pass_cpu.py)."""
    (line,) = run_driver(exe, "call", h, w, n_cap, cus, arrays, n, "show=brief", *[f"{k}={v}" for k, v in tuning.items()])
    return parse(line)[1]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = build_driver(tmp_path_factory.mktemp("pilot_plan"))
    if not exe:
        pytest.skip("g++ not available")
    return exe


# ---- (a) the table -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cap,f,lds", [(1, 2, 67072), (37, 2, 67072), (77, 2, 67072), (1024, 4, 132096), (1027, 4, 132096)])
def test_plan_at_120x160(driver, n_cap, f, lds):
    p = plan_of(driver, 120, 160, n_cap)
    head = p["head"]
    assert (head["on"], head["wsplit"], head["R2"], head["bands"], head["lds"]) == (1, 1, 6, 5, 135392)
    assert [l["served_by"] for l in p["layers"]] == ["band<whole>", "band<whole>", "frame5", "chain", "chain", "chain", "chain", "dense"]
    c3 = p["layers"][2]
    assert (c3["frame5"], c3["frame5_bands"], c3["frame5_lds"]) == (1, 1, 128128)
    assert [(l["frame"], l["frame_bands"]) for l in p["layers"][3:7]] == [(1, 1)] * 4
    chain = p["chain"]
    assert (chain["first"], chain["nl"], chain["F"], chain["lds"]) == (3, 4, f, lds)
    d = call_of(driver, 120, 160, n_cap, n_cap)
    assert (d["nf"], d["KS"]) == (1, 4 if n_cap == 1027 else 8)


def test_plan_at_240x320(driver):
    p = plan_of(driver, 240, 320, 512)
    head = p["head"]
    assert (head["on"], head["wsplit"], head["w2p"], head["cpr"], head["R2"], head["bands"], head["lds"]) == (1, 2, 39, 31, 6, 10, 139328)
    c3 = p["layers"][2]
    assert (c3["frame5"], c3["frame5_bands"], c3["frame5_ohb"], c3["frame5_lds"]) == (1, 5, 6, 148096)
    assert [(l["frame"], l["frame_bands"]) for l in p["layers"][3:7]] == [(1, 2), (1, 2), (1, 3), (1, 3)]
    assert p["chain"]["first"] == -1
    assert [l["served_by"] for l in p["layers"]] == ["band<split>", "band<split>", "frame5", "frame", "frame", "frame", "frame", "dense"]
    unsplit = plan_of(driver, 240, 320, 512, fuse_wsplit_max=1)
    assert unsplit["head"]["on"] == 0 and [l["served_by"] for l in unsplit["layers"][:2]] == ["u8", "span<1>"]
    for n, nf, ks in [(6, 1, None), (40, 1, None), (77, 1, None), (150, 2, 62), (512, 2, 31)]:
        d = call_of(driver, 240, 320, 512, n)
        assert d["nf"] == nf and (ks is None or d["KS"] == ks), (n, d)
        assert call_of(driver, 240, 320, 512, n, dense=2)["nf"] == 1


def test_plan_at_100x132_and_130x300(driver):
    p = plan_of(driver, 100, 132, 9)
    head = p["head"]
    assert (head["on"], head["wsplit"], head["w2p"], head["bands"], head["lds"]) == (1, 2, 15, 4, 85760)     # a frame row of 396 bytes is no multiple of 16
    assert (p["chain"]["first"], p["chain"]["F"]) == (3, 2)
    p = plan_of(driver, 130, 300, 131)
    head = p["head"]
    assert (head["on"], head["wsplit"], head["w2p"], head["lds"]) == (1, 2, 36, 132896)
    c3 = p["layers"][2]
    assert (c3["frame5"], c3["frame5_bands"], c3["frame5_lds"]) == (1, 2, 156928) and 158 * 1024 - c3["frame5_lds"] == 4864
    assert p["chain"]["first"] == -1


# every layer on its single-layer kernel, and of those the quad-load one wherever it applies: what tests/test_pilot_fallback.py loads its pilots with
FALLBACK = dict(no_fuse=1, span_layers_mask=0, frame5=0, frame_layers_mask=0, chain_layers=0)


def persistent_batch(plan, layer, cus):
    """The smallest odd batch at which conv(layer + 1)'s single-layer kernel gets more 32-pixel tiles than the waves that are resident: the grid is capped at
    cus x res_wg_per_cu workgroups (single_grid_x), below the cap it has a wave per tile, so the first such batch is the first past cap x waves x 32 pixels."""
    l = plan["layers"][layer]
    waves = cus * l["res_wg_per_cu"] * (l["res_block"] // 64)
    return (32 * waves // (l["OH"] * l["OW"]) + 1) | 1


def tiles_and_waves(plan, call, layer, n):
    """(32-pixel tiles, resident waves) of conv(layer + 1) launched by itself on n frames"""
    l = plan["layers"][layer]
    return (n * l["OH"] * l["OW"] + 31) // 32, call[f"grid{layer}"] * (l["res_block"] // 64)


@pytest.mark.parametrize("size,n_cap", [((120, 160), 1), ((120, 160), 5), ((100, 132), 9), ((96, 100), 37)])
def test_fallback_plan_is_the_quad_load_kernel_on_conv2_to_conv7(driver, size, n_cap):
    """trs_conv_lt_kernel under FALLBACK: <1> on conv2 (5 waves, 3 workgroups per CU), <2> on conv3..conv7, conv6 and conv7 in two slices of 64 channels,
    conv7 with 7 waves in 162,624 of the CU's 163,840 bytes.  The K lengths are 80, 100, 72, 72, 72 and 144 granules."""
    h, w = size
    p = plan_of(driver, h, w, n_cap, **FALLBACK)
    assert [l["served_by"] for l in p["layers"]] == ["u8", "lt<1>", "lt<2>", "lt<2>", "lt<2>", "lt<2>", "lt<2>", "dense"]
    assert p["head"]["runs"] == 0 and p["chain"]["first"] == -1
    res = lambda i: tuple(p["layers"][i][k] for k in ("res_nb", "res_ysplit", "res_block", "res_lds", "res_wg_per_cu"))
    assert res(1) == (1, 1, 320, 51648, 3)
    assert res(2) == (2, 1, 1024, 135824, 1)
    assert res(3) == res(4) == (2, 1, 1024, 107040, 1)
    assert res(5) == (2, 2, 1024, 107040, 1)
    assert res(6) == (2, 2, 448, 162624, 1) and LDS_BYTES - res(6)[3] == 1216
    assert [l["G_pad"] for l in p["layers"][1:7]] == [80, 100, 72, 72, 72, 144] and p["layers"][1]["run_pad"] == 16
    ohw = {(120, 160): [999, 204, 150, 104, 66, 36], (100, 132): [660, 117, 77, 45, 21, 5], (96, 100): [462, 81, 49, 25, 9, 1]}[size]
    assert [l["OH"] * l["OW"] for l in p["layers"][1:7]] == ohw
    # conv2's padding granule of the last output column is the spare last column of the same conv1 row: a frame is a multiple of 4 wide (trs_create), so conv1's
    # width W / 2 - 2 is even and conv2's windows end one column short of it
    l1 = p["layers"][1]
    assert l1["IW"] == w // 2 - 2 and 2 * (l1["OW"] - 1) + 5 == l1["IW"] - 1


def test_default_plans_of_large_frames_reach_the_quad_load_kernel(driver):
    """360x480 and 480x640 with the default tuning: the head cut in 3 and 4 parts, conv3 in 14 bands of 3 rows and 29 of 2, and trs_conv_lt_kernel<2>
    where a row band of a 3x3 layer's input does not fit LDS twice over: conv7, and conv4..conv7."""
    p = plan_of(driver, 360, 480, 3)
    head, c3 = p["head"], p["layers"][2]
    assert (head["on"], head["runs"], head["wsplit"], head["w2p"], head["cpr"], head["R2"], head["bands"], head["lds"]) == (1, 1, 3, 39, 31, 6, 15, 139328)
    assert (c3["frame5"], c3["frame5_bands"], c3["frame5_ohb"], c3["frame5_lds"]) == (1, 14, 3, 135040)
    assert [(l["frame"], l["frame_bands"], l["frame_ohb"]) for l in p["layers"][3:7]] == [(1, 5, 8), (1, 5, 8), (1, 8, 5), (0, 1, 34)]
    assert [l["served_by"] for l in p["layers"]] == ["band<split>", "band<split>", "frame5", "frame", "frame", "frame", "lt<2>", "dense"]
    assert p["chain"]["first"] == -1
    p = plan_of(driver, 480, 640, 2)
    head, c3 = p["head"], p["layers"][2]
    assert (head["on"], head["runs"], head["wsplit"], head["w2p"], head["cpr"], head["R2"], head["bands"], head["lds"]) == (1, 1, 4, 40, 32, 5, 24, 129664)
    assert (c3["frame5"], c3["frame5_bands"], c3["frame5_ohb"], c3["frame5_lds"]) == (1, 29, 2, 140928)
    assert [l["frame"] for l in p["layers"][3:7]] == [0, 0, 0, 0]
    assert [l["served_by"] for l in p["layers"]] == ["band<split>", "band<split>", "frame5", "lt<2>", "lt<2>", "lt<2>", "lt<2>", "dense"]
    assert p["chain"]["first"] == -1
    for l in p["layers"][3:7]:
        assert (l["res_nb"], l["res_block"], l["res_lds"]) == ((2, 448, 162624) if l["i"] == 6 else (2, 1024, 107040))


@pytest.mark.parametrize("size,n_cap", [((96, 100), 37), ((96, 100), 1027), ((120, 100), 5), ((120, 96), 5)])
def test_a_layer_one_pixel_wide_stays_off_the_kernels_that_divide_by_its_width(driver, size, n_cap):
    """Frames 96 and 100 wide leave conv7 one pixel wide.  trs_conv_frame_kernel and trs_conv_chain_kernel turn a pixel index into (frame, row, column) with
    pilot_magic(OH x OW) and pilot_magic(OW), and pilot_magic(1) is 2^32 cut to 0: every quotient 0.  The chain at 96x100 gave the second frame of every
    workgroup the first one's conv7 window (found by tests/test_pilot_fallback.py, A at 96x100).  The plan keeps such a layer on the quad-load kernel, and with
    conv7 off the frame kernel there is no chain."""
    h, w = size
    p = plan_of(driver, h, w, n_cap)
    c7 = p["layers"][6]
    assert c7["OW"] == 1 and c7["OH"] == {96: 1, 120: 4}[h] and c7["frame"] == 0
    assert [l["served_by"] for l in p["layers"][2:]] == ["frame5", "frame", "frame", "frame", "lt<2>", "dense"] and p["chain"]["first"] == -1
    assert all(l["frame"] == 1 and l["OW"] >= 3 for l in p["layers"][3:6])
    assert (c7["res_nb"], c7["res_ysplit"], c7["res_block"], c7["res_lds"]) == (2, 2, 448, 162624)
    assert plan_of(driver, h, w, n_cap, chain_layers=3)["chain"]["first"] == -1
    wider = plan_of(driver, h, 104, n_cap)                                    # the next legal width: conv7 two pixels wide, the chain as everywhere
    assert wider["layers"][6]["OW"] == 2 and wider["chain"]["first"] == 3 and [l["served_by"] for l in wider["layers"][3:7]] == ["chain"] * 4


def test_no_plan_hands_pilot_magic_a_divisor_of_one(driver):
    """Every divisor the plan turns into a pilot_magic factor is 2 or more: OW and the unit's pixels of a layer on the frame kernel or in the chain, conv3's OW on
    trs_conv_frame5_kernel, the head's part width and chunks per row.  All legal widths from 64 to 320, two heights."""
    for w in range(64, 324, 4):
        for h in (96, 121):
            for kind, r in map(parse, run_driver(driver, "plan", h, w, 37, 256, 22)):
                where = (kind, h, w, r.get("i"))
                if kind == "layer" and (r["frame"] or r["frame5"]):
                    assert r["OW"] >= 2 and r["OH"] * r["OW"] >= 2, where
                elif kind == "head" and r["on"] and r["wsplit"] > 1:
                    assert r["magic_full"] > 0 and r["magic_cpr"] > 0 and r["cpr"] >= 2 and r["w2p"] >= 2, where
                elif kind == "chain" and r["first"] >= 0:
                    assert all(r[f"magic_uout{j}"] > 0 and r[f"magic_ow{j}"] > 0 for j in range(r["nl"])), where


@pytest.mark.parametrize("layer,n,tiles,waves", [(1, 267, 3855, 3840), (2, 1619, 4099, 4096)])
def test_batches_that_make_the_quad_load_kernel_loop(driver, layer, n, tiles, waves):
    """96x100 under FALLBACK on 256 CUs: 267 frames give conv2 (462 pixels a frame, 768 workgroups of 5 waves) and 1,619 give conv3 (81 pixels a frame,
    256 workgroups of 16 waves) more tiles than resident waves, so some waves take a second tile; each is the smallest odd batch that does, and its
    last tile is ragged."""
    p = plan_of(driver, 96, 100, n, **FALLBACK)
    assert persistent_batch(p, layer, 256) == n
    assert tiles_and_waves(p, call_of(driver, 96, 100, n, n, **FALLBACK), layer, n) == (tiles, waves) and tiles > waves
    assert n * p["layers"][layer]["OH"] * p["layers"][layer]["OW"] % 32 != 0
    first = 32 * waves // (p["layers"][layer]["OH"] * p["layers"][layer]["OW"]) + 1     # the first batch that loops: n, or the even one in front of it
    assert first in (n, n - 1)
    t, w = tiles_and_waves(p, call_of(driver, 96, 100, n, first - 1, **FALLBACK), layer, first - 1)
    assert t <= w, (first - 1, t, w)


def test_refusals_come_back_through_the_plan(driver):
    small = plan_of(driver, 28, 160, 4)
    assert small["refuse"] == {"H": 28, "W": 160, "n_cap": 4, "code": -5, "text": REFUSALS[0]} and not small["layers"]


# ---- (b) properties of every plan ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [64, 132, 160, 300, 320])
@pytest.mark.parametrize("n_cap", [1, 37, 1027])
def test_every_plan_fits_and_is_aligned(driver, w, n_cap):
    seen, planned = set(), 0
    for kind, r in map(parse, run_driver(driver, "plan", "29:260", w, n_cap, 256, 22)):
        seen.add(r["H"])
        where = (kind, r["H"], w, n_cap, r.get("i"))
        if kind == "refuse":
            assert r["code"] == -5 and r["text"] in REFUSALS, where
        elif kind == "layer":
            planned += r["i"] == 0
            assert r["i"] == 7 or 0 < r["res_lds"] <= LDS_BYTES, where
            for tag in ("frame", "frame5"):
                if r[tag]:
                    bands, ohb = r[tag + "_bands"], r[tag + "_ohb"]
                    assert 0 < r[tag + "_lds"] <= LDS_BYTES, where
                    assert bands * ohb >= r["OH"] > (bands - 1) * ohb, where
        elif kind == "head" and r["on"]:
            assert r["lds"] <= LDS_BYTES, where
            for off in ("off_w2", "off_b", "off_tile", "off_band"):
                assert r[off] % 16 == 0 and 0 < r[off] < r["lds"], (where, off)
            assert r["off_w2"] < r["off_b"] < r["off_tile"] and r["off_tile"] + r["tile_bytes"] <= r["off_band"] and r["off_band"] + r["band_bytes"] == r["lds"], where
        elif kind == "chain" and r["first"] >= 0:
            assert r["lds"] <= LDS_BYTES, where
            for off in ("offA", "offB", "off_bias"):
                assert r[off] % 16 == 0 and 0 <= r[off] < r["lds"], (where, off)
            assert r["offA"] < r["offB"] < r["off_bias"], where
    assert seen == set(range(29, 261))                                       # every size answered: a plan or a refusal
    assert planned > 100 if w > 64 else planned == 0                         # (a frame 64 wide is too small for the seven convolutions)


@pytest.mark.parametrize("w", [64, 132, 160, 300, 320])
def test_dense1_slices_cover_k_and_frame_groups_cover_the_batch(driver, w):
    pat = re.compile(r" n=(\d+) G=(\d+) nf=(\d+) gps=(\d+) KS=(\d+) groups=(\d+) dense_grid=(\d+) dense_lds=(\d+) ")
    lines = 0
    for line in run_driver(driver, "call", "29:260", w, 1027, 256, 22, "1:300", "show=brief"):
        if not line.startswith("call "):
            assert line.startswith("refuse "), line
            continue
        n, g, nf, gps, ks, groups, grid, lds = map(int, pat.search(line).groups())
        lines += 1
        assert ks * gps >= g > (ks - 1) * gps, line
        assert grid % 8 == 0 and grid >= groups * ks, line
        assert groups * 32 * nf >= n and nf in (1, 2) and lds <= LDS_BYTES, line
    assert lines > 100 * 300 if w > 64 else lines == 0


# ---- (c) packing ---------------------------------------------------------------------------------------------------------------------------

def fp16_bits(x):
    return np.clip(x.astype(np.float32), -65504.0, 65504.0).astype(np.float16).view(np.uint16)


def numpy_pack(i, ih, iw, kernel):
    """The granule layout as the kernels' comments state it: [g][cout padded to 32][8 input values] of fp16 and, per granule, the byte offset of its
    8 values from the output pixel's first input byte.  A kernel row is one run of KW x CIN input values in NHWC order, padded with zero granules to
    a multiple of 4; conv1's run is the 15 bytes of 5 RGB pixels + 1, in two granules, its weights x 256 / 255; dense1 is one run."""
    if i == 7:
        cin, cout = kernel.shape
        rows = [kernel]
        px_bytes, row_bytes, cout_pad = 2, 0, 128
    else:
        kh, kw, cin, cout = kernel.shape
        rows = [kernel[r].reshape(kw * cin, cout) for r in range(kh)]
        px_bytes, row_bytes, cout_pad = (1, iw * 3, 32) if i == 0 else (2, iw * cin * 2, (cout + 31) // 32 * 32)
    if i == 0:
        rows = [np.concatenate([r * (np.float32(256.0) / np.float32(255.0)), np.zeros((1, cout), np.float32)]) for r in rows]
    run = rows[0].shape[0] // 8
    run_pad = run if i == 0 else (run + 3) // 4 * 4
    g_real = len(rows) * run_pad
    g_pad = (g_real + 3) // 4 * 4
    w = np.zeros((g_pad, cout_pad, 8), np.uint16)
    goff = np.zeros(g_pad, np.int32)
    is_padding = np.ones(g_pad, bool)
    for r, row in enumerate(rows):
        for gi in range(run_pad):
            g = r * run_pad + gi
            goff[g] = r * row_bytes + gi * 8 * px_bytes
            if gi < run:
                w[g, :cout, :] = fp16_bits(row[gi * 8:gi * 8 + 8]).T
                is_padding[g] = False
    goff[g_real:] = goff[g_real - 1]
    return w, goff, is_padding, cout_pad


def glorot(rng, shape):
    fan = (shape[0] * shape[1] * (shape[2] + shape[3])) if len(shape) == 4 else sum(shape)
    lim = math.sqrt(6.0 / fan)
    return rng.uniform(-lim, lim, shape).astype(np.float32)


def pack(driver, tmp_path, i, ih, iw, kernel, bias):
    (tmp_path / "k.bin").write_bytes(np.ascontiguousarray(kernel, np.float32).tobytes())
    (tmp_path / "b.bin").write_bytes(np.ascontiguousarray(bias, np.float32).tobytes())
    lines = run_driver(driver, "pack", i, ih, iw, tmp_path / "k.bin", tmp_path / "b.bin", tmp_path / "out")
    return lines, {ext: np.fromfile(tmp_path / f"out.{ext}", dtype) for ext, dtype in (("w", np.uint16), ("goff", np.int32), ("bias", np.float32))}


@pytest.mark.parametrize("i,ih,iw", [(0, 16, 16), (1, 16, 16), (3, 16, 16), (7, 1, 5)], ids=["conv1", "conv2", "conv4", "dense1-G80"])
def test_packing_equals_the_numpy_restatement(driver, tmp_path, i, ih, iw):
    rng = np.random.default_rng(40 + i)
    shape = (ih * iw * 128, 100) if i == 7 else (SPEC[i][0], SPEC[i][0], SPEC[i][2], SPEC[i][3])
    kernel = glorot(rng, shape)
    kernel.reshape(-1)[:4] = [7.0e4, -7.0e4, 3.0e-6, 1.0e-9]                 # beyond the range (saturates), a binary16 subnormal, below the smallest one
    bias = rng.uniform(-0.05, 0.05, shape[-1]).astype(np.float32)
    lines, got = pack(driver, tmp_path, i, ih, iw, kernel, bias)
    head = parse(lines[0])[1]
    want_w, want_goff, is_padding, cout_pad = numpy_pack(i, ih, iw, kernel)
    assert (head["G_pad"], head["COUT_PAD"]) == (len(want_goff), cout_pad) and (i != 7 or head["G"] == 80) and (i != 1 or (head["run"], head["run_pad"]) == (15, 16))
    assert np.array_equal(got["w"].reshape(want_w.shape), want_w)
    assert np.array_equal(got["goff"], want_goff)
    assert np.array_equal(got["bias"], np.concatenate([bias, np.zeros(cout_pad - len(bias), np.float32)]))
    # the padding granules: zero weights on an address inside the input of the first output pixel's frame
    assert is_padding.sum() == {0: 2, 1: 5, 3: 0, 7: 0}[i]
    assert not got["w"].reshape(want_w.shape)[is_padding].any()
    assert (got["goff"] >= 0).all() and (got["goff"] + 16 <= head["in_bytes"]).all()
    if i == 1:
        # trs_conv12_band_kernel reads a window as two runs, the even conv1 columns (3 pixels = 9 granules of 8 channels) then the odd (2 pixels = 6): conv2's
        # granules are packed in that order for it, the row's padding granule last
        order = [kw * 3 + c8 for kw in (0, 2, 4) for c8 in range(3)] + [kw * 3 + c8 for kw in (1, 3) for c8 in range(3)] + [15]
        assert [int(x) for x in lines[1].split()[1:]] == order
        parity = np.fromfile(tmp_path / "out.parity", np.uint16).reshape(5, 16, cout_pad, 8)
        assert np.array_equal(parity, want_w.reshape(5, 16, cout_pad, 8)[:, order])


def test_conv1_bound_for_the_fused_heads_epilogue(driver, tmp_path):
    rng = np.random.default_rng(7)
    kernel, bias = glorot(rng, (5, 5, 3, 24)), rng.uniform(-0.05, 0.05, 24).astype(np.float32)

    def bounded(k):
        lines, _ = pack(driver, tmp_path, 0, 16, 16, k, bias)
        return int(lines[1].split()[1])

    assert bounded(kernel) == 1
    assert bounded(kernel * np.float32(3e5)) == 0
    with_nan = kernel.copy()
    with_nan[2, 3, 1, 17] = np.nan
    assert bounded(with_nan) == 0


# ---- (d) the tail's blob of small fp32 weights ---------------------------------------------------------------------------------------------

TAIL_SLOTS = ["feature1.k", "feature1.b", "feature2.k", "feature2.b", "feature3.k", "feature3.b", "dense1.behind", "dense2.k", "dense2.b", "dense3.k", "dense3.b",
              "out.k", "out.b", "current_spd_1.k", "current_spd_1.b", "current_spd_2.k", "current_spd_2.b", "current_spd_3.k", "current_spd_3.b", "dense4.behind",
              "dense5.k", "dense5.b", "dense6.k", "dense6.b", "out_steering.k", "out_steering.b"]          # XO_* in order


def keras_arrays(rng, h, w, n_arrays):
    """([(layer name, kernel, bias)] in trs_pilot_load's order, F): every array at its Keras shape (include/trsim.h; keras_train.py:127-174, 184-245)."""
    ih, iw = h, w
    layers = []
    for i, (k, s, cin, cout) in enumerate(SPEC):
        ih, iw = (ih - k) // s + 1, (iw - k) // s + 1
        layers.append((f"conv{i + 1}", (k, k, cin, cout)))
    flat = ih * iw * 128
    f = {22: None, 28: (4, 8, 16), 42: (16, 32, 64)}[n_arrays]
    layers += [("dense1", (flat + (f[2] if f else 0), 100)), ("dense2", (100, 50)), ("dense3", (50, 25)), ("out", (25, 1 if n_arrays == 42 else 2))]
    if f:
        layers += [("feature1", (1, f[0])), ("feature2", (f[0], f[1])), ("feature3", (f[1], f[2]))]
    if n_arrays == 42:
        layers += [("current_spd_1", (1, f[0])), ("current_spd_2", (f[0], f[1])), ("current_spd_3", (f[1], f[2])),
                   ("dense4", (flat + 2 * f[2], 100)), ("dense5", (100, 50)), ("dense6", (50, 25)), ("out_steering", (25, 1))]
    assert 2 * len(layers) == n_arrays
    return [(nm, rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape[-1]).astype(np.float32)) for nm, shape in layers], flat


@pytest.mark.parametrize("h,w", [(120, 160), (100, 132)])
@pytest.mark.parametrize("n_arrays", [22, 28, 42])
def test_tail_blob_equals_the_numpy_restatement(driver, tmp_path, h, w, n_arrays):
    """pack_tail_blob: every slot is one Keras array, whole, or the rows of dense1 / dense4 behind the flatten; slots lie back to back in XO_* order, the ones an
    architecture lacks at offset 0.  The driver holds every array on the heap at exactly its size under ASan: reading past dense1 or dense4 would stop it."""
    layers, flat = keras_arrays(np.random.default_rng(n_arrays + h), h, w, n_arrays)
    for k, a in enumerate(a for _, kern, bias in layers for a in (kern, bias)):
        (tmp_path / f"a{k}.bin").write_bytes(a.tobytes())
    (line,) = run_driver(driver, "blob", h, w, n_arrays, tmp_path, tmp_path / "out")
    rec = parse(line)[1]
    got = np.fromfile(tmp_path / "out.blob", np.float32)
    parts = {}
    for nm, kern, bias in layers:
        parts[nm + ".k"], parts[nm + ".b"] = kern.reshape(-1), bias
    for nm in ("dense1", "dense4"):
        if nm + ".k" in parts:
            parts[nm + ".behind"] = parts[nm + ".k"].reshape(-1, 100)[flat:].reshape(-1)
    have = [s for s in TAIL_SLOTS if s in parts and (n_arrays != 22 or not s.endswith(".behind"))]
    want, offsets, at = [], {}, 0
    for s in have:
        offsets[s] = at
        want.append(parts[s])
        at += parts[s].size
    want = np.concatenate(want)
    widths = {22: (0, 0, 0), 28: (4, 8, 16), 42: (16, 32, 64)}[n_arrays]
    assert (rec["arch"], rec["F"], rec["slots"]) == ({22: 0, 28: 2, 42: 3}[n_arrays], flat, len(TAIL_SLOTS))
    assert (rec["f1"], rec["f2"], rec["f3"]) == widths and rec["floats"] == want.size
    assert [rec[f"xo{k}"] for k in range(len(TAIL_SLOTS))] == [offsets.get(s, 0) for s in TAIL_SLOTS]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len(have) == {22: 6, 28: 13, 42: 26}[n_arrays]
