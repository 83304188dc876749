"""A pass of the pilot as data (csrc/trsim_pilot_pass.hpp) on the CPU: tests/pilot_plan_driver.cpp, built with AddressSanitizer + UBSan, prints what pilot_pass and
pilot_materialise schedule and the parameter block of every launch; the tests hold them against a restatement written here from the kernels' comments.  The sweep:
every frame height 60..260 at four widths, batch capacities 1, 37 and 1024, batches of 1 and of the capacity, 22 and 42 weight arrays, the default tuning and six
single departures from it, 256 CUs."""
import functools
import re

import numpy as np
import pytest

from test_pilot_plan_cpu import LDS_BYTES, SPEC, driver, parse, run_driver          # noqa: F401  (driver is a fixture)

CUS = 256
WIDTHS = [100, 128, 160, 320]
TUNINGS = [{}, {"no_fuse": 1}, {"chain_layers": 0}, {"chain_layers": 3}, {"frame_layers_mask": 0}, {"frame5": 0}, {"span_layers_mask": 0}]
CAPS_AND_BATCHES = [(1, 1), (37, 1), (37, 37), (1024, 1), (1024, 1024)]
FRAMES_TEXT, ACT_TEXT = "frames larger than 2 GiB: lower the batch", "activation larger than 2 GiB: lower the batch"
FRAME_BLOCK, FRAME5_BLOCK, CHAIN_BLOCK = 64 * (8 + 4), 64 * (4 + 4), 512           # 8 compute + 4 loader waves; 4 + 4; 8 waves
ids = lambda t: "-".join(f"{k}{v}" for k, v in t.items()) or "default"


def geometry(h, w):
    """[(IH, IW, OH, OW, CIN, COUT)] of conv1..conv7 ('valid' convolutions of Keras_2D_CNN)"""
    out = []
    for k, s, cin, cout in SPEC:
        oh, ow = (h - k) // s + 1, (w - k) // s + 1
        out.append((h, w, oh, ow, cin, cout))
        h, w = oh, ow
    return out


@functools.lru_cache(maxsize=None)
def magic_divides(magic, d, p_end):
    """floor(p / d) == umulhi(p, magic) for every p < p_end"""
    p = np.arange(p_end, dtype=np.uint64)
    return bool(np.array_equal((p * np.uint64(magic)) >> np.uint64(32), p // np.uint64(d)))


def up(x, m):
    return (x + m - 1) // m * m


def passes_of(exe, w, n_cap, n, arrays, tuning):
    """[(plan of H, call record, [(launch record, [(block kind, block record)])])] for H = 60..260, refused plans left out"""
    t = [f"{k}={v}" for k, v in tuning.items()]
    plans = {}
    for kind, r in map(parse, run_driver(exe, "plan", "60:260", w, n_cap, CUS, arrays, *t)):
        if kind != "refuse":
            p = plans.setdefault(r["H"], {"layers": []})
            p["layers"].append(r) if kind == "layer" else p.__setitem__(kind, r)
    out = []
    for kind, r in map(parse, run_driver(exe, "call", "60:260", w, n_cap, CUS, arrays, n, *t)):
        if kind == "call":
            out.append((plans[r["H"]], r, []))
        elif kind == "launch":
            out[-1][2].append((r, []))
        elif kind != "refuse":
            out[-1][2][-1][1].append((kind, r))
    assert len(out) == len(plans) > 0
    return out


def check_schedule(plan, call, launches, h, w, n, arrays):
    geo = geometry(h, w)
    elems = lambda buf: h * w if buf == -1 else geo[buf][2] * geo[buf][3] * geo[buf][5]
    where = (h, w, n, arrays)
    # 1. conv1..conv7 each by exactly one launch, ascending; then dense1, and dense4 for 42 arrays; both read conv7's activation
    convs = [(l, b) for l, b in launches if l["first"] < 7]
    assert [i for l, _ in convs for i in range(l["first"], l["last"] + 1)] == list(range(7)), where
    tail = [l for l, _ in launches[len(convs):]]
    assert [(l["first"], l["last"], l["dst"], l["src"], l["kind"]) for l in tail] == [(j, j, j, 6, "dense") for j in range(7, 9 if arrays == 42 else 8)], where
    assert call["count"] == len(launches)
    # 2. every launch reads what the one before it wrote, the first the frames; in_bytes is that buffer's size
    src = -1
    for l, _ in convs:
        assert l["src"] == src and l["dst"] == l["last"], (where, l)
        src = l["dst"]
    for l, _ in launches:
        assert l["in_bytes"] == n * elems(l["src"]) * (3 if l["src"] == -1 else 2), (where, l)
        assert 1 <= l["grid_x"] and 1 <= l["grid_y"] and 0 < l["lds"] <= l["lds_max"] <= LDS_BYTES, (where, l)
    # the flags after a pass: conv1's activation is there when conv1 ran as its own layer, the chain's interior when there is no chain
    kinds = [l["kind"] for l, _ in convs]
    assert call["act0_valid"] == int(kinds[0] == "u8") and call["chain_mid_valid"] == int("chain" not in kinds), where
    # 3. and 4. per kernel: the grid within the bound its grid function states, the block size it is built for, the integers of its block
    for l, blocks in launches:
        i, pl = l["first"], plan["layers"][l["first"]]
        (bkind, b), rest = blocks[0], blocks[1:]
        g = geo[i] if i < 7 else None
        at = (where, l, b)
        if l["kind"].startswith("band"):
            head, (_, c2) = plan["head"], rest[0]
            assert l["block"] == 1024 and l["lds"] == l["lds_max"] == head["lds"] and l["grid_y"] == 1, at
            parts = max(1, head["wsplit"])
            assert l["grid_x"] <= min(CUS, n * head["bands"] * parts) and (l["kind"] == "band<split>") == (head["wsplit"] > 1), at
            assert (b["frames_bytes"], b["N"], b["IH"], b["IW"]) == (n * h * w * 3, n, h, w), at
            assert (b["OH1"], b["OW1"], b["OH2"], b["OW2"]) == (geo[0][2], geo[0][3], geo[1][2], geo[1][3]), at
            assert all(b[k] == head[k] for k in ("R2", "bands", "off_w2", "off_b", "off_tile", "tile_bytes", "off_band", "band_bytes", "wsplit", "w2p", "cpr")), at
            assert b["roll"] == call["roll"] and (not b["roll"] or (n * parts >= CUS and head["bands"] > 1)), at
            assert (c2["M"], c2["nt_out"], c2["COUT"], c2["COUT_PAD"], c2["oscale_bits"]) == (n * geo[1][2] * geo[1][3], 0, 32, 32, 0x3F800000), at
            if head["wsplit"] > 1:                                             # a part's conv1 tile is (2 R2 + 3) rows of w1 = 2 w2p + 3 columns; its staged rows have cpr chunks
                w1, rows_in = 2 * b["w2p"] + 3, 2 * (2 * b["R2"] + 3) + 3
                assert magic_divides(b["magic_full"], w1, up((2 * b["R2"] + 3) * w1, 32)) and magic_divides(b["magic_cpr"], b["cpr"], rows_in * b["cpr"]), at
        elif l["kind"] == "chain":
            ch = plan["chain"]
            assert i == ch["first"] and l["last"] == 6 and ch["nl"] == 7 - i and l["block"] == CHAIN_BLOCK and l["lds"] == l["lds_max"] == ch["lds"], at
            assert l["grid_x"] == -(-n // ch["F"]) and l["grid_y"] == 1, at     # F frames per workgroup
            assert (b["N"], b["F"], b["nl"], b["split_first"], b["offA"], b["offB"], b["off_bias"]) == (n, ch["F"], ch["nl"], ch["split_first"], ch["offA"], ch["offB"], ch["off_bias"]), at
            for j in range(ch["nl"]):
                ih, iw, oh, ow, cin, cout = geo[i + j]
                f = lambda k: b[f"{k}{j}"]
                assert (f("IH"), f("IW"), f("OH"), f("OW"), f("COUT"), f("cg"), 1 << f("cgs")) == (ih, iw, oh, ow, cout, cin // 8, cin // 8), (at, j)
                assert (f("nt"), f("nb")) == (ch[f"nt{j}"], ch[f"nb{j}"]) and f("nt") in (2, 3) and f("nb") in (1, 2), (at, j)
                px = up(ch["F"] * oh * ow, 32 * f("nt"))                         # pixels of a workgroup's frames, in whole items
                assert magic_divides(f("magic_uout"), oh * ow, px) and magic_divides(f("magic_ow"), ow, up(oh * ow, 32)), (at, j)
        elif l["kind"] == "frame":
            ih, iw, oh, ow, cin, cout = g
            assert l["block"] == FRAME_BLOCK and (l["lds"], l["lds_max"]) == (pl["frame_lds"], LDS_BYTES) and l["grid_y"] == 1, at
            assert l["grid_x"] == min(-(-n * b["bands"] // b["F"]), CUS), at     # one persistent workgroup per CU walks the groups of F units
            assert (b["N"], b["IH"], b["IW"], b["OH"], b["OW"], b["COUT"], b["COUT_PAD"], b["KH"], b["KW"]) == (n, ih, iw, oh, ow, cout, cout, 3, 3), at
            assert (b["F"], b["bands"], b["ohb"]) == (pl["frame_f"], pl["frame_bands"], pl["frame_ohb"]) and b["ihb"] == b["ohb"] + 3 - 1, at
            assert b["cg"] == cin // 8 == b["instance"] and 1 << b["cgs"] == b["cg"], at
            uout = b["ohb"] * ow
            assert magic_divides(b["magic_uout"], uout, up(b["F"] * uout, 64)) and magic_divides(b["magic_ow"], ow, up(uout, 64)), at
            assert b["magic_bands"] == 0 if b["bands"] == 1 else magic_divides(b["magic_bands"], b["bands"], n * b["bands"] + b["F"]), at
        elif l["kind"] == "frame5":
            ih, iw, oh, ow, cin, cout = g
            assert i == 2 and l["block"] == FRAME5_BLOCK and (l["lds"], l["lds_max"]) == (pl["frame5_lds"], LDS_BYTES) and l["grid_y"] == 1, at
            assert l["grid_x"] == min(n * b["bands"], CUS), at                   # one persistent workgroup per CU walks the units
            assert (b["N"], b["IH"], b["IW"], b["OH"], b["OW"], b["F"], b["COUT"]) == (n, ih, iw, oh, ow, 1, 64) and b["ev"] == (iw + 1) // 2, at
            assert (b["bands"], b["ohb"]) == (pl["frame5_bands"], pl["frame5_ohb"]) and b["ihb"] == (ih if b["bands"] == 1 else 2 * b["ohb"] + 3), at
            assert magic_divides(b["magic_ow"], ow, up(b["ohb"] * ow, 64)), at
        elif l["kind"] == "dense":
            assert l["block"] == 256 and l["lds"] == l["lds_max"] == call["dense_lds"] and l["grid_x"] == call["dense_grid"] and l["grid_y"] == 1, at
            assert (b["n"], b["G"], b["gps"], b["KS"], b["groups"], b["nf"]) == (n, geo[6][2] * geo[6][3] * 16, call["gps"], call["KS"], call["groups"], call["nf"]), at
            assert b["KS"] * b["gps"] >= b["G"] > (b["KS"] - 1) * b["gps"] and b["groups"] * 32 * b["nf"] >= n and l["grid_x"] >= b["groups"] * b["KS"], at
        else:
            ih, iw, oh, ow, cin, cout = g
            assert bkind == "conv" and l["kind"] in ("u8", "span<1>", "span<2>", "lt<1>", "lt<2>") and (l["kind"] == "u8") == (i == 0), at
            assert (l["block"], l["grid_y"], l["lds"], l["lds_max"]) == (pl["res_block"], pl["res_ysplit"], pl["res_lds"], pl["res_lds"]), at
            tiles, waves = -(-n * oh * ow // 32), pl["res_block"] // 64
            assert l["grid_x"] <= max(1, min(-(-tiles // waves), CUS * pl["res_wg_per_cu"])) and (i == 0 or l["kind"].endswith(f"<{pl['res_nb']}>")), at
            px = 3 if i == 0 else cin * 2
            assert (b["N"], b["IH"], b["IW"], b["CIN"], b["OH"], b["OW"], b["COUT"], b["COUT_PAD"], b["S"]) == (n, ih, iw, cin, oh, ow, cout, up(cout, 32), SPEC[i][1]), at
            assert (b["M"], b["in_px_bytes"], b["in_bytes"]) == (n * oh * ow, px, n * ih * iw * px) and b["in_bytes"] == l["in_bytes"], at
            assert b["nt_out"] == int(n * oh * ow * cout * 2 > 128 << 20), at    # outputs above 128 MB leave non-temporally
            assert (b["KH"], b["KW"], b["G"], b["G_pad"], b["run_pad"], b["span_nl"]) == (SPEC[i][0], SPEC[i][0], pl["G"], pl["G_pad"], pl["run_pad"], pl["span_nl"]), at
            assert (b["cg"], b["oscale_bits"]) == ((0, 0x3B800000) if i == 0 else (cin // 8, 0x3F800000)), at     # conv1's sums x 2^-8; elsewhere x 1


@pytest.mark.parametrize("tuning", TUNINGS, ids=ids)
@pytest.mark.parametrize("w", WIDTHS)
def test_every_pass_covers_the_network_and_fills_its_blocks(driver, w, tuning):
    kinds = set()
    for arrays in (22, 42):
        for n_cap, n in CAPS_AND_BATCHES:
            for plan, call, launches in passes_of(driver, w, n_cap, n, arrays, tuning):
                check_schedule(plan, call, launches, call["H"], w, n, arrays)
                kinds.update(l["kind"] for l, _ in launches)
    assert "dense" in kinds and (tuning or ("frame5" in kinds and ("chain" in kinds or "frame" in kinds)))


MAT = re.compile(r"materialise H=(\d+) .* lo=(\d) hi=(\d) act0_valid=(\d) chain_mid_valid=(\d) code=0 count=(\d+) layers=(\S+) srcs=(\S+) after_act0_valid=(\d) after_chain_mid_valid=(\d) chain_first=(-?\d+) head_runs=(\d)")


@pytest.mark.parametrize("tuning", TUNINGS, ids=ids)
@pytest.mark.parametrize("w", WIDTHS)
def test_materialise_launches_what_is_needed_and_not_valid(driver, w, tuning):
    """pilot_materialise for every lo <= hi in 0..7 and all four flag pairs: conv1 exactly when lo..hi holds layer 0 and conv1's activation is not valid; the chain's
    interior conv(first + 1)..conv6, whole, exactly when lo..hi touches it and it is not valid; each launch reads the frames, a layer the pass stored, or one just
    written; afterwards a flag is set when it was set or its layers have just been launched."""
    seen = 0
    for arrays in (22, 42):
        for n_cap in (1, 37, 1024):
            lines = run_driver(driver, "materialise", "60:260", w, n_cap, CUS, arrays, n_cap, "0:7", "0:7", "0:1", "0:1", "show=brief", *[f"{k}={v}" for k, v in tuning.items()])
            for line in lines:
                if line.startswith("refuse "):
                    continue
                m = MAT.match(line)
                assert m, line
                h, lo, hi, a0, cm, count, layers, srcs, a0_after, cm_after, cf, head = (int(x) if re.fullmatch(r"-?\d+", x) else x for x in m.groups())
                interior = list(range(cf, 6)) if cf >= 0 else []
                want = ([0] if lo == 0 and not a0 else []) + (interior if interior and not cm and lo <= interior[-1] and hi >= interior[0] else [])
                got = [] if layers == "-" else [int(x) for x in str(layers).split(",")]
                assert got == want and count == len(want), line
                valid = {-1} | {i for i in range(7) if (i != 0 or a0) and (i not in interior or cm)}
                for layer, src in zip(got, [] if srcs == "-" else [int(x) for x in str(srcs).split(",")]):
                    assert src == layer - 1 and src in valid, line
                    valid.add(layer)
                assert (a0_after, cm_after) == (int(a0 or 0 in got), int(cm or (bool(interior) and interior[0] in got))), line
                seen += 1
    assert seen >= 6 * 36 * 4 * (100 if w > 100 else 1)


def test_materialise_prints_the_blocks_of_its_launches(driver):
    """120x160, 64 frames, layers 0..7 with nothing valid: conv1 by itself and conv4..conv6 on the frame kernel, each with its launch and block, from the right buffers"""
    lines = [parse(l) for l in run_driver(driver, "materialise", 120, 160, 64, CUS, 22, 64, 0, 7, 0, 0)]
    assert [k for k, _ in lines] == ["materialise", "launch", "conv", "launch", "frame", "launch", "frame", "launch", "frame"]
    assert [(r["kind"], r["first"], r["src"], r["dst"]) for k, r in lines if k == "launch"] == [("u8", 0, -1, 0), ("frame", 3, 2, 3), ("frame", 4, 3, 4), ("frame", 5, 4, 5)]
    assert lines[2][1]["in_bytes"] == 64 * 120 * 160 * 3 and [r["ihb"] for k, r in lines if k == "frame"] == [12, 10, 8]


def smallest_over(per_frame):
    return (2 ** 31 - 1) // per_frame + 1


def test_the_two_refusals_at_2_gib(driver):
    """240x320.  Frames: the smallest batch whose frames pass 2^31 - 1 bytes is refused with the frames' text by the fused head, which reads them; one frame fewer is
    not refused for its frames (conv2's output, 57 x 77 x 32 fp16, is larger than a frame: conv3 refuses that batch for its input).  Activations (no_fuse = 1): the
    largest input of a single-layer launch is conv1's output, 118 x 158 x 24 fp16; the smallest batch at which it passes 2^31 - 1 bytes is refused, one fewer runs."""
    h, w = 240, 320
    geo = geometry(h, w)

    def outcome(n, **tuning):
        (line,) = run_driver(driver, "call", h, w, n, CUS, 22, n, "show=brief", *[f"{k}={v}" for k, v in tuning.items()])
        kind, r = parse(line)
        return (r["code"], r["text"]) if kind == "refuse" else None

    n = smallest_over(h * w * 3)
    assert n * h * w * 3 > 2 ** 31 - 1 >= (n - 1) * h * w * 3
    assert outcome(n) == (-5, FRAMES_TEXT)
    act1 = geo[1][2] * geo[1][3] * geo[1][5] * 2
    assert act1 > h * w * 3 and outcome(n - 1) == (-5, ACT_TEXT) and outcome(smallest_over(act1)) == (-5, ACT_TEXT) and outcome(smallest_over(act1) - 1) is None
    inputs = [h * w * 3] + [g[2] * g[3] * g[5] * 2 for g in geo[:6]]           # what conv1..conv7 read, per frame
    n = smallest_over(max(inputs))
    assert max(inputs) == inputs[1] == 118 * 158 * 24 * 2
    assert outcome(n, no_fuse=1) == (-5, ACT_TEXT) and outcome(n - 1, no_fuse=1) is None


def test_a_buffer_of_exactly_2_gib_is_refused(driver):
    """The first size refused is 2^31 bytes (an int holds one less).  2^31 - 1 is prime and every buffer's size is a product, so only a buffer of exactly 2^31 bytes
    tells '>= 2^31' from '> 2^31'.  150x152: conv3's output is 16 x 16 x 64 fp16 = 2^15 bytes a frame, and materialising the chain's interior launches conv4 on it by itself:
    65,536 frames are refused, 65,535 are not."""
    h, w, n = 150, 152, 65536
    assert geometry(h, w)[2][2:4] == (16, 16) and n * 16 * 16 * 64 * 2 == 2 ** 31

    def outcome(n):
        (line,) = run_driver(driver, "materialise", h, w, 65536, CUS, 22, n, 3, 5, 1, 0, "show=brief")
        r = parse(line)[1]
        assert r["chain_first"] == 3
        return r["code"], r.get("text"), r["count"]

    assert outcome(n) == (-5, ACT_TEXT, 0) and outcome(n - 1) == (0, None, 3)
