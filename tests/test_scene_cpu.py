"""The host-only owner of a handle's scene (csrc/trsim_scene.hpp) on the CPU, built with AddressSanitizer + UBSan as a stand-alone program on the
product's tables: which colours the host filters under which combination of frame filter, lighting and lens; the uniform-row count; and the byte
images the kernels read (the lens planes and palette, the dynamic filter's table, the colour half of the block behind the raster image), against the
oracle and numpy restatements of the layouts the kernels' comments state."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import track_points
from test_image_path import FUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKS = ["generated", "mountain"]                       # flat | with elevation
SHAPES = [(2, 8), (7, 8), (64, 64)]                      # the smallest frame, an odd height, and one whose flat palette has sky, ground and far rows
LENS = (1.5, 0.3)
V_DEPTH, V_DYN, V_HILLS, V_LENS, V_LIGHT = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def scene_driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("scene") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "scene_driver.cpp"),
                           os.path.join(ROOT, "triton-racer-sim_amd", "csrc", "trsim_tables.cpp")])
    return str(exe)


def run_driver(scene_driver, *args):
    out = subprocess.run([scene_driver, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def dynamic(cfg):
    return dict(cfg, preprocessing_dynamic_brightness_enabled=True)


@pytest.fixture()
def scene(scene_driver, oracle_api, make_env, tmp_path):
    """scene(track, (H, W), cfg=None, light=False, lens=False): the driver's lines, and its files as arrays under their suffixes."""
    from triton_racer_sim_amd import _ffi
    runs = []

    def _scene(track, shape, cfg=None, light=False, lens=False):
        d = tmp_path / str(len(runs))
        d.mkdir()
        runs.append(d)
        c = _ffi.TrsConfig()
        oracle_api.default_config(C.byref(c))
        c.n_envs, c.img_h, c.img_w = 2, shape[0], shape[1]
        (d / "cfg.bin").write_bytes(bytes(c))
        (d / "pts.bin").write_bytes(np.ascontiguousarray(track_points(track), dtype=np.float64).tobytes())
        pre = "-"
        if cfg is not None:
            pre = d / "pre.bin"
            pre.write_bytes(bytes(make_env("oracle", n_envs=1, track=None, render=False, img_h=2, img_w=4).pre_config(cfg)))
        got = run_driver(scene_driver, "scene", d / "cfg.bin", d / "pts.bin", pre, int(light), int(lens), LENS[0], LENS[1], d / "t")
        for name, dtype in (("raw", np.uint32), ("pal", np.uint32), ("sky", np.uint32), ("lens", np.float32), ("lensraw", np.uint32), ("lenspal", np.uint32),
                            ("lensimg", np.uint8), ("dyn", np.uint32)):
            if (d / f"t.{name}").exists():
                got["." + name] = np.fromfile(d / f"t.{name}", dtype=dtype)
        return got

    return _scene


def oracle_filtered(make_env, colours, cfg):
    """The oracle's ImgPreprocessing.__process of packed colours 0x00BBGGRR laid out as one frame of 4 columns (a palette's shape; the last row filled
    up by repetition, two rows at least: the smallest frame)."""
    n = len(colours)
    colours = np.resize(np.asarray(colours, np.uint32), (max((n + 3) // 4, 2), 4))
    frame = np.stack([colours & 255, (colours >> 8) & 255, (colours >> 16) & 255], -1).astype(np.uint8)[None]
    out = make_env("oracle", n_envs=1, track=None, render=False, img_h=frame.shape[1], img_w=4).preprocess_host(frame, cfg).astype(np.uint32)
    return (out[..., 0] | (out[..., 1] << 8) | (out[..., 2] << 16)).reshape(-1)[:n]


def leading_uniform_rows(pal):
    pal = pal.reshape(-1, 4)
    uniform = (pal == pal[:, :1]).all(axis=1)
    return int(np.argmin(uniform)) if not uniform.all() else len(pal)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("track", TRACKS)
def test_unfiltered_flat_palette_is_the_oracles(scene, make_env, track, shape):
    want = make_env("oracle", n_envs=1, img_h=shape[0], img_w=shape[1], track=track_points(track)).fetch("palette").reshape(-1)
    got = scene(track, shape)
    assert np.array_equal(got[".pal"], want) and np.array_equal(got[".raw"], want)
    assert int(got["variant"][0]) == (V_HILLS if track == "mountain" else 0)
    assert int(got["hill"][1]) == 0                                         # (no filter for the kernels either)


@pytest.mark.parametrize("cfg", FUSED)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("track", TRACKS)
def test_static_filter_is_applied_by_the_host_unless_lit_or_dynamic(scene, make_env, track, shape, cfg):
    """A static filter: the flat palette, the sky and the far colour are the oracle's filter of the raw ones, and the kernels get the filter (filt) for the
    colours they blend.  With lighting the host leaves all three raw (the kernels light, then filter: filt stays set); a dynamic filter is the kernels' alone."""
    got = scene(track, shape, cfg)
    raw = got[".raw"]
    assert np.array_equal(got[".pal"], oracle_filtered(make_env, raw, cfg))
    assert not np.array_equal(got[".pal"], raw)                             # (the configuration does filter this palette)
    plain = scene(track, shape)
    sky_far = np.concatenate([plain[".sky"], [np.uint32(int(plain["hill"][0]))]])
    assert np.array_equal(np.concatenate([got[".sky"], [np.uint32(int(got["hill"][0]))]]), oracle_filtered(make_env, sky_far, cfg))
    assert int(got["hill"][1]) == 1 and int(got["variant"][0]) & V_DYN == 0
    lit = scene(track, shape, cfg, light=True)
    assert np.array_equal(lit[".pal"], raw) and np.array_equal(lit[".sky"], plain[".sky"]) and lit["hill"][0] == plain["hill"][0]
    assert int(lit["hill"][1]) == 1 and int(lit["variant"][0]) & V_LIGHT
    dyn = scene(track, shape, dynamic(cfg))
    assert np.array_equal(dyn[".pal"], raw) and np.array_equal(dyn[".sky"], plain[".sky"]) and dyn["hill"][0] == plain["hill"][0]
    assert int(dyn["hill"][1]) == 0 and int(dyn["variant"][0]) & V_DYN


@pytest.mark.parametrize("cfg", FUSED)
@pytest.mark.parametrize("shape", SHAPES)
def test_lens_palette_is_filtered_and_never_lit(scene, make_env, shape, cfg):
    """The lens palette is filtered by the host whenever the filter is static — whatever light_on says: no LENS kernel lights — and raw otherwise."""
    got = scene("generated", shape, cfg, lens=True)
    raw = got[".lensraw"]
    assert raw.shape == (513 * 4,) and np.array_equal(scene("generated", shape, lens=True)[".lenspal"], raw)
    want = oracle_filtered(make_env, raw, cfg)
    assert np.array_equal(got[".lenspal"], want) and not np.array_equal(want, raw)
    assert np.array_equal(scene("generated", shape, cfg, light=True, lens=True)[".lenspal"], want)
    assert np.array_equal(scene("generated", shape, dynamic(cfg), lens=True)[".lenspal"], raw)
    assert int(got["variant"][0]) == V_LENS


@pytest.mark.parametrize("cfg", [None] + FUSED)
@pytest.mark.parametrize("shape", SHAPES)
def test_uniform_row_count(scene, shape, cfg):
    """The count that comes with the flat palette is the number of leading rows with four equal colours of THAT palette; none on a track with elevation or
    under a lens.  At 64 rows the flat track has uniform rows (sky, beyond the far plane) and rows that see the track."""
    H = shape[0]
    flat = scene("generated", shape, cfg)
    n = int(flat["uni_rows"][0])
    assert n == leading_uniform_rows(flat[".pal"]) and 0 <= n <= H
    if H == 64:
        assert 0 < n < H
    lit = scene("generated", shape, cfg, light=True)
    assert int(lit["uni_rows"][0]) == leading_uniform_rows(lit[".pal"])
    assert int(scene("mountain", shape, cfg)["uni_rows"][0]) == 0
    assert int(scene("generated", shape, cfg, lens=True)["uni_rows"][0]) == 0


def test_dynamic_table(scene):
    """kDynTabWords of FUSED[2] (three filters, two on channel 2: the later one owns the channel): OpenCV's reciprocals [512] | rngb[768]: entry c * 256 + x has
    byte ch = 0xFF when value x of component c lies inside the range of the filter that owns channel ch | sel: 0xFF in the channels that carry a mask (+ 3
    spare words) | cnt[256]: the class counts of a 4-pixel pack of 2-bit classes, n0 | n1 << 8 | n2 << 16 | n3 << 24."""
    cfg = dynamic(FUSED[2])
    t = scene("generated", (7, 8), cfg)[".dyn"]
    assert t.shape == (512 + 768 + 4 + 256,)
    i = np.arange(1, 256, dtype=np.float64)
    assert t[0] == 0 and t[256] == 0
    assert np.array_equal(t[1:256], np.rint((255 << 12) / i).astype(np.uint32))
    assert np.array_equal(t[257:512], np.rint((180 << 12) / (6 * i)).astype(np.uint32))
    bounds, chans = cfg["preprocessing_color_filter_hsvs"], cfg["preprocessing_color_filter_destination_channels"]
    owner = {ch: f for f, ch in enumerate(chans)}                           # a later filter on the same channel replaces an earlier one
    assert owner == {2: 2, 0: 1}
    want = np.zeros(768, np.uint32)
    for c in range(3):
        for x in range(256):
            for ch, f in owner.items():
                if min(bounds[f][0][c], 255) <= x <= min(bounds[f][1][c], 255):
                    want[c * 256 + x] |= 0xFF << (8 * ch)
    assert np.array_equal(t[512:1280], want)
    assert t[1280] == 0x00FF00FF and not t[1281:1284].any()
    cnt = np.array([sum(1 << (8 * ((p >> (2 * k)) & 3)) for k in range(4)) for p in range(256)], np.uint32)
    assert np.array_equal(t[1284:], cnt)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("track", TRACKS)
def test_lens_image_is_the_sliced_table(scene, track, shape):
    """F | L | D | M | palette: each plane [H][W/2] is the right half of the frame's table, M the low 16 bits of channel 3's bit pattern, every plane on a
    multiple of 256 bytes in that order without overlap, the palette (lens_palette, here filtered) at off_pal to the end."""
    H, W = shape
    wh = W // 2
    got = scene(track, shape, FUSED[0], lens=True)
    img, table = got[".lensimg"], got[".lens"].reshape(H, W, 4)[:, wh:, :]
    off_L, off_D, off_M, off_pal, size = (int(x) for x in got["lensimg"])
    assert all(o % 256 == 0 for o in (off_L, off_D, off_M, off_pal))
    assert H * wh * 4 <= off_L and off_L + H * wh * 4 <= off_D and off_D + H * wh * 4 <= off_M and off_M + H * wh * 2 <= off_pal
    assert size == len(img) == off_pal + 513 * 16
    for ch, off in enumerate((0, off_L, off_D)):
        assert np.array_equal(img[off:off + H * wh * 4].view(np.uint32), np.ascontiguousarray(table[..., ch]).reshape(-1).view(np.uint32)), ch
    rows = np.ascontiguousarray(table[..., 3]).reshape(-1).view(np.uint32)
    assert rows.max() <= 512
    assert np.array_equal(img[off_M:off_M + H * wh * 2].view(np.uint16), (rows & 0xFFFF).astype(np.uint16))
    assert np.array_equal(img[off_pal:].view(np.uint32), got[".lenspal"]) and not np.array_equal(got[".lenspal"], got[".lensraw"])


@pytest.mark.parametrize("cfg", FUSED)
def test_bounds_are_packed_once(scene_driver, scene, make_env, tmp_path, cfg):
    """One config's HSV bounds are the same numbers in the hill block's f_* fields, in FParams and in the dynamic filter's table, and they are h | s << 8 | v << 16."""
    pc = make_env("oracle", n_envs=1, track=None, render=False, img_h=2, img_w=4).pre_config(cfg)
    (tmp_path / "pre.bin").write_bytes(bytes(pc))
    got = run_driver(scene_driver, "bounds", tmp_path / "pre.bin")
    want = [v for k in range(4) for v in (pc.hsv_lo[k][0] | pc.hsv_lo[k][1] << 8 | pc.hsv_lo[k][2] << 16,
                                          pc.hsv_hi[k][0] | pc.hsv_hi[k][1] << 8 | pc.hsv_hi[k][2] << 16, pc.dst_channel[k])]
    assert [int(x) for x in got["bounds"]] == want
    assert got["hill_bounds"] == got["bounds"] == got["fparams_bounds"]
    assert [int(got["hill"][i]) for i in (1, 2, 3)] == [1, pc.color_filter_enabled, pc.n_filters] == [1] + [int(x) for x in got["fparams"][2:4]]
    assert got["hill"][4:6] == got["fparams"][4:6] and float(got["hill"][4]) == np.float32(pc.contrast_ratio) and float(got["hill"][5]) == np.float32(pc.contrast_offset)
    assert got["fparams"][:2] == ["40", "119"]
    # the table's masks, read back: per channel that carries a mask, the values of component c that are in range are exactly [lo, hi] of the owning filter
    t = scene("generated", (2, 8), dynamic(cfg))[".dyn"]
    owner = {pc.dst_channel[f]: f for f in range(pc.n_filters)}
    assert t[1280] == sum(0xFF << (8 * ch) for ch in owner)
    for ch, f in owner.items():
        for c in range(3):
            inside = np.nonzero((t[512 + c * 256:512 + (c + 1) * 256] >> (8 * ch)) & 0xFF)[0]
            lo, hi = (want[3 * f] >> (8 * c)) & 255, (want[3 * f + 1] >> (8 * c)) & 255
            assert np.array_equal(inside, np.arange(lo, hi + 1)), (ch, c)


def test_dynamic_filter_width_rule(scene_driver):
    """dyn_filter_width_ok, written with the brightness window's bounds, is the rule trs_set_frame_filter had as a literal: with rpp = 512 / (W / 4) rows per
    pass, refuse when rpp < 1 or ceil(79 / rpp) > 16."""
    got = {int(w): int(ok[0]) for w, ok in run_driver(scene_driver, "width").items()}
    assert sorted(got) == list(range(4, 1025, 4))
    for W, ok in got.items():
        rpp = 512 // (W // 4)
        assert ok == (0 if rpp < 1 or (79 + rpp - 1) // rpp > 16 else 1), W
    assert set(got.values()) == {0, 1}
