"""The lens camera's host tables (include/trsim_spec.h, "lens camera") on the CPU: the product's builder (csrc/trsim_tables.cpp,
build_lens_tables) built with AddressSanitizer + UBSan against an independent numpy binary64 restatement of the spec paragraph, bit for bit —
per pixel F, L, depth and palette row, and the 513-row lens palette — plus the properties the kernels rely on: the pinhole limit, a wider
horizontal field with a stronger lens, and the exact mirror symmetry that lets the device keep half the table."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import track_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOG_MAX = 0.65
BASE = np.array([[58, 132, 62], [92, 92, 98], [236, 236, 236], [232, 200, 40]], np.float64)
FOG = np.array([176, 196, 208], np.float64)
SKY_TOP, SKY_HOR = np.array([104, 156, 228], np.float64), np.array([192, 216, 240], np.float64)
SKY0, FAR = 256, 512
SIZES = [(60, 80), (120, 160), (240, 320)]
LENSES = [(0.5, 0.5, 0.0), (1.5, 0.3, 0.4), (0.0, 0.0, -0.6), (2.0, 2.0, 0.0)]


def _pack(rgb):
    rgb = np.floor(rgb + 0.5).astype(np.uint32)                          # round_colour: floor(v + 0.5), binary64
    return rgb[..., 0] | (rgb[..., 1] << 8) | (rgb[..., 2] << 16)


def spec_lens_palette():
    """uint32[513][4]: G(q) = the flat fog blend at TRS_FOG_MAX * ((q + 0.5) / 256), S(q) = the flat sky blend at g = (q + 0.5) / 256, FAR."""
    q = np.arange(256, dtype=np.float64)
    fw = FOG_MAX * ((q + 0.5) / 256.0)
    ground = _pack(BASE[None, :, :] * (1.0 - fw)[:, None, None] + FOG[None, None, :] * fw[:, None, None])
    g = (q + 0.5) / 256.0
    sky = _pack(SKY_TOP[None, :] + (SKY_HOR - SKY_TOP)[None, :] * g[:, None])
    far = _pack(BASE[0] * (1.0 - FOG_MAX) + FOG * FOG_MAX)
    pal = np.zeros((513, 4), np.uint32)
    pal[:256] = ground
    pal[256:512] = sky[:, None]
    pal[512] = far
    return pal


def spec_lens_table(H, W, cell, kx, ky, fov_v_deg=80.0, pitch_deg=10.0, cam_h=1.0, z_far=40.0):
    """float32[H][W][4]: F, L, depth, palette row (uint32 bits) per pixel, binary64 in the spec's operation order."""
    half_h, half_w = H / 2.0, W / 2.0
    f = half_h / math.tan(fov_v_deg * math.pi / 180.0 / 2.0)
    pitch = pitch_deg * math.pi / 180.0
    cp, sp = math.cos(pitch), math.sin(pitch)
    px = (np.arange(W, dtype=np.float64) + 0.5)[None, :] - half_w
    py = half_h - (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    px, py = np.broadcast_to(px, (H, W)), np.broadcast_to(py, (H, W))
    xn, yn = px / f, py / f
    rho2 = (px * px + py * py) / (half_h * half_h)
    xr, yr = xn * (1.0 + kx * rho2), yn * (1.0 + ky * rho2)
    dy, dz = yr * cp - sp, yr * sp + cp
    sky = dy >= -1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        t = cam_h / (-dy)
        zd = t * dz
    far = ~sky & (zd > z_far)
    ground = ~sky & ~far
    g = np.clip((half_h - yr * f) / half_h, 0.0, 1.0)
    row = np.full((H, W), FAR, np.int64)
    row[sky] = SKY0 + np.minimum(np.trunc(g[sky] * 256.0).astype(np.int64), 255)
    row[ground] = np.clip(np.trunc(zd[ground] / z_far * 256.0).astype(np.int64), 0, 255)
    out = np.zeros((H, W, 4), np.float32)
    out[..., 2] = np.float32(z_far)
    out[..., 0][ground] = (zd[ground] / cell).astype(np.float32)
    out[..., 1][ground] = ((t[ground] * xr[ground]) / cell).astype(np.float32)
    out[..., 2][ground] = zd[ground].astype(np.float32)
    out[..., 3] = row.astype(np.uint32).view(np.float32)
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("lens_tables") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "lens_tables_driver.cpp"),
                           os.path.join(ROOT, "triton-racer-sim_amd", "csrc", "trsim_tables.cpp")])
    return str(exe)


def run_driver(driver, oracle_api, tmp_path, track, H, W, kx, ky):
    from triton_racer_sim_amd import _ffi
    cfg = _ffi.TrsConfig()
    oracle_api.default_config(C.byref(cfg))
    cfg.n_envs, cfg.img_h, cfg.img_w = 2, H, W
    (tmp_path / "cfg.bin").write_bytes(bytes(cfg))
    (tmp_path / "pts.bin").write_bytes(np.ascontiguousarray(track_points(track), dtype=np.float64).tobytes())
    out = subprocess.run([driver, str(tmp_path / "cfg.bin"), str(tmp_path / "pts.bin"), repr(float(kx)), repr(float(ky)), str(tmp_path / "t")],
                         capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    cell = float(out.stdout.split()[0])
    lens = np.fromfile(tmp_path / "t.lens", dtype=np.float32).reshape(H, W, 4)
    pal = np.fromfile(tmp_path / "t.lenspal", dtype=np.uint32).reshape(513, 4)
    rowtab = np.fromfile(tmp_path / "t.rowtab", dtype=np.float32).reshape(H, 2)
    return cell, lens, pal, rowtab


@pytest.mark.parametrize("lens", LENSES)
@pytest.mark.parametrize("shape", SIZES)
@pytest.mark.parametrize("track", ["generated", "mountain"])
def test_lens_tables_equal_the_numpy_restatement(driver, oracle_api, tmp_path, track, shape, lens):
    H, W = shape
    kx, ky, _ = lens
    cell, got, pal, _ = run_driver(driver, oracle_api, tmp_path, track, H, W, kx, ky)
    want = spec_lens_table(H, W, cell, kx, ky)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{len(bad)} entries differ, first {bad[:4].tolist()}: got {got[tuple(bad[0][:2])]} want {want[tuple(bad[0][:2])]}"
    assert np.array_equal(pal, spec_lens_palette())


@pytest.mark.parametrize("shape", SIZES)
def test_zero_lens_has_the_flat_rows(driver, oracle_api, tmp_path, shape):
    """kx = ky = 0: every pixel's class (SKY / FAR / GROUND) is its flat row's, and F is the flat row_lz[v] bit for bit."""
    H, W = shape
    cell, got, _, rowtab = run_driver(driver, oracle_api, tmp_path, "generated", H, W, 0.0, 0.0)
    flat_pal = np.fromfile(tmp_path / "t.palette", dtype=np.uint32).reshape(H, 4)
    row = got[..., 3].view(np.uint32)
    cls = np.where(row < 256, 0, np.where(row < 512, 1, 2))               # 0 ground, 1 sky, 2 far
    # the flat table: row_k == 0 exactly on SKY and FAR rows; a FAR row has the far colour (fogged grass), a SKY row a sky colour
    flat_ground = rowtab[:, 1] != 0
    far_rgb = spec_lens_palette()[FAR, 0]
    flat_cls = np.where(flat_ground, 0, np.where(flat_pal[:, 0] == far_rgb, 2, 1))
    assert (flat_cls == 2).any() and (flat_cls == 1).any()
    assert np.array_equal(cls, np.broadcast_to(flat_cls[:, None], (H, W)))
    F = got[..., 0]
    g = flat_ground
    assert np.array_equal(F[g].view(np.uint32), np.broadcast_to(rowtab[g, 0][:, None], (int(g.sum()), W)).view(np.uint32))


def test_stronger_lens_widens_the_horizontal_field(driver, oracle_api, tmp_path):
    H, W = 120, 160
    cell, t0, _, _ = run_driver(driver, oracle_api, tmp_path, "generated", H, W, 0.0, 0.0)
    _, t1, _, _ = run_driver(driver, oracle_api, tmp_path, "generated", H, W, 0.8, 0.0)
    _, t2, _, _ = run_driver(driver, oracle_api, tmp_path, "generated", H, W, 1.6, 0.0)
    v = H - 1                                                              # the bottom row sees the ground at every lens strength here
    for u in (0, W - 1):
        assert t0[v, u, 3].view(np.uint32) < 256 and t1[v, u, 3].view(np.uint32) < 256 and t2[v, u, 3].view(np.uint32) < 256
        assert abs(t0[v, u, 1]) < abs(t1[v, u, 1]) < abs(t2[v, u, 1])


@pytest.mark.parametrize("lens", LENSES)
@pytest.mark.parametrize("shape", SIZES)
def test_mirror_symmetry_is_exact(driver, oracle_api, tmp_path, shape, lens):
    """u and W-1-u: F, depth and palette row bit-identical, L exactly negated on the ground (the kernels store the right half only)."""
    H, W = shape
    _, t, _, _ = run_driver(driver, oracle_api, tmp_path, "generated", H, W, lens[0], lens[1])
    m = t[:, ::-1, :]
    u = t.view(np.uint32)
    mu = m.view(np.uint32)
    for k in (0, 2, 3):
        assert np.array_equal(u[..., k], mu[..., k]), k
    ground = u[..., 3] < 256                                              # (SKY and FAR pixels keep L = +0, which the kernels never use)
    assert np.array_equal(t[..., 1][ground].view(np.uint32), (-m[..., 1])[ground].view(np.uint32))
    assert not t[..., 1][~ground].any()
