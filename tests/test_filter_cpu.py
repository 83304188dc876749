"""The host-only owner of the static colour filter (csrc/trsim_filter.hpp) on the CPU, built with AddressSanitizer + UBSan as a stand-alone program:
OpenCV's reciprocal tables against their definition, and the filter of ONE colour — what the rasteriser's palette is filtered with — against the
oracle's ImgPreprocessing.__process of a whole frame, byte for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_image_path import FUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def filter_driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("filter") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "filter_driver.cpp")])
    return str(exe)


def run_filter(filter_driver, *args):
    out = subprocess.run([filter_driver, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return out.stdout


def test_reciprocal_table_is_opencvs(filter_driver):
    """sdiv_table[i] = round((255 << 12) / i), hdiv_table180[i] = round((180 << 12) / (6 i)), entry 0 of both = 0: all 512 entries."""
    got = np.array([int(x) for x in run_filter(filter_driver, "table").split()], dtype=np.int64)
    assert got.shape == (512,)
    i = np.arange(1, 256, dtype=np.float64)
    assert got[0] == 0 and got[256] == 0
    assert np.array_equal(got[1:256], np.rint((255 << 12) / i).astype(np.int64))
    assert np.array_equal(got[257:], np.rint((180 << 12) / (6 * i)).astype(np.int64))


@pytest.fixture(scope="module")
def colour_frame(oracle_api):
    """One 64x64 frame of colours: the generated track's palette, a grey ramp, seeded random colours."""
    from triton_racer_sim_amd.env import BatchedEnv
    env = BatchedEnv(n_envs=1, img_h=64, img_w=64, _api=oracle_api)
    try:
        pal = env.fetch("palette").reshape(-1).astype(np.uint32)
    finally:
        env.close()
    pal = np.stack([pal & 255, (pal >> 8) & 255, (pal >> 16) & 255], -1).astype(np.uint8)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    n = 64 * 64 - len(pal) - len(grey)
    assert len(pal) == 64 * 4 and n > 0
    rnd = np.random.default_rng(14).integers(0, 256, (n, 3), dtype=np.uint8)
    return np.concatenate([pal, grey, rnd]).reshape(1, 64, 64, 3)


@pytest.mark.parametrize("cfg", FUSED)
def test_filter_colour_equals_the_oracle(filter_driver, make_env, colour_frame, tmp_path, cfg):
    """filter_colour of every colour of the frame = the oracle's preprocess_host of the frame (no dynamic brightness, no Canny: the static configurations
    the fused frame filter runs with)."""
    env = make_env("oracle", n_envs=1, track=None, render=False, img_h=64, img_w=64)
    want = env.preprocess_host(colour_frame, cfg)
    (tmp_path / "cfg.bin").write_bytes(bytes(env.pre_config(cfg)))
    (tmp_path / "in.bin").write_bytes(colour_frame.tobytes())
    run_filter(filter_driver, "filter", tmp_path / "cfg.bin", tmp_path / "in.bin", tmp_path / "out.bin")
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(want.shape)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, colour_frame)                          # (the configuration does filter)
