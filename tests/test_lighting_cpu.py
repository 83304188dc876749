"""Scene lighting's per-channel rule (include/trsim_spec.h, "scene lighting") on the CPU: the product's function (csrc/trsim_tables.hpp, light_channel
and light_colour — the code the LIGHT kernels light palette entries with), built with AddressSanitizer + UBSan, against an independent numpy binary32
restatement, bit for bit, on every channel value 0..255 — gains 0, negative, huge, +-inf and NaN, biases at +-255 and beyond, the identity."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = [(1.0, 0.0), (0.0, 0.0), (0.0, 17.0), (0.0, -0.5), (0.0, -0.49), (-1.0, 0.0), (-1.0, 255.0), (-0.5, 128.0), (1.0, 255.0), (1.0, -255.0),
         (2.0, -255.0), (1.4, 30.0), (0.6, -30.0), (0.999, 0.0), (1.0001, 0.4999), (1e30, 0.0), (1e30, -1e30), (3.4e38, 3.4e38), (-3.4e38, 255.0),
         (np.inf, 0.0), (-np.inf, 0.0), (np.inf, -np.inf), (np.nan, 0.0), (1.0, np.nan), (1.0, np.inf), (1.0, -np.inf), (1.7, 254.5),
         (1.0, 254.49998), (0.5, 0.0), (1.0 / 3.0, 1.0 / 3.0)]


def spec_light(x, g, b):
    """numpy restatement: t = (float)x * gain; t = t + bias; t = t + 0.5f (each rounded to binary32); !(t > 0) -> 0 (NaN too), t >= 255 -> 255, else (int)t."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float32(x) * np.float32(g)
        t = (t + np.float32(b)).astype(np.float32)
        t = (t + np.float32(0.5)).astype(np.float32)
        out = np.where(~(t > 0), 0, np.where(t >= 255, 255, np.trunc(np.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0))))
    return out.astype(np.uint32)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("light") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "light_driver.cpp")])
    return str(exe)


def run_driver(driver, tmp_path, pairs):
    pairs = np.asarray(pairs, np.float32).reshape(-1, 2)
    (tmp_path / "pairs.bin").write_bytes(pairs.tobytes())
    out = subprocess.run([driver, str(tmp_path / "pairs.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    raw = (tmp_path / "out.bin").read_bytes()
    n = len(pairs)
    ch = np.frombuffer(raw[:n * 256], np.uint8).reshape(n, 256)
    col = np.frombuffer(raw[n * 256:], np.uint32).reshape(n, 256)
    return pairs, ch, col


def test_channel_rule_matches_restatement(driver, tmp_path):
    pairs, ch, col = run_driver(driver, tmp_path, PAIRS)
    x = np.arange(256, dtype=np.uint32)
    for i, (g, b) in enumerate(pairs):
        want = spec_light(x, g, b)
        bad = np.nonzero(ch[i] != want)[0]
        assert bad.size == 0, f"gain {g!r} bias {b!r}: x = {bad[:8]} -> {ch[i][bad[:8]]}, spec {want[bad[:8]]}"
        assert np.array_equal(col[i], want * np.uint32(0x010101)), f"gain {g!r} bias {b!r}: light_colour differs from light_channel per channel"


def test_identity_and_saturation(driver, tmp_path):
    _, ch, _ = run_driver(driver, tmp_path, [(1.0, 0.0), (1.0, 255.0), (1.0, -255.0), (0.0, 0.0), (np.nan, 3.0), (np.inf, 0.0)])
    x = np.arange(256)
    assert np.array_equal(ch[0], x)                    # gain 1, bias 0: the identity, bit for bit
    assert np.all(ch[1] == 255) and np.all(ch[2] == 0)
    assert np.all(ch[3] == 0)                          # 0 * x + 0 + 0.5 -> (int)0.5 = 0
    assert np.all(ch[4] == 0)                          # NaN -> 0
    assert ch[5][0] == 0 and np.all(ch[5][1:] == 255)  # inf * 0 = NaN -> 0; inf -> 255


def test_random_pairs(driver, tmp_path):
    rng = np.random.default_rng(7)
    pairs = np.stack([rng.uniform(-3, 3, 400), rng.uniform(-300, 300, 400)], axis=1)
    pairs, ch, _ = run_driver(driver, tmp_path, pairs)
    x = np.arange(256, dtype=np.uint32)
    for i, (g, b) in enumerate(pairs):
        assert np.array_equal(ch[i], spec_light(x, g, b)), (g, b)
