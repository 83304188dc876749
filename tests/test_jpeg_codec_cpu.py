"""The camera codec ("camera codec (JPEG round trip)", include/trsim_spec.h) restated in numpy from the spec text — the quantised coefficients of
tests/test_jpeg_cpu.py handed straight to the dequantiser, inverse transform, upsampling and colour of tests/test_jpeg_decode_cpu.py — and pinned three
ways: against decode(encode()) of those two restatements, against Pillow's save and open byte for byte (where Pillow imports), and against what the
shared header csrc/trsim_jpeg_codec.hpp computes on the host (tests/jpeg_codec_driver.cpp, built with the address and undefined-behaviour sanitizers).
tests/test_jpeg_codec_gpu.py takes its reference from here."""
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_jpeg_cpu import QUALITIES, ZZ, coefficients, encode, frame, quant_tables
from test_jpeg_decode_cpu import DECODED, decode, samples, upsample

SIZES = [(8, 8), (8, 12), (24, 40), (50, 100), (60, 80), (120, 160), (240, 320)]
KINDS = ["noise", "ramp", "flat0", "flat255", "checker"]                # the kinds of test_jpeg_cpu.frame()
assert QUALITIES == [75, 50, 95, 100, 10]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def roundtrip(img, quality=75):
    """codec(frame, quality) of one uint8[H][W][3] frame: no file, no entropy stage"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    assert w > 4 and 1 <= quality <= 100
    mh, mw = -(-h // 16), -(-w // 16)
    z = coefficients(img, quality).reshape(mh, mw, 6, 64)              # quantised, zig-zag order (dummy Y blocks filled in: they lie beyond [:h, :w])
    ql, qc = ([t[ZZ[k]] for k in range(64)] for t in quant_tables(quality))     # the entries the coefficients were quantised with, zig-zag order
    y = samples(z[:, :, :4], ql).reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(16 * mh, 16 * mw)[:h, :w]
    cb, cr = (upsample(samples(z[:, :, 4 + c], qc).transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw), h, w) - 128 for c in range(2))
    fix = lambda x: int(x * 65536 + 0.5)
    r = y + ((fix(1.402) * cr + 32768) >> 16)
    g = y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    b = y + ((fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pillow_roundtrip(img, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())))


# ---- 1. against the two restatements it is composed from ----------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_restatement_equals_decode_of_encode(h, w):
    for q in QUALITIES:
        for kind in KINDS:
            img = frame(kind, h, w)
            want, status, _ = decode(encode(img, q), h, w)
            assert status == DECODED
            assert np.array_equal(roundtrip(img, q), want), (kind, h, w, q)


# ---- 2. against Pillow ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_restatement_equals_pillow_save_and_open(h, w):
    pytest.importorskip("PIL")
    for q in QUALITIES:
        for kind in KINDS:
            img = frame(kind, h, w)
            assert np.array_equal(roundtrip(img, q), pillow_roundtrip(img, q)), (kind, h, w, q)


def test_the_codec_is_lossy_where_the_frames_are_hard():
    """what the feature is for: flat colours with hard edges come back changed, and a flat frame comes back as it was"""
    img = frame("checker", 24, 40)
    assert not np.array_equal(roundtrip(img, 75), img)
    assert np.array_equal(roundtrip(frame("flat255", 24, 40), 75), frame("flat255", 24, 40))


# ---- 3. against the shared header, on the host and under the sanitizers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec_driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("jpeg_codec") / "jpeg_codec_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "jpeg_codec_driver.cpp")])
    return str(exe)


def run_driver(exe, *args, expect=0):
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=120)
    assert out.returncode == expect, out.stderr[-2000:]
    return out.stdout.splitlines()


def test_host_function_equals_the_restatement(codec_driver, tmp_path):
    """codec_frame — colour, edges, the block round trip, upsampling and colour back, all from the functions the kernel calls — on frames held in heap
    buffers of exactly their size; every content and every quality at every size"""
    path = tmp_path / "frame.rgb"
    for i, (h, w) in enumerate(SIZES + [(9, 8), (17, 33)]):
        for k, kind in enumerate(KINDS):
            q = QUALITIES[(i + k) % len(QUALITIES)]
            img = frame(kind, h, w)
            path.write_bytes(img.tobytes())
            (row,) = run_driver(codec_driver, "frame", h, w, q, path)
            got = np.frombuffer(bytes.fromhex(row), np.uint8).reshape(h, w, 3)
            assert np.array_equal(got, roundtrip(img, q)), (kind, h, w, q)
        img = frame("noise", h, w, seed=1)
        path.write_bytes(img.tobytes())
        for q in QUALITIES:
            (row,) = run_driver(codec_driver, "frame", h, w, q, path)
            assert bytes.fromhex(row) == roundtrip(img, q).tobytes(), ("noise", h, w, q)
    path.write_bytes(frame("noise", 8, 4).tobytes())
    assert run_driver(codec_driver, "frame", 8, 4, 75, path, expect=3) == []          # a chroma plane two samples wide: refused, as the decoder refuses it


def test_the_kernels_lds_plan(codec_driver):
    """both BASELINE sizes fit a workgroup's 160 KiB many times over, the regions do not overlap, and the width limit is the one include/trsim.h states"""
    for w in (8, 160, 320, 1200):
        first, limit = run_driver(codec_driver, "plan", w)
        off = [int(v) for v in first.split()]
        mw = -(-w // 16)
        sizes = [512, 16 * w * 3, 256 * mw, 128 * mw, 4 * 8 * 72 * 4, 2 * 256 * mw, 3 * 128 * mw]
        assert all(o % 16 == 0 for o in off)
        for k in range(7):
            assert off[k + 1] - off[k] >= sizes[k], (w, k)
        assert off[7] <= 160 * 1024
        assert int(limit) == 1200
    assert int(run_driver(codec_driver, "plan", 1216)[0].split()[7]) > 160 * 1024
    assert int(run_driver(codec_driver, "plan", 160)[0].split()[7]) <= 32 * 1024 and int(run_driver(codec_driver, "plan", 320)[0].split()[7]) <= 64 * 1024
