"""Training the pilot's tail, without a GPU (include/trsim_spec.h, "training the pilot's tail"): a numpy restatement of the loss, the backward pass through
the small layers, the small gradients, the power-of-two quantisation of delta1, dense1's weight gradient and Adam in Keras's form; the spec's vectors; the
host-only rules of csrc/trsim_train.hpp under a stand-alone sanitizer driver (tests/train_driver.cpp); the library's defaults and the refusals that need no
device; and the restatement's gradients against torch.autograd in binary64 on a small tail (F = 256, n = 5).  tests/test_train_gpu.py imports the
restatement and compares the kernels with it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from triton_racer_sim_amd import _ffi

f32 = np.float32
SIZES = (100, 50, 25, 2)                                    # outputs of dense1, dense2, dense3, output_layer
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")    # the eight trained arrays in the order of trs_pilot_train_begin


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def scale_exponent(bits):
    """s of a batch from the largest bit pattern of |delta1|: E = floor(log2(max)), s = 14 - E clamped to [-100, 100]; 0 for an all-zero batch"""
    a = int(bits) & 0x7FFFFFFF
    if a == 0:
        return 0
    E = (a.bit_length() - 1) - 149 if (a >> 23) == 0 else (a >> 23) - 127
    return max(-100, min(100, 14 - E))


def max_abs_bits(d1):
    return int((np.ascontiguousarray(d1, f32).view(np.uint32) & np.uint32(0x7FFFFFFF)).max())


def quantise(d1, s):
    """q = binary16_rn(delta1 * 2^s): the scaling is exact in binary32, one rounding to nearest even"""
    with np.errstate(over="ignore"):
        return (np.asarray(d1, f32) * f32(2.0 ** s)).astype(np.float16)


def alpha_t(lr, beta1, beta2, t):
    """lr sqrt(1 - beta2^t) / (1 - beta1^t) in binary64 from the config's binary32 values, rounded once"""
    b1, b2 = float(f32(beta1)), float(f32(beta2))
    return f32(float(f32(lr)) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def adam(g, m, v, w, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
    """One update in binary32, every operation rounded by itself: m = b1 m + c1 g; v = b2 v + c2 (g g); w = w - (alpha_t m) / (sqrt(v) + eps), with
    c = (float)(1 - (double)beta).  Returns (m, v, w)."""
    g, m, v, w = (np.asarray(a, f32) for a in (g, m, v, w))
    b1, b2, e = f32(beta1), f32(beta2), f32(eps)
    c1, c2 = f32(1.0 - float(b1)), f32(1.0 - float(b2))
    a = alpha_t(lr, beta1, beta2, t)
    m = (b1 * m).astype(f32) + (c1 * g).astype(f32)
    v = (b2 * v).astype(f32) + (c2 * (g * g).astype(f32)).astype(f32)
    w = w - ((a * m).astype(f32) / (np.sqrt(v).astype(f32) + e).astype(f32)).astype(f32)
    return m.astype(f32), v.astype(f32), w.astype(f32)


def forward(z1, P, dtype=np.float64):
    """(z2, z3, out) behind dense1's pre-activation z1 [n][100]; P: dict of the small layers' arrays"""
    z1 = np.asarray(z1, dtype)
    a1 = np.maximum(z1, 0)
    z2 = a1 @ P["w2"].astype(dtype) + P["b2"].astype(dtype)
    z3 = np.maximum(z2, 0) @ P["w3"].astype(dtype) + P["b3"].astype(dtype)
    out = np.maximum(z3, 0) @ P["w4"].astype(dtype) + P["b4"].astype(dtype)
    return z2, z3, out


def backward(z1, z2, z3, out, y, P, dtype=np.float64):
    """loss and (delta1 .. delta4) of steps 2 and 3: the masks come from the pre-activations given"""
    n = len(out)
    e = np.asarray(out, dtype) - np.asarray(y, dtype)
    loss = (e * e).sum() / (2 * n)
    d4 = e / n
    d3 = (d4 @ P["w4"].astype(dtype).T) * (np.asarray(z3) > 0)
    d2 = (d3 @ P["w3"].astype(dtype).T) * (np.asarray(z2) > 0)
    d1 = (d2 @ P["w2"].astype(dtype).T) * (np.asarray(z1) > 0)
    return loss, d1, d2, d3, d4


def small_gradients(z1, z2, z3, d1, d2, d3, d4, dtype=np.float64):
    """gW2, gW3, gW4 and the four bias gradients of step 4"""
    a = [np.maximum(np.asarray(z, dtype), 0) for z in (z1, z2, z3)]
    d = [np.asarray(x, dtype) for x in (d1, d2, d3, d4)]
    g = {"b1": d[0].sum(0)}
    for l in (2, 3, 4):
        g[f"w{l}"] = a[l - 2].T @ d[l - 1]
        g[f"b{l}"] = d[l - 1].sum(0)
    return g


def gw1_reference(x7h, d1):
    """(gW1 float64[F][100], tolerance float64[F][100], s): the binary64 sum of the products of the binary16 activation with the quantised delta1, scaled
    back; the tolerance is (n + 1) 2^-24 sum_i |x7 q| 2^-s per element"""
    s = scale_exponent(max_abs_bits(d1))
    q = quantise(d1, s).astype(np.float64)
    x = np.asarray(x7h, np.float64)
    back = 2.0 ** -s
    return (x.T @ q) * back, (len(x) + 1) * 2.0 ** -24 * (np.abs(x).T @ np.abs(q)) * back, s


def glorot(rng, fan_in, fan_out):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, (fan_in, fan_out)).astype(f32)


def small_tail(F, seed):
    rng = np.random.default_rng(seed)
    P, fan_in = {}, F
    for l, out in enumerate(SIZES, 1):
        P[f"w{l}"] = glorot(rng, fan_in, out)
        P[f"b{l}"] = rng.uniform(-0.1, 0.1, out).astype(f32)
        fan_in = out
    return P


# ---- vectors of the spec -----------------------------------------------------------------------------------------------------------------
def bits_of(x):
    return int(np.asarray(x, f32).view(np.uint32))


def test_exponent_rule_vectors():
    assert scale_exponent(0) == 0 and scale_exponent(0x80000000) == 0             # all zero (and -0)
    assert scale_exponent(bits_of(1.0)) == 14 and scale_exponent(bits_of(1.9999999)) == 14 and scale_exponent(bits_of(2.0)) == 13
    assert scale_exponent(bits_of(0.5)) == 15 and scale_exponent(bits_of(-3e-6)) == 14 + 19     # 3e-6 in [2^-19, 2^-18)
    assert scale_exponent(bits_of(2.0 ** 14)) == 0 and scale_exponent(bits_of(2.0 ** 15)) == -1
    assert scale_exponent(bits_of(2.0 ** -86)) == 100 and scale_exponent(bits_of(2.0 ** -87)) == 100    # the clamp from above
    assert scale_exponent(1) == 100 and scale_exponent(0x007FFFFF) == 100 and scale_exponent(0x00400000) == 100   # subnormals: E = -149, -127, -127
    assert scale_exponent(bits_of(2.0 ** 114)) == -100 and scale_exponent(bits_of(2.0 ** 120)) == -100   # the clamp from below
    assert scale_exponent(0x7F800000) == -100 and scale_exponent(0x7FC00000) == -100                     # Inf and NaN patterns: E = 128
    for x in (1.0, 1.5, 3e-6, 123.0, 2.0 ** -20):                                 # the largest value lands in [2^14, 2^15)
        qmax = float(quantise(np.array([x], f32), scale_exponent(bits_of(x)))[0])
        assert 2.0 ** 14 <= qmax < 2.0 ** 15


def test_quantisation_is_exact_scaling_then_one_rounding():
    d = np.array([1.0, -0.75, 2.0 ** -11 * 1.0001, 3.0e-5, -2.0 ** -15, 0.0, 2.0 ** -40], f32)
    s = scale_exponent(max_abs_bits(d))
    assert s == 14
    q = quantise(d, s)
    assert q[0] == 16384 and q[1] == -12288 and q[5] == 0
    assert q[2] == np.float16(8.0) and float(q[4]) == -0.5                         # 8.0008 rounds to 8 (spacing 2^-7 there); -0.5 is exact
    assert float(q[6]) == 2.0 ** -24 * round(2.0 ** -26 * 2.0 ** 24) == 0.0           # below half the smallest subnormal: zero


def test_alpha_vectors():
    assert bits_of(alpha_t(1e-3, 0.9, 0.999, 1)) == 0x39A5CB17
    assert bits_of(alpha_t(1e-3, 0.9, 0.999, 2)) == 0x3976BEEF
    assert bits_of(alpha_t(1e-3, 0.9, 0.999, 1000)) == 0x3A507326
    assert abs(float(alpha_t(1e-3, 0.9, 0.999, 1)) - 1e-3 * math.sqrt(1 - 0.999) / (1 - 0.9)) < 3e-9    # 0.999f is 1.3e-8 above 0.999: 6.4e-6 relative in the root


def test_adam_hand_checked_update():
    """g = 1, m = v = 0, w = 1 at t = 1: m = c1 = (float)(1 - 0.9f), v = c2 = (float)(1 - 0.999f), and the step is alpha_1 c1 / (sqrt(c2) + eps)."""
    m, v, w = adam(f32(1.0), f32(0.0), f32(0.0), f32(1.0), 1)
    assert bits_of(m) == 0x3DCCCCD0 and bits_of(v) == 0x3A831200 and bits_of(w) == 0x3F7FBE77
    assert abs(float(w) - (1.0 - 1e-3)) < 2e-7                                      # Adam's first step is lr in size
    m0, v0, w0 = adam(f32(0.0), f32(0.0), f32(0.0), f32(0.3), 7)                   # a zero gradient on fresh moments keeps every bit
    assert bits_of(m0) == 0 and bits_of(v0) == 0 and bits_of(w0) == bits_of(0.3)


# ---- the restatement against autograd ----------------------------------------------------------------------------------------------------
def test_restatement_matches_autograd_float64():
    import torch
    F, n = 256, 5
    rng = np.random.default_rng(3)
    P = small_tail(F, 4)
    x7 = np.maximum(rng.normal(0.0, 1.0, (n, F)), 0).astype(np.float16).astype(np.float64)
    y = rng.uniform(-1, 1, (n, 2))
    T = {k: torch.tensor(P[k].astype(np.float64), requires_grad=True) for k in NAMES}
    h = torch.tensor(x7)
    z1t = h @ T["w1"] + T["b1"]
    out_t = torch.relu(torch.relu(torch.relu(z1t) @ T["w2"] + T["b2"]) @ T["w3"] + T["b3"]) @ T["w4"] + T["b4"]
    loss_t = ((out_t - torch.tensor(y)) ** 2).sum() / (2 * n)                      # Keras's 'mse' over [n][2]
    loss_t.backward()
    z1 = x7 @ P["w1"].astype(np.float64) + P["b1"].astype(np.float64)
    z2, z3, out = forward(z1, P)
    loss, d1, d2, d3, d4 = backward(z1, z2, z3, out, y, P)
    g = small_gradients(z1, z2, z3, d1, d2, d3, d4)
    g["w1"] = x7.T @ d1
    assert abs(loss - float(loss_t.detach())) < 1e-13
    assert 0.2 < (z1 > 0).mean() < 0.8
    for k in NAMES:
        np.testing.assert_allclose(g[k], T[k].grad.numpy(), rtol=1e-11, atol=1e-14, err_msg=k)
    # the quantised gradient of dense1 is the exact one to binary16's precision: 2^-11 relative per product, measured on the absolute sum
    ref, _, s = gw1_reference(x7, d1.astype(f32))
    bound = 2.0 ** -11 * (np.abs(x7).T @ np.abs(d1)) + 2.0 ** -24 * 2.0 ** -s * np.abs(x7).sum(0)[:, None]
    assert (np.abs(ref - g["w1"]) <= bound * 1.001 + 1e-30).all()


# ---- the host-only rules under a sanitizer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train") / "train_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", ROOT, os.path.join(ROOT, "tests", "train_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.split()


def test_driver_exponent_rule(driver):
    pats = [0, 0x80000000, 1, 0x00400000, 0x007FFFFF, 0x00800000, 0x7F800000, 0x7FC00000] + [bits_of(x) for x in
            (1.0, 1.9999999, 2.0, 0.5, -3e-6, 2.0 ** 14, 2.0 ** 15, 2.0 ** -86, 2.0 ** -87, 2.0 ** 114, 2.0 ** 120, 6.1e-5, 65504.0)]
    rng = np.random.default_rng(0)
    pats += [int(p) for p in rng.integers(0, 2 ** 32, 200, dtype=np.uint64)]
    got = [int(x) for x in run_driver(driver, "exp", *pats)]
    assert got == [scale_exponent(p) for p in pats]


def test_driver_alpha_and_constants(driver):
    out = run_driver(driver, "alpha", 1, 2, 3, 1000, 100000)
    assert [int(x, 16) for x in out[:5]] == [bits_of(alpha_t(1e-3, 0.9, 0.999, t)) for t in (1, 2, 3, 1000, 100000)]
    assert [int(x, 16) for x in out[5:7]] == [0x3DCCCCD0, 0x3A831200]             # 1 - beta1, 1 - beta2
    assert [int(x, 16) for x in run_driver(driver, "pow2", -100, -1, 0, 14, 100)] == [bits_of(2.0 ** e) for e in (-100, -1, 0, 14, 100)]


def test_driver_layout(driver):
    for F in (256, 4608, 16640, 70528):
        off = [int(x) for x in run_driver(driver, "layout", F)]
        sizes = [F * 100, 100, 5000, 50, 1250, 25, 50, 2]
        assert off == [sum(sizes[:a]) for a in range(9)]
    got = [int(x) for x in run_driver(driver, "debug", 37, 4608)]
    want = [74, 3700, 1850, 925, 3700, 1850, 925, 74, 460800, 5000, 1250, 50, 100, 50, 25, 2] + [460800, 100, 5000, 50, 1250, 25, 50, 2] * 2 + [1, 1, 460800, 0, 0]
    assert got == want                                                             # items 0 .. 34, then two unknown ones (35, -1)


def test_driver_config_refusals(driver):
    out = run_driver(driver, "config")
    assert out == ["ok"], out


# ---- the library without a device ----------------------------------------------------------------------------------------------------------
def test_ffi_binds_the_training_symbols():
    assert set(_ffi.TRAIN_SYMBOLS) <= set(_ffi.PILOT_SYMBOLS)
    assert _ffi.TRAIN_SYMBOLS == ["default_train_config", "pilot_train_begin", "pilot_train_step", "pilot_train_get", "pilot_train_debug", "pilot_train_end"]


def test_defaults_and_struct_size(hip_api):
    cfg = _ffi.TrsTrainConfig()
    hip_api.default_train_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_ffi.TrsTrainConfig) == 24
    assert (bits_of(cfg.lr), bits_of(cfg.beta1), bits_of(cfg.beta2), bits_of(cfg.eps)) == (bits_of(1e-3), bits_of(0.9), bits_of(0.999), bits_of(1e-7))
    assert cfg.train_mask == 0xF                                                   # the last field reads back: no padding drift
    hip_api.default_train_config(None)                                             # NULL is ignored


def test_refusals_without_a_device(hip_api):
    w1 = np.zeros((128, 100), f32)
    arrs = (C.c_void_p * 8)(w1.ctypes.data, *([None] * 7))

    def refused(rc, code, text):
        assert rc == code, (rc, hip_api.last_error())
        assert text in (hip_api.last_error() or b"").decode()

    def cfg(**kw):
        c = _ffi.TrsTrainConfig()
        hip_api.default_train_config(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    for kw, text in (({"struct_size": 8}, "struct_size"), ({"lr": 0.0}, "lr"), ({"lr": float("nan")}, "lr"), ({"lr": float("inf")}, "lr"),
                     ({"beta1": 1.0}, "beta1"), ({"beta1": -0.1}, "beta1"), ({"beta2": 1.0}, "beta2"), ({"beta2": float("nan")}, "beta2"),
                     ({"eps": 0.0}, "eps"), ({"eps": -1e-7}, "eps"), ({"train_mask": 0}, "train_mask"), ({"train_mask": 0x10}, "train_mask")):
        refused(hip_api.pilot_train_begin(None, C.byref(cfg(**kw)), arrs), -1, text)
    refused(hip_api.pilot_train_begin(None, None, None), -1, "dense1's kernel")
    refused(hip_api.pilot_train_begin(None, None, (C.c_void_p * 8)()), -1, "dense1's kernel")
    refused(hip_api.pilot_train_begin(None, None, arrs), -1, "null handle")
    refused(hip_api.pilot_train_begin(None, C.byref(cfg()), arrs), -1, "null handle")
    refused(hip_api.pilot_train_step(None, None, None, 1, None), -1, "null handle")
    refused(hip_api.pilot_train_get(None, None, None), -1, "null handle")
    refused(hip_api.pilot_train_debug(None, 0, None, 0), -1, "null handle")
    refused(hip_api.pilot_train_end(None), -1, "null handle")
