"""Training the speed-as-feature pilot, without a GPU (include/trsim_spec.h, "training the pilot's tail, side branch"): tests/test_train_cpu.py's numpy
restatement extended with the branch fin -> feature1 -> feature2 -> feature3 and dense1's rows behind the flatten, checked against torch.autograd in binary64 on
a small tail (F = 256, n = 9, some fin = 0, some dead ReLUs in every branch layer); the 28-array session's host-only rules of csrc/trsim_train.hpp under a
stand-alone sanitizer driver (tests/train_side_driver.cpp); the bindings and the refusals that need no device.  tests/test_train_side_gpu.py imports the
restatement and compares the kernels with it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_train_cpu as R
from conftest import ROOT
from triton_racer_sim_amd import _ffi

f32 = np.float32
SIDE = ("f1w", "f1b", "f2w", "f2b", "f3w", "f3b")          # kernel and bias of feature1 (1 -> 4), feature2 (4 -> 8), feature3 (8 -> 16)
NAMES = R.NAMES + SIDE                                     # the 14 trained arrays in the order of trs_pilot_train_begin_ex; w1 is [F + 16][100]
WIDTHS = (1, 4, 8, 16)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def branch(fin, P, dtype=np.float64):
    """(y1, y2, y3): the branch's activations behind their ReLUs from fin [n] (speed / 20 as the loader delivers it)"""
    y = np.asarray(fin, dtype).reshape(-1, 1)
    out = []
    for l in (1, 2, 3):
        y = np.maximum(y @ P[f"f{l}w"].astype(dtype) + P[f"f{l}b"].astype(dtype), 0)
        out.append(y)
    return out


def forward(zf, fin, P, dtype=np.float64):
    """zf [n][100]: dense1's sum over the flatten with its bias (the slabs).  Returns y1 .. y3, z1 = zf + y3 W1Y, and z2, z3, out behind it."""
    y1, y2, y3 = branch(fin, P, dtype)
    z1 = np.asarray(zf, dtype) + y3 @ P["w1"][-16:].astype(dtype)
    z2, z3, out = R.forward(z1, P, dtype)
    return {"y1": y1, "y2": y2, "y3": y3, "z1": z1, "z2": z2, "z3": z3, "out": out}


def backward(f, y, P, dtype=np.float64):
    """loss, delta1 .. delta4 as the tail's, then the branch: delta-y3 = [y3 > 0] . (delta1 W1Y^T), delta-y2 and delta-y1 through feature3 and feature2"""
    loss, d1, d2, d3, d4 = R.backward(f["z1"], f["z2"], f["z3"], f["out"], y, P, dtype)
    dy3 = (d1 @ P["w1"][-16:].astype(dtype).T) * (f["y3"] > 0)
    dy2 = (dy3 @ P["f3w"].astype(dtype).T) * (f["y2"] > 0)
    dy1 = (dy2 @ P["f2w"].astype(dtype).T) * (f["y1"] > 0)
    return {"loss": loss, "d1": d1, "d2": d2, "d3": d3, "d4": d4, "dy1": dy1, "dy2": dy2, "dy3": dy3}


def small_gradients(fin, f, b, dtype=np.float64):
    """the tail's small gradients, gW1Y (rows F .. F + 15 of dense1's kernel) and the branch's six"""
    g = R.small_gradients(f["z1"], f["z2"], f["z3"], b["d1"], b["d2"], b["d3"], b["d4"], dtype)
    g["w1y"] = np.asarray(f["y3"], dtype).T @ np.asarray(b["d1"], dtype)
    ins = (np.asarray(fin, dtype).reshape(-1, 1), f["y1"], f["y2"])
    for l, a in zip((1, 2, 3), ins):
        d = np.asarray(b[f"dy{l}"], dtype)
        g[f"f{l}w"] = np.asarray(a, dtype).T @ d
        g[f"f{l}b"] = d.sum(0)
    return g


def side_layout(F):
    sizes = [(F + 16) * 100, 100, 5000, 50, 1250, 25, 50, 2, 4, 4, 32, 8, 128, 16]
    return [sum(sizes[:a]) for a in range(15)]


def small_side_tail(F, seed):
    """A tail of 14 arrays: branch biases of both signs, so that every branch layer has dead and live units over a range of features"""
    rng = np.random.default_rng(seed)
    P = R.small_tail(F + 16, seed)
    for l in (1, 2, 3):
        P[f"f{l}w"] = R.glorot(rng, WIDTHS[l - 1], WIDTHS[l])
        P[f"f{l}b"] = rng.uniform(-0.3, 0.3, WIDTHS[l]).astype(f32)
    return P


# ---- the restatement against autograd ----------------------------------------------------------------------------------------------------
def test_restatement_matches_autograd_float64():
    import torch
    F, n = 256, 9
    rng = np.random.default_rng(5)
    P = small_side_tail(F, 6)
    x7 = np.maximum(rng.normal(0.0, 1.0, (n, F)), 0).astype(np.float16).astype(np.float64)
    fin = np.array([0.0, 0.0, -0.4, 0.05, 0.3, 0.55, 0.8, 1.0, 2.5])
    y = rng.uniform(-1, 1, (n, 2))
    T = {k: torch.tensor(P[k].astype(np.float64), requires_grad=True) for k in NAMES}
    s = torch.tensor(fin).reshape(-1, 1)
    for l in (1, 2, 3):
        s = torch.relu(s @ T[f"f{l}w"] + T[f"f{l}b"])
    z1t = torch.cat([torch.tensor(x7), s], 1) @ T["w1"] + T["b1"]                  # the concatenation behind the flatten, in front of dense1
    out_t = torch.relu(torch.relu(torch.relu(z1t) @ T["w2"] + T["b2"]) @ T["w3"] + T["b3"]) @ T["w4"] + T["b4"]
    loss_t = ((out_t - torch.tensor(y)) ** 2).sum() / (2 * n)
    loss_t.backward()
    zf = x7 @ P["w1"][:F].astype(np.float64) + P["b1"].astype(np.float64)
    f = forward(zf, fin, P)
    b = backward(f, y, P)
    g = small_gradients(fin, f, b)
    g["w1"] = np.concatenate([x7.T @ b["d1"], g["w1y"]])
    assert abs(b["loss"] - float(loss_t.detach())) < 1e-13
    for l in (1, 2, 3):                                                            # dead and live units in every branch layer, and frames whose feature is 0
        alive = f[f"y{l}"] > 0
        assert (alive.any(0) & ~alive.all(0)).any(), l
    assert (fin == 0).sum() == 2 and np.abs(g["f1w"]).max() > 0
    for k in NAMES:
        np.testing.assert_allclose(g[k], T[k].grad.numpy(), rtol=1e-11, atol=1e-14, err_msg=k)


# ---- the host-only rules under a sanitizer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def side_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train_side") / "train_side_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", ROOT, os.path.join(ROOT, "tests", "train_side_driver.cpp"), "-o", exe])
    return exe


def test_driver_layout(side_driver):
    for F in (128, 4608, 16640, 70528):
        got = [int(x) for x in R.run_driver(side_driver, "layout", F)]
        want = side_layout(F)
        assert got[:15] == want
        assert got[15] == F * 100                                                  # W1Y: rows F .. F + 15 of array 0
        assert got[16:] == want[:9]                                                # what the 22-array kernels are given: array 0 whole, then 1 .. 7
        assert want[14] - want[8] + 1600 == 1792                                   # the values the side kernels own


def test_driver_debug_sizes(side_driver):
    got = [int(x) for x in R.run_driver(side_driver, "debug", 37)]
    arrays = [1600, 4, 4, 32, 8, 128, 16]
    want = [37, 148, 296, 592, 148, 296, 592, 0] + (arrays + [0]) * 3 + [0, 0]
    assert got[:34] == want
    assert got[34] == 1 + 4 + 8 + 16 + 4 + 8 + 16 + 4 and got[35] == 1792
    assert [v[1] for v in _ffi.TRAIN_SIDE_ARRAYS.values()] == arrays and [v[0] for v in _ffi.TRAIN_SIDE_ARRAYS.values()] == list(range(7))
    assert {k: v[0] for k, v in _ffi.TRAIN_SIDE_DEBUG.items()} == {"fin": 0, "y1": 1, "y2": 2, "y3": 3, "dy1": 4, "dy2": 5, "dy3": 6, "g": 8, "m": 16, "v": 24}


def test_driver_config_and_count_refusals(side_driver):
    assert R.run_driver(side_driver, "config") == ["ok"]
    out = R.run_driver(side_driver, "count")
    got = {(int(out[i]), int(out[i + 1])): out[i + 2] for i in range(0, len(out), 3)}
    for pilot in (22, 28, 42):
        for n in (8, 14, 0, 7, 22, 28):
            want = "limit" if pilot == 42 else "ok" if (pilot, n) in ((22, 8), (28, 14)) else "arg"
            assert got[(pilot, n)] == want, (pilot, n)


# ---- the library without a device ----------------------------------------------------------------------------------------------------------
def test_ffi_binds_the_side_symbols(hip_api):
    assert _ffi.TRAIN_SIDE_SYMBOLS == ["pilot_train_begin_ex", "pilot_train_step_ex", "pilot_train_get_ex", "pilot_train_debug_side"]
    assert set(_ffi.TRAIN_SIDE_SYMBOLS) <= set(_ffi.PILOT_SYMBOLS) and not set(_ffi.TRAIN_SIDE_SYMBOLS) & set(_ffi.SYMBOLS)
    assert hip_api.has_train_side and all(callable(getattr(hip_api, s)) for s in _ffi.TRAIN_SIDE_SYMBOLS)
    assert _ffi.TRAIN_SIDE_LAYERS[:4] == _ffi.TRAIN_LAYERS and _ffi.TRAIN_SIDE_LAYERS[4:] == ("feature1", "feature2", "feature3")


def test_refusals_without_a_device(hip_api):
    w1 = np.zeros((128 + 16, 100), f32)
    arrs = (C.c_void_p * 14)(w1.ctypes.data, *([None] * 13))

    def refused(rc, code, text):
        assert rc == code, (rc, hip_api.last_error())
        assert text in (hip_api.last_error() or b"").decode(), hip_api.last_error()

    def cfg(**kw):
        c = _ffi.TrsTrainConfig()
        hip_api.default_train_config(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    for n in (0, 7, 22, 28, -1):
        refused(hip_api.pilot_train_begin_ex(None, None, arrs, n), -1, "n_arrays")
    for kw, n, text in (({"train_mask": 0x80}, 14, "train_mask"), ({"train_mask": 0}, 14, "train_mask"), ({"train_mask": 0x10}, 8, "train_mask"),
                        ({"train_mask": 0x7F}, 8, "train_mask"), ({"train_mask": 0x20, "lr": 0.0}, 14, "lr"), ({"struct_size": 8}, 14, "struct_size"),
                        ({"beta2": 1.0}, 14, "beta2")):
        refused(hip_api.pilot_train_begin_ex(None, C.byref(cfg(**kw)), arrs, n), -1, text)
    refused(hip_api.pilot_train_begin_ex(None, None, None, 14), -1, "dense1's kernel")
    refused(hip_api.pilot_train_begin_ex(None, None, (C.c_void_p * 14)(), 14), -1, "dense1's kernel")
    for c, n in ((None, 14), (None, 8), (cfg(train_mask=0x20), 14), (cfg(train_mask=0x7F), 14), (cfg(), 14)):
        refused(hip_api.pilot_train_begin_ex(None, None if c is None else C.byref(c), arrs, n), -1, "null handle")
    refused(hip_api.pilot_train_step_ex(None, None, None, None, 1, None), -1, "null handle")
    refused(hip_api.pilot_train_get_ex(None, None, 7, None), -1, "n_arrays")
    refused(hip_api.pilot_train_get_ex(None, None, 14, None), -1, "null handle")
    refused(hip_api.pilot_train_debug_side(None, 0, None, 0), -1, "null handle")
