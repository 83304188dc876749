"""Training the pilot's last convolutions, without a GPU (include/trsim_spec.h, "training the pilot's last convolutions"): a numpy restatement of rules 2-5
(the gradient at conv7's output, the per-layer power-of-two scale, the data gradient, the weight and bias gradients), checked against torch.autograd in
binary64 at three small shapes; the sensitivity of that reference to the mistakes a kernel of this kind makes (a shifted tap, a dropped frame, a dropped last
k-step, a dropped 64-channel half of conv7's input), each at least ten times the derived bound; and the host-only rules of csrc/trsim_train_conv.hpp under a
stand-alone sanitizer driver (tests/train_conv_driver.cpp): the mask check, the master layout, the packed index against pack_layer, the reduction split.
tests/test_train_conv_gpu.py imports the restatement and compares the kernels with it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_train_cpu as R
from conftest import ROOT
from triton_racer_sim_amd import _ffi

f32, U = np.float32, 2.0 ** -24
CHANNELS = ((64, 64), (64, 64), (64, 128), (128, 128))       # (CIN, COUT) of conv4 .. conv7
CHUNK = 64


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def g7(x7h, w1h, q1, s):
    """Rule 2: G7 [n][F] = [x7 > 0] . 2^-s sum_o W1h[k][o] q1[o], in binary64 from the binary16 values"""
    return (np.asarray(x7h) > 0) * (np.asarray(q1, np.float64) @ np.asarray(w1h, np.float64).T) * 2.0 ** -s


def g7_abs(w1h, q1, s):
    return (np.abs(np.asarray(q1, np.float64)) @ np.abs(np.asarray(w1h, np.float64)).T) * 2.0 ** -s


def scale_of(G):
    """Rule 3: the exponent of a layer's scale from the binary32 gradient, by the tail's rule"""
    return R.scale_exponent(R.max_abs_bits(np.asarray(G, f32)))


def dgrad(q, wh, xin, s, taps=None):
    """Rule 4: G(l-1) [n][IH][IW][CIN] from q(l) [n][OH][OW][COUT] under 2^s, W(l)h [3][3][CIN][COUT] and x(l-1); taps: the (kh, kw) that take part"""
    q, wh = np.asarray(q, np.float64), np.asarray(wh, np.float64)
    n, OH, OW, _ = q.shape
    G = np.zeros(np.shape(xin), np.float64)
    for kh, kw in (taps or [(a, b) for a in range(3) for b in range(3)]):
        G[:, kh:kh + OH, kw:kw + OW, :] += q @ wh[kh, kw].T
    return G * (np.asarray(xin) > 0) * 2.0 ** -s


def dgrad_abs(q, wh, xin, s):
    return dgrad(np.abs(np.asarray(q, np.float64)), np.abs(np.asarray(wh, np.float64)), np.ones(np.shape(xin)), s)


def wgrad(xin, q, s):
    """Rule 5: (gW [3][3][CIN][COUT], gb [COUT]) from x(l-1) and q(l) under 2^s"""
    x, q = np.asarray(xin, np.float64), np.asarray(q, np.float64)
    n, OH, OW, _ = q.shape
    gw = np.stack([np.stack([np.einsum("nyxc,nyxo->co", x[:, kh:kh + OH, kw:kw + OW], q) for kw in range(3)]) for kh in range(3)])
    return gw * 2.0 ** -s, q.sum((0, 1, 2)) * 2.0 ** -s


def split(P, cu_count):
    """train_conv_split: (chunks, chunks per slice, slices) of P output pixels"""
    chunks = (P + CHUNK - 1) // CHUNK
    want = max(1, min(chunks, (2 * max(1, cu_count) + 8) // 9))
    per = (chunks + want - 1) // want
    return chunks, per, (chunks + per - 1) // per


def packed_index(cin, cout, kh, kw, ci, co):
    return ((kh * (3 * cin // 8) + kw * (cin // 8) + ci // 8) * cout + co) * 8 + ci % 8


def stored(G, s):
    """delta(l) as the device stores and hands it out: binary16(G 2^s) 2^-s"""
    return R.quantise(np.asarray(G, f32), s).astype(np.float64) * 2.0 ** -s


# the derived bounds (tests/test_train_conv_gpu.py uses the same): a sum of `terms` exact binary32 products in any order errs by at most (terms + 1) 2^-24
# sum |terms|; storing a value as binary16 under 2^s adds 2^-11 of it (normal) or half a subnormal step, 2^-25 2^-s
def stored_bound(ref, sum_abs, terms, s):
    acc = (terms + 1) * U * np.asarray(sum_abs)
    return acc * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 * 2.0 ** -s


def wgrad_bounds(xin, q, s, cu_count):
    """(bound of gW, bound of gb): a slice's running sum of at most per_slice x 64 products, then the slices in order"""
    n, OH, OW, _ = np.shape(q)
    _, per, slices = split(n * OH * OW, cu_count)
    aw, ab = wgrad(np.abs(np.asarray(xin, np.float64)), np.abs(np.asarray(q, np.float64)), s)
    k = (per * CHUNK + slices + 1) * U
    return k * aw, k * ab


# ---- the restatement against autograd, and what the reference notices ----------------------------------------------------------------------------
def small_case(n, ih, iw, seed):
    """conv6 -> conv7 -> dense1 on an ih x iw x 64 input: binary16-valued activations and weights, q1 as the tail would hand it over"""
    rng = np.random.default_rng(seed)
    h16 = lambda a: np.asarray(a, f32).astype(np.float16).astype(np.float64)
    x5 = h16(np.maximum(rng.normal(0.3, 1.0, (n, ih, iw, 64)), 0))
    k6, k7 = h16(rng.normal(0, 0.06, (3, 3, 64, 128))), h16(rng.normal(0, 0.05, (3, 3, 128, 128)))
    b6, b7 = rng.normal(0, 0.05, 128), rng.normal(0, 0.05, 128)
    F = (ih - 4) * (iw - 4) * 128
    w1 = h16(rng.normal(0, 0.1, (F, 100)))
    d1 = (rng.normal(0, 1e-3, (n, 100)) * (rng.random((n, 100)) < 0.6)).astype(f32)
    return x5, k6, b6, k7, b7, w1, d1


def conv_nhwc(torch, x, k, b):
    import torch.nn.functional as Fn
    return Fn.conv2d(x.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), b).permute(0, 2, 3, 1)


CASES = [(2, 7, 8), (3, 5, 5), (2, 5, 6)]      # x5 (x 64): conv7's input x6 is 5 x 6 and 3 x 3, x7 is 3 x 4 and 1 x 1; and a 5 x 6 (x 64) input, x7 1 x 2


@pytest.mark.parametrize("n,ih,iw", CASES)
def test_restatement_matches_autograd_float64(n, ih, iw):
    import torch
    x5, k6, b6, k7, b7, w1, d1 = small_case(n, ih, iw, seed=ih)
    T = {k: torch.tensor(v, requires_grad=True) for k, v in (("x5", x5), ("k6", k6), ("b6", b6), ("k7", k7), ("b7", b7))}
    x6t = torch.relu(conv_nhwc(torch, T["x5"], T["k6"], T["b6"]))
    x7t = torch.relu(conv_nhwc(torch, x6t, T["k7"], T["b7"]))
    s1 = R.scale_exponent(R.max_abs_bits(d1))
    q1 = R.quantise(d1, s1).astype(np.float64)
    up = q1 * 2.0 ** -s1                                                    # dL/dz1 as the tail hands it on
    ((x7t.reshape(n, -1) @ torch.tensor(w1)) * torch.tensor(up)).sum().backward(inputs=list(T.values()))
    x6, x7 = x6t.detach().numpy(), x7t.detach().numpy()
    assert 0.2 < (x7 > 0).mean() < 0.8 and 0.2 < (x6 > 0).mean() < 0.8
    # no quantisation in between (s = 0 and binary64 values): the rules are autograd's
    G7 = g7(x7.reshape(n, -1), w1, q1, s1).reshape(x7.shape)
    gw7, gb7 = wgrad(x6, G7, 0)
    G6 = dgrad(G7, k7, x6, 0)
    gw6, gb6 = wgrad(x5, G6, 0)
    G5 = dgrad(G6, k6, np.ones_like(x5), 0)                                 # (x5 is a leaf: no mask)
    for got, want, what in ((gw7, T["k7"].grad, "gW7"), (gb7, T["b7"].grad, "gb7"), (gw6, T["k6"].grad, "gW6"), (gb6, T["b6"].grad, "gb6"), (G5, T["x5"].grad, "G5")):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-10, atol=1e-16, err_msg=what)
    # with each delta stored as binary16 under its scale, the gradients stay within binary16's precision of the exact ones, measured on the absolute sums
    s7 = scale_of(G7)
    q7 = R.quantise(G7.astype(f32), s7)
    gw7q, _ = wgrad(x6, q7, s7)
    assert (np.abs(gw7q - gw7) <= 2.0 ** -10 * wgrad(np.abs(x6), np.abs(G7), 0)[0] + 2.0 ** -24 * 2.0 ** -s7 * np.abs(x6).sum() + 1e-30).all()


@pytest.mark.parametrize("n,ih,iw", CASES)
def test_the_reference_notices_each_mistake_tenfold(n, ih, iw):
    """Before any comparison: against the bounds the GPU test allows, the reference moves at least ten times as far when one tap is shifted, one frame is
    dropped, the last k-step of a reduction is dropped, or one 64-channel half of conv7's input is dropped."""
    x5, k6, b6, k7, b7, w1, d1 = small_case(n, ih, iw, seed=ih)
    x6 = np.maximum(sum(np.einsum("nyxc,co->nyxo", x5[:, kh:kh + ih - 2, kw:kw + iw - 2], k6[kh, kw]) for kh in range(3) for kw in range(3)) + b6, 0)
    x6 = x6.astype(np.float16).astype(np.float64)
    x7 = np.maximum(sum(np.einsum("nyxc,co->nyxo", x6[:, kh:kh + ih - 4, kw:kw + iw - 4], k7[kh, kw]) for kh in range(3) for kw in range(3)) + b7, 0)
    x7 = x7.astype(np.float16).astype(np.float64)
    s1 = R.scale_exponent(R.max_abs_bits(d1))
    q1 = R.quantise(d1, s1).astype(np.float64)
    G7 = g7(x7.reshape(n, -1), w1, q1, s1).reshape(x7.shape)
    s7 = scale_of(G7)
    q7 = R.quantise(G7.astype(f32), s7).astype(np.float64)
    b_g7 = stored_bound(G7, g7_abs(w1, q1, s1).reshape(x7.shape), 128, s7)
    G6 = dgrad(q7, k7, x6, s7)
    b_g6 = stored_bound(G6, dgrad_abs(q7, k7, x6, s7), 9 * 128, scale_of(G6))
    gw7, gb7 = wgrad(x6, q7, s7)
    b_gw7, b_gb7 = wgrad_bounds(x6, q7, s7, 256)

    def moved(a, b, bound):                                                 # over the values that have a bound (a sum without terms is exactly zero)
        return float((np.abs(a - b)[bound > 0] / bound[bound > 0]).max())

    noticed = {}
    noticed["a shifted tap, G6"] = moved(dgrad(q7, np.roll(k7, 1, axis=1), x6, s7), G6, b_g6)     # tap (kh, kw) reads the kernel of (kh, kw - 1)
    rolled = np.stack([np.stack([wgrad(np.roll(x6, 1, axis=2), q7, s7)[0][kh, kw] for kw in range(3)]) for kh in range(3)])
    noticed["a shifted tap, gW7"] = moved(rolled, gw7, b_gw7)
    noticed["a dropped frame, gW7"] = moved(wgrad(x6[1:], q7[1:], s7)[0], gw7, b_gw7)
    noticed["a dropped frame, gb7"] = moved(wgrad(x6[1:], q7[1:], s7)[1], gb7, b_gb7)
    q7_cut = q7.reshape(-1, 128).copy()
    q7_cut[-(len(q7_cut) % 16 or 16):] = 0                                  # the last k-step of 16 pixels of the weight gradient's reduction
    noticed["the last k-step dropped, gW7"] = moved(wgrad(x6, q7_cut.reshape(q7.shape), s7)[0], gw7, b_gw7)
    q1_cut = q1.copy(); q1_cut[:, 96:] = 0                                  # the last k-step of 16 outputs of G7's reduction (outputs 96 .. 99 are real)
    noticed["the last k-step dropped, G7"] = moved(g7(x7.reshape(n, -1), w1, q1_cut, s1).reshape(x7.shape), G7, b_g7)
    k7_half = k7.copy(); k7_half[:, :, 64:, :] = 0                          # conv7's input channels 64 .. 127
    noticed["a 64-channel half of conv7's input dropped, G6"] = moved(dgrad(q7, k7_half, x6, s7), G6, b_g6)
    x6_half = x6.copy(); x6_half[..., 64:] = 0
    noticed["a 64-channel half of conv7's input dropped, gW7"] = moved(wgrad(x6_half, q7, s7)[0], gw7, b_gw7)
    print(f"{n} x {ih}x{iw}: " + ", ".join(f"{k} {v:.0f} x the bound" for k, v in noticed.items()))
    assert all(v >= 10.0 for v in noticed.values()), noticed


# ---- the host-only rules under a sanitizer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train_conv") / "train_conv_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", ROOT, os.path.join(ROOT, "tests", "train_conv_driver.cpp"), "-o", exe])
    return exe


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.split()


def test_driver_mask_refusals(conv_driver):
    assert run(conv_driver, "mask") == ["ok"]


def test_driver_master_layout(conv_driver):
    off = [int(x) for x in run(conv_driver, "layout")]
    sizes = []
    for cin, cout in CHANNELS:
        sizes += [9 * cin * cout, cout]
    assert off == [sum(sizes[:a]) for a in range(9)] and off[8] == 294912 + 384


def test_driver_packed_index_is_pack_layers(conv_driver):
    """every layer: pack_layer on a kernel of distinct binary16 values (0, 1, 2, ... as small integers times 2^-k) puts K[kh][kw][ci][co] where the index says"""
    for j, (cin, cout) in enumerate(CHANNELS):
        out = run(conv_driver, "pack", j)
        assert out[0] == "ok" and int(out[1]) == 9 * cin * cout, out
        probe = [(0, 0, 0, 0), (2, 2, cin - 1, cout - 1), (1, 2, 9, 33), (2, 0, 17, 5)]
        got = [int(x) for x in run(conv_driver, "index", j, *[v for p in probe for v in p])]
        assert got == [packed_index(cin, cout, *p) for p in probe]


@pytest.mark.parametrize("ih,iw", [(9, 9), (10, 14), (12, 17), (14, 35), (27, 37)])        # x3 of 93x100, 96x128, 120x160, 130x300, 240x320
def test_driver_split_covers_every_pixel_once(conv_driver, ih, iw):
    for j in range(4):
        oh, ow = ih - 2 * (j + 1), iw - 2 * (j + 1)
        for n in (1, 3, 70):
            for cu in (256, 1, 304):
                v = [int(x) for x in run(conv_driver, "split", j, ih - 2 * j, iw - 2 * j, n, cu)]
                P, chunks, per, slices = v[:4]
                assert P == n * oh * ow and (chunks, per, slices) == split(P, cu)
                spans = list(zip(v[4::2], v[5::2]))
                assert len(spans) == slices and spans[0][0] == 0 and spans[-1][1] == P
                assert all(a < b for a, b in spans) and all(spans[i][1] == spans[i + 1][0] for i in range(slices - 1))
                assert all(a % CHUNK == 0 for a, _ in spans)


def test_driver_sizes_and_debug_items(conv_driver):
    v = [int(x) for x in run(conv_driver, "sizes", 12, 17, 70, 256, 2)]      # 120x160, 70 frames, trained from conv6 up
    assert v[:5] == [70 * 6 * 11 * 128, 0, 0, 70 * 6 * 11 * 128, 70 * 4 * 9 * 128]
    assert v[5] == min((70 * 4 * 9 + 63) // 64, 57) * (9 * 128 * 128 + 128)   # the most slices any n <= 70 can have: one per chunk of the 70 frames' 40
    d = [int(x) for x in run(conv_driver, "debug", 3, 6, 11, 37)]            # conv7 over 6 x 11, 37 frames: items 0 .. 8, then 9 and -1
    assert d == [37 * 4 * 9 * 128, 147456, 128, 147456, 147456, 128, 128, 1, 147456, 0, 0]


@pytest.mark.parametrize("ih3,iw3,n_cap", [(12, 17, 1024), (12, 17, 102), (10, 14, 64), (9, 9, 300), (14, 35, 130), (27, 37, 512)])
@pytest.mark.parametrize("cu,lowest", [(256, 0), (256, 3), (304, 1), (7, 0)])
def test_driver_every_batch_size_fits_the_buffers(conv_driver, ih3, iw3, n_cap, cu, lowest):
    """slices(n) does not grow steadily with n: at 120x160 and 256 CUs conv7 has 53 slices at n = 1024 and 57 at n = 1000 or 100.  Every n in 1 .. n_cap must fit
    what the session allocated for n_cap, and the buffer is no larger than the largest need times the slack of one slice count (57 against 53)."""
    out = run(conv_driver, "fits", ih3, iw3, n_cap, cu, lowest)
    assert out[0] == "ok", " ".join(out)
    part = [int(x) for x in run(conv_driver, "sizes", ih3, iw3, n_cap, cu, lowest)][5]
    assert int(out[1]) <= part <= int(out[1]) * 1.25


def test_the_slice_count_is_not_monotone():
    assert split(1024 * 36, 256)[2] == 53 and split(1000 * 36, 256)[2] == 57 and split(100 * 36, 256)[2] == 57


# ---- the library without a device ----------------------------------------------------------------------------------------------------------
def test_ffi_binds_the_conv_training_symbols():
    assert set(_ffi.TRAIN_CONV_SYMBOLS) <= set(_ffi.PILOT_SYMBOLS)
    assert _ffi.TRAIN_CONV_LAYERS == ("conv4", "conv5", "conv6", "conv7")


def test_refusals_without_a_device(hip_api):
    arrs = (C.c_void_p * 8)()
    for call in (lambda: hip_api.pilot_train_convs(None, 0xF, arrs), lambda: hip_api.pilot_train_get_convs(None, arrs),
                 lambda: hip_api.pilot_train_debug_conv(None, 0, 0, None, 0)):
        assert call() == -1 and b"null handle" in hip_api.last_error()
