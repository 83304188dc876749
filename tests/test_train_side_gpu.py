"""Training the speed-as-feature pilot on the device (include/trsim_spec.h, "training the pilot's tail, side branch"; the SIDE kernels of
csrc/trsim_train.hip) against the numpy restatement of tests/test_train_side_cpu.py.  As in tests/test_train_gpu.py the reference behind conv7 starts from the
kernel's own conv7 activation and every value the step hands out is compared with the binary64 evaluation of the sum that defines it, over the inputs the kernel
read.  Exact rules are compared bit for bit: out against trs_pilot_forward_ex, fin and y1 .. y3 against a binary32 restatement of the same fmaf chains, Adam
from the device's own gradients, the dropout masks.

Tolerances are derived, not measured: tests/test_train_gpu.py's running-sum bound (terms + 1) 2^-24 sum |terms| per value.  New here: z1 carries 16 more
fmaf steps behind the slabs' sum (chain_bound over y3 and W1Y with the slabs' sum as the start, added to the matrix-core bound of that sum); delta-y3, delta-y2,
delta-y1 are chains of 100, 16 and 8 terms from 0; the branch's gradients are sums over the n frames like the other small ones, gF1's terms being products
rounded once each, which the same (n + 1) 2^-24 sum |terms| covers (n - 1 additions and one rounding per term).  The branch's ReLU masks are the stored
activations' own, so no frame is left out for them; the tail's masks are the reference's, with the frames near a kink left out as before."""
import ctypes as C
import time

import numpy as np
import pytest

import test_dropout_cpu as D
import test_train_cpu as R
import test_train_side_cpu as S
from test_pilot import planner                                                              # noqa: F401  (a fixture)
from test_pilot_plan_cpu import call_of, driver                                             # noqa: F401  (driver is a fixture)
from test_pilot_slices import flatten_shape, slice_frames
from test_pilot_types import conv_stack_pure
from test_train_conv_gpu import ALL, LAYERS, ConvTrainer, check_conv_step, halves
from test_train_gpu import (BATCH, CAP, EPOCHS, SMALL, TAIL, WIDE, Trainer, U, bits, chain_bound, labels_for, params_of, tail_weights, worst,
                            z1_reference)
from triton_racer_sim_amd import _ffi

f32, f64 = np.float32, np.float64
KIND = "cnn_2d_speed_as_feature"
TINY = (93, 100)                                # conv7 is one pixel: F = 128, one feature tile
SIDE_BATCHES = (1, 15, 17, 37, 70)              # ragged and whole k-steps of 16 frames, a second 64-frame GEMM chunk
SIDE_ARRAYS = tuple(_ffi.TRAIN_SIDE_ARRAYS)     # w1y, f1w, f1b, f2w, f2b, f3w, f3b
SHAPES = {"w1y": (16, 100), "f1w": (1, 4), "f1b": (4,), "f2w": (4, 8), "f2b": (8,), "f3w": (8, 16), "f3b": (16,)}
BRANCH = ("feature1", "feature2", "feature3")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def side_weights(h, w, seed):
    """tail_weights' 28 arrays with the branch drawn again: kernels of positive entries and biases of both signs, so a large feature lights every unit and a
    small one leaves the units with a negative bias dead (asserted from the restatement before anything is compared: branch_is_mixed)"""
    named, F = tail_weights(h, w, seed=seed, kind=KIND)
    rng = np.random.default_rng(seed + 23)
    for l, nm in enumerate(BRANCH, 1):
        k = np.abs(R.glorot(rng, S.WIDTHS[l - 1], S.WIDTHS[l])) + f32(0.05)
        b = rng.uniform(0.05, 0.3, S.WIDTHS[l]).astype(f32) * np.where(np.arange(S.WIDTHS[l]) % 2 == 0, f32(-1.0), f32(1.0))
        named[nm] = (k.astype(f32), b.astype(f32))
    return named, F


def speeds_for(n, seed):
    """'gym/speed' per frame: 0, a negative one and one large enough to light every branch unit among them (from three frames on)"""
    s = np.random.default_rng(seed).uniform(0.0, 20.0, n).astype(f32)
    s[:3] = np.array([0.0, -5.0, 120.0], f32)[:n]
    return s


def features_of(speed):
    """s20 as the speed_feature loader delivers it and trs_pilot_tail_ex_kernel computes it: one binary32 division"""
    return (np.asarray(speed, f32) / f32(20.0)).astype(f32)


def side_params(named):
    P = params_of(named)
    for l, nm in enumerate(BRANCH, 1):
        P[f"f{l}w"], P[f"f{l}b"] = np.asarray(named[nm][0], f32), np.asarray(named[nm][1], f32)
    return P


def params_from(arrays):
    return dict(zip(S.NAMES, arrays))


def fma32(x, y, z):
    """fmaf in numpy: the product of two binary32 values is exact in binary64; the sum is rounded to odd there (TwoSum gives what the addition lost), so
    the final rounding to binary32 is the single rounding of the exact x y + z"""
    p, z = np.asarray(x, f64) * np.asarray(y, f64), np.asarray(z, f64)
    s = p + z
    bb = s - p
    err = (p - (s - bb)) + (z - bb)
    si = np.ascontiguousarray(s).view(np.int64)
    fix = (err != 0) & ((si & 1) == 0)
    larger = (err > 0) == (s > 0)
    si = np.where(fix, np.where(larger, si + 1, si - 1), si)
    return si.view(f64).astype(f32)


def branch32(fin, P):
    """(y1, y2, y3) in binary32 as the kernels chain them: from the bias, k ascending, one fmaf per term, then the ReLU"""
    y, out = np.asarray(fin, f32).reshape(-1, 1), []
    for l in (1, 2, 3):
        w, s = P[f"f{l}w"], np.broadcast_to(P[f"f{l}b"], (len(y), S.WIDTHS[l])).astype(f32)
        for k in range(w.shape[0]):
            s = fma32(y[:, k:k + 1], w[k][None, :], s)
        y = np.maximum(s, f32(0.0))
        out.append(y)
    return out


def branch_is_mixed(fin, P):
    """every branch layer has a unit that is dead for one frame and alive for another, and the largest feature lights every unit"""
    ys = S.branch(fin, P)
    big = int(np.argmax(fin))
    return all(((y > 0).any(0) & ~(y > 0).all(0)).any() for y in ys) and all((y[big] > 0).all() for y in ys)


def side_reference(x7, fin, P, gps):
    """test_train_gpu.pure_reference with the branch: the chain from conv7's activation and the feature alone, its bounds, the frames to leave out"""
    F = x7.shape[1]
    flat = dict(P, w1=P["w1"][:F])
    zf, bf = z1_reference(x7, flat, gps)
    f = S.forward(zf, fin, P)
    b1 = bf + chain_bound(f["y3"], P["w1"][F:], zf, 16)
    b2 = chain_bound(np.maximum(f["z1"], 0), P["w2"], P["b2"], 100)
    b3 = chain_bound(np.maximum(f["z2"], 0), P["w3"], P["b3"], 50)
    near = (np.abs(f["z1"]) < 10 * b1).any(1) | (np.abs(f["z2"]) < 10 * b2).any(1) | (np.abs(f["z3"]) < 10 * b3).any(1)
    return dict(f, zf=zf, bound_flat=bf, near=near)


# ---- on the CPU: the condition on the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,n,ksplit", [TINY + (37, 0), SMALL + (70, 0), WIDE + (37, 1), WIDE + (37, 10)])
def test_the_reference_alone_keeps_the_cap(driver, h, w, n, ksplit):
    named, F = side_weights(h, w, seed=3)
    P = side_params(named)
    fin = features_of(speeds_for(n, seed=n))
    assert branch_is_mixed(fin, P)
    x7 = np.asarray(conv_stack_pure(slice_frames(h, w, n, seed=1), named), f32).astype(np.float16)
    call = call_of(driver, h, w, n, n, arrays=28, **({"ksplit": ksplit} if ksplit else {}))
    assert call["G"] * 8 == F and (ksplit == 0 or call["KS"] == ksplit)
    ref = side_reference(x7, fin, P, call["gps"])
    active = float((ref["z1"] > 0).mean())
    moved = float(np.abs(ref["z1"] - ref["zf"]).mean())
    print(f"{h}x{w}, {n} frames, KS {call['KS']}: {ref['near'].mean():.3f} of the frames left out, {active:.2f} of dense1's units active, the branch moves z1 by "
          f"{moved:.2f} on average, max |out| {np.abs(ref['out']).max():.2f}")
    assert ref["near"].mean() <= CAP
    assert 0.2 <= active <= 0.8 and moved > 0.05
    assert 0.1 <= (ref["z2"] > 0).mean() <= 0.9 and 0.1 <= (ref["z3"] > 0).mean() <= 0.9


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------
class SideTrainer(Trainer):
    """test_train_gpu.Trainer on a 28-array pilot: a step also takes the frames' speeds, which go up as the feature s20"""

    def step(self, frames, y, speed):
        d_frames, d_y = self.upload(frames, y)
        d_f = self.env.scratch(22, (len(frames), 1), np.float32)
        self.env.upload(d_f, features_of(speed).reshape(-1, 1))
        return self.env.pilot_train_step(d_frames, d_y, len(frames), features=d_f)

    def debug(self, n):
        d = Trainer.debug(self, n)
        e = self.env
        for k, (_, width) in _ffi.TRAIN_SIDE_DEBUG.items():
            if width is not None:
                d[k] = e.pilot_train_debug_side(k).reshape(n, width)
        for nm in SIDE_ARRAYS:
            d["g_" + nm] = e.pilot_train_debug_side("g", nm).reshape(SHAPES[nm])
        return d

    def gradients(self):
        """the 14 gradients in the order of the trained arrays: dense1's whole kernel is the GEMM's rows and W1Y's behind them"""
        g = Trainer.gradients(self)
        side = [self.env.pilot_train_debug_side("g", nm).copy() for nm in SIDE_ARRAYS]
        return [np.concatenate([g[0], side[0]])] + g[1:] + side[1:]

    def moments(self):
        e, out = self.env, []
        for item in ("m", "v"):
            tail = [e.pilot_train_debug(item, a).copy() for a in range(8)]
            side = [e.pilot_train_debug_side(item, nm).copy() for nm in SIDE_ARRAYS]
            out.append([np.concatenate([tail[0], side[0]])] + tail[1:] + side[1:])
        return out


def check_side_step(P, y, fin, d, gps, tag):
    """One step's debug items against the restatement; P: the 14 arrays the step read.  Prints the largest |error| / bound per quantity."""
    n, F = len(y), d["x7"].shape[1]
    x7, y64 = d["x7"], y.astype(f64)
    ref = side_reference(x7, fin, P, gps)
    keep = ~ref["near"]
    W = {k: P[k].astype(f64) for k in ("w2", "w3", "w4", "f2w", "f3w")}
    W1Y = P["w1"][F:].astype(f64)
    # exact rules: the feature as given, the branch's chains
    assert np.array_equal(bits(d["fin"].ravel()), bits(fin)), tag
    for l, yl in enumerate(branch32(fin, P), 1):
        assert np.array_equal(bits(d[f"y{l}"]), bits(yl)), (tag, l, int((bits(d[f"y{l}"]) != bits(yl)).sum()))
    y1, y2, y3 = (d[k].astype(f64) for k in ("y1", "y2", "y3"))
    ratios = {}
    # forward, stage by stage from the values the kernel read: z1 is the slabs' sum and 16 fmaf steps over the device's own y3
    ratios["z1"] = worst(d["z1"], ref["zf"] + y3 @ W1Y, ref["bound_flat"] + chain_bound(y3, P["w1"][F:], ref["zf"], 16))
    a1, a2, a3 = (np.maximum(d[k].astype(f64), 0) for k in ("z1", "z2", "z3"))
    for k, a, l, terms in (("z2", a1, 2, 100), ("z3", a2, 3, 50), ("out", a3, 4, 25)):
        ratios[k] = worst(d[k], a @ W[f"w{l}"] + P[f"b{l}"].astype(f64), chain_bound(a, P[f"w{l}"], P[f"b{l}"], terms))
    # backward through the tail: the reference's masks, the frames near a kink left out
    out64 = d["out"].astype(f64)
    ratios["delta4"] = worst(d["delta4"], (out64 - y64) / n, 3 * U * (np.abs(out64) + np.abs(y64)) / n)
    d4, d3, d2, d1 = (d[k].astype(f64) for k in ("delta4", "delta3", "delta2", "delta1"))
    ratios["delta3"] = worst(d["delta3"], (d4 @ W["w4"].T) * (ref["z3"] > 0), 3 * U * (np.abs(d4) @ np.abs(W["w4"]).T), keep)
    ratios["delta2"] = worst(d["delta2"], (d3 @ W["w3"].T) * (ref["z2"] > 0), 26 * U * (np.abs(d3) @ np.abs(W["w3"]).T), keep)
    ratios["delta1"] = worst(d["delta1"], (d2 @ W["w2"].T) * (ref["z1"] > 0), 51 * U * (np.abs(d2) @ np.abs(W["w2"]).T), keep)
    # and through the branch: the masks are the stored activations' own
    dy3, dy2, dy1 = (d[k].astype(f64) for k in ("dy3", "dy2", "dy1"))
    ratios["dy3"] = worst(d["dy3"], (d1 @ W1Y.T) * (y3 > 0), 101 * U * (np.abs(d1) @ np.abs(W1Y).T))
    ratios["dy2"] = worst(d["dy2"], (dy3 @ W["f3w"].T) * (y2 > 0), 17 * U * (np.abs(dy3) @ np.abs(W["f3w"]).T))
    ratios["dy1"] = worst(d["dy1"], (dy2 @ W["f2w"].T) * (y1 > 0), 9 * U * (np.abs(dy2) @ np.abs(W["f2w"]).T))
    for l, yl in ((1, y1), (2, y2), (3, y3)):
        assert not d[f"dy{l}"][yl == 0].any(), (tag, l)
    # the small gradients: sums over the frames of the kernel's own activations and deltas
    for l, a, dl in ((2, a1, d2), (3, a2, d3), (4, a3, d4)):
        ratios[f"gw{l}"] = worst(d[f"gw{l}"], a.T @ dl, (n + 1) * U * (np.abs(a).T @ np.abs(dl)))
    for l, dl in ((1, d1), (2, d2), (3, d3), (4, d4)):
        ratios[f"gb{l}"] = worst(d[f"gb{l}"], dl.sum(0), (n + 1) * U * np.abs(dl).sum(0))
    fin64 = fin.astype(f64).reshape(-1, 1)
    for nm, a, dl in (("w1y", y3, d1), ("f3w", y2, dy3), ("f2w", y1, dy2), ("f1w", fin64, dy1)):
        ratios["g_" + nm] = worst(d["g_" + nm], a.T @ dl, (n + 1) * U * (np.abs(a).T @ np.abs(dl)))
    for nm, dl in (("f3b", dy3), ("f2b", dy2), ("f1b", dy1)):
        ratios["g_" + nm] = worst(d["g_" + nm], dl.sum(0), (n + 1) * U * np.abs(dl).sum(0))
    # dense1's flatten rows: the same products in binary64
    g_ref, tol, s = R.gw1_reference(x7, d["delta1"])
    assert d["s"] == s, (tag, d["s"], s)
    ratios["gw1"] = worst(d["gw1"], g_ref, tol)
    left = float(ref["near"].mean())
    print(f"{tag}: s = {s}, left out {left:.3f}; max |error| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)
    assert n < 20 or left <= CAP, (tag, left)
    if n >= 3:
        assert branch_is_mixed(fin, P), tag
        assert all(d["g_" + nm].any() for nm in SIDE_ARRAYS), tag
    return ref


def forward_of(env, frames, speed):
    return env.pilot_forward_host(frames, speed=speed)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,batches", [TINY + ((37,),), SMALL + (SIDE_BATCHES,)], ids=["93x100", "120x160"])
def test_forward_identity_branch_backward_and_gradients_at_every_batch_shape(make_env, planner, h, w, batches):
    """One handle per batch size: out of the step equals trs_pilot_forward_ex bit for bit, fin and y1 .. y3 the binary32 restatement; z, the deltas, every
    gradient and gW1 against the binary64 restatement; two runs of the step's gradients agree bit for bit."""
    t0 = time.perf_counter()
    named, F = side_weights(h, w, seed=3)
    P = side_params(named)
    all_frames = slice_frames(h, w, max(batches), seed=1)
    for n in batches:
        frames, y, speed = all_frames[:n], labels_for(n, seed=n), speeds_for(n, seed=n)
        call = planner.call(h, w, n, n, arrays=28)
        tr = SideTrainer(make_env, h, w, n, named)
        fwd = forward_of(tr.env, frames, speed)
        loss = tr.step(frames, y, speed)
        d = tr.debug(n)
        assert np.array_equal(bits(d["out"]), bits(fwd)), n
        assert abs(loss - float(((d["out"].astype(f64) - y) ** 2).sum() / (2 * n))) <= (2 * n + 1) * U * loss + 1e-12
        check_side_step(P, y, features_of(speed), d, call["gps"], f"{h}x{w} n = {n}")
        twin = SideTrainer(make_env, h, w, n, named)
        twin.step(frames, y, speed)
        for a, b in zip(tr.gradients(), twin.gradients()):
            assert np.array_equal(bits(a), bits(b)), n
    print(f"{len(batches)} batch sizes took {time.perf_counter() - t0:.2f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("ksplit", [1, 10])
def test_wide_frames_at_two_slice_counts_and_a_smaller_batch_behind_a_larger(make_env, planner, ksplit):
    """130x300 at 1 and 10 K slices, 37 frames, then 17 frames on the same handle with the 14 arrays the first step left"""
    h, w = WIDE
    named, F = side_weights(h, w, seed=3)
    frames, y, speed = slice_frames(h, w, 37, seed=1), labels_for(37, seed=5), speeds_for(37, seed=5)
    call = planner.call(h, w, 37, 37, arrays=28, ksplit=ksplit)
    assert call["KS"] == ksplit and F == 16640
    tr = SideTrainer(make_env, h, w, 37, named, ksplit=ksplit)
    speed2 = speeds_for(17, seed=6)                                      # the smaller batch's own 0, negative and large speed
    before2 = forward_of(tr.env, frames[20:37], speed2)
    fwd = forward_of(tr.env, frames, speed)
    tr.step(frames, y, speed)
    d = tr.debug(37)
    assert np.array_equal(bits(d["out"]), bits(fwd))
    check_side_step(side_params(named), y, features_of(speed), d, call["gps"], f"{h}x{w} KS {ksplit} n = 37")
    arrays, t = tr.env.pilot_train_weights()
    assert t == 1 and len(arrays) == 14
    small = planner.call(h, w, 37, 17, arrays=28, ksplit=ksplit)
    fwd2 = forward_of(tr.env, frames[20:37], speed2)                     # the handle drives with the updated pilot, with no pilot_load
    assert np.abs(fwd2 - before2).max() > 1e-4
    tr.step(frames[20:37], y[20:37], speed2)
    d2 = tr.debug(17)
    assert np.array_equal(bits(d2["out"]), bits(fwd2))
    check_side_step(params_from(arrays), y[20:37], features_of(speed2), d2, small["gps"], f"{h}x{w} KS {ksplit} n = 17 behind 37")


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [None, ("feature2",)], ids=["all", "feature2"])
def test_adam_reproduces_bit_for_bit_from_the_device_gradient(make_env, layers):
    """Steps t = 1, 2, 3 on different batches: from the gradients the device hands out, the numpy float32 restatement gives m, v and the 14 masters bit for
    bit (dense1's kernel whole: the GEMM's rows and W1Y); a layer that is not named keeps every bit of its weights and moments; the forward pass after the
    steps equals that of a fresh handle given pilot_weights(): W1Y and the branch moved where trs_pilot_tail_ex_kernel reads them."""
    h, w = SMALL
    named, F = side_weights(h, w, seed=3)
    frames, speed = slice_frames(h, w, 48, seed=1), speeds_for(48, seed=9)
    tr = SideTrainer(make_env, h, w, 16, named, lr=2e-3, layers=layers)
    names = TAIL + BRANCH
    w_prev = [np.asarray(named[l][j], f32).ravel().copy() for l in names for j in (0, 1)]
    m_prev, v_prev = [np.zeros_like(a) for a in w_prev], [np.zeros_like(a) for a in w_prev]
    trained = [layers is None or names[a // 2] in layers for a in range(14)]
    before = forward_of(tr.env, frames[:16], speed[:16])
    for t in (1, 2, 3):
        sl = slice(16 * (t - 1), 16 * t)
        tr.step(frames[sl], labels_for(16, seed=40 + t), speed[sl])
        g = tr.gradients()
        (m, v), (arrays, steps) = tr.moments(), tr.env.pilot_train_weights()
        assert steps == t and len(arrays) == 14
        for a in range(14):
            want = R.adam(g[a], m_prev[a], v_prev[a], w_prev[a], t, lr=2e-3) if trained[a] else (m_prev[a], v_prev[a], w_prev[a])
            for got, ref, what in zip((m[a], v[a], arrays[a].ravel()), want, "mvw"):
                assert np.array_equal(bits(got), bits(ref)), (t, S.NAMES[a], what, int((bits(got) != bits(ref)).sum()))
            assert g[a].any(), (t, S.NAMES[a])
            m_prev[a], v_prev[a], w_prev[a] = m[a], v[a], arrays[a].ravel().copy()
        with np.errstate(over="ignore"):
            assert np.array_equal(bits(tr.env.pilot_train_debug("pack1")), bits(arrays[0][:F].astype(np.float16).astype(f32)).ravel()), t
    moved = [float(np.abs(w_prev[a] - np.asarray(named[names[a // 2]][a % 2]).ravel()).max()) for a in range(14)]
    assert all(mv > 1e-3 if trained[a] else mv == 0.0 for a, mv in enumerate(moved)), moved
    if layers is None:
        assert float(np.abs(arrays[0][F:] - named["dense1"][0][F:]).max()) > 1e-3         # W1Y itself
    after = forward_of(tr.env, frames[:16], speed[:16])
    assert np.abs(after - before).max() > 1e-5
    weights = tr.env.pilot_weights()
    assert len(weights) == 28 and all(np.array_equal(weights[i], tr.env._pilot_arrays[i]) for i in range(14))
    assert all(np.array_equal(weights[14 + a], arrays[a]) for a in range(14))
    fresh = make_env("hip", n_envs=16, img_h=h, img_w=w)
    fresh.pilot_load(weights)
    assert np.array_equal(bits(forward_of(fresh, frames[:16], speed[:16])), bits(after))
    tr.env.pilot_train_end()
    assert np.array_equal(bits(forward_of(tr.env, frames[:16], speed[:16])), bits(after))
    assert all(np.array_equal(a, b) for a, b in zip(tr.env.pilot_weights(), weights))


@pytest.mark.gpu
def test_two_handles_agree_after_three_steps(make_env):
    h, w = SMALL
    named, F = side_weights(h, w, seed=3)
    frames, speed = slice_frames(h, w, 32, seed=1), speeds_for(32, seed=2)
    a, b = SideTrainer(make_env, h, w, 24, named), SideTrainer(make_env, h, w, 24, named)
    for t in range(3):
        sl, y = slice(4 * t, 4 * t + 24), labels_for(24, seed=60 + t)
        assert a.step(frames[sl], y, speed[sl]) == b.step(frames[sl], y, speed[sl])
    for x, y_ in zip(a.env.pilot_train_weights()[0], b.env.pilot_train_weights()[0]):
        assert np.array_equal(bits(x), bits(y_))
    for (ma, va), (mb, vb) in ((a.moments(), b.moments()),):
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(ma + va, mb + vb))
    assert np.array_equal(bits(forward_of(a.env, frames[:24], speed[:24])), bits(forward_of(b.env, frames[:24], speed[:24])))


@pytest.mark.gpu
def test_dropout_at_all_four_sites_leaves_the_branch_alone(make_env, planner):
    """120x160, 17 frames, all four sites: x7' and a'(l) are the host's masks applied, bit for bit; fin and y1 .. y3 are those of a step without dropout
    (the concatenation lies behind x7's Dropout and the feature layers have none), while out is not"""
    h, w, n = SMALL + (17,)
    named, F = side_weights(h, w, seed=3)
    frames, y, speed = slice_frames(h, w, n, seed=1), labels_for(n, seed=n), speeds_for(n, seed=n)
    tr = SideTrainer(make_env, h, w, n, named, dropout=D.DROP_RATE, dropout_sites=_ffi.DROPOUT_SITES, dropout_seed=D.DROP_SEED)
    plain = SideTrainer(make_env, h, w, n, named)
    fwd = forward_of(tr.env, frames, speed)                                        # inference never drops
    x7 = tr.env.pilot_layer(6, (n,) + flatten_shape(h, w)).reshape(n, -1)
    tr.step(frames, y, speed)
    plain.step(frames, y, speed)
    d, p = tr.debug(n), plain.debug(n)
    keep, s = D.masks_for(0xF, 1, n, F)
    for j in range(4):
        assert np.array_equal(tr.env.pilot_train_dropout_keep(1, j, n), keep[j]), j
    half = lambda a: np.ascontiguousarray(a, np.float16).view(np.uint16)
    assert np.array_equal(half(d["x7"]), half(D.drop_x7(x7.astype(np.float16), keep[0], s[0])))
    assert keep[0].shape == (n, F) and 0.05 < (~keep[0]).mean() < 0.15
    for l, width in ((1, 100), (2, 50), (3, 25)):
        a = tr.env.pilot_train_debug(f"a{l}").reshape(n, width)
        assert np.array_equal(bits(a), bits(D.drop_act(d[f"z{l}"], keep[l], s[l]))), l
        assert not d[f"delta{l}"][~keep[l]].any(), l
    for k in ("fin", "y1", "y2", "y3"):
        assert np.array_equal(bits(d[k]), bits(p[k])), k
    assert np.array_equal(bits(p["out"]), bits(fwd)) and not np.array_equal(bits(d["out"]), bits(fwd))
    # delta-y3 of the dropped step is the chain over ITS delta1, which carries site 1's mask and scale
    W1Y = named["dense1"][0][F:].astype(f64)
    d1, y3 = d["delta1"].astype(f64), d["y3"].astype(f64)
    assert worst(d["dy3"], (d1 @ W1Y.T) * (y3 > 0), 101 * U * (np.abs(d1) @ np.abs(W1Y).T)) <= 1.0
    assert not np.array_equal(bits(d["dy3"]), bits(p["dy3"]))


class SideConvTrainer(ConvTrainer):
    def step(self, frames, y, speed):
        d_frames, d_y = self.upload(frames, y)
        d_f = self.env.scratch(22, (len(frames), 1), np.float32)
        self.env.upload(d_f, features_of(speed).reshape(-1, 1))
        return self.env.pilot_train_step(d_frames, d_y, len(frames), features=d_f)


@pytest.mark.gpu
def test_96x128_the_convolutions_train_under_a_side_session(make_env):
    """conv4 .. conv7 under a 28-array session, 70 frames and then 3 on one handle: delta7 .. delta4 and the convolutions' gradients against
    tests/test_train_conv_gpu.py's reference within its bounds (G7 reads delta1's quantised copy, dense1's flatten granules and x7 alone)"""
    h, w, batches = 96, 128, (70, 3)
    named, F = side_weights(h, w, seed=3)
    frames, speed = slice_frames(h, w, max(batches), seed=1), speeds_for(max(batches), seed=4)
    tr = SideConvTrainer(make_env, h, w, max(batches), named, ALL)
    cur = halves(named)
    cur["dense1"] = cur["dense1"][:F]
    for n in batches:
        fwd = forward_of(tr.env, frames[:n], speed[:n])
        tr.step(frames[:n], labels_for(n, seed=n), speed[:n])
        assert np.array_equal(bits(tr.env.pilot_train_debug("out").reshape(n, 2)), bits(fwd)), n
        grads = check_conv_step(tr, cur, n, f"{h}x{w} n = {n} side session, all convolutions")
        assert set(grads) == set(LAYERS) and tr.env.pilot_train_debug_side("g", "f1w").any()
        for nm in LAYERS:
            cin, cout = named[nm][0].shape[2:]
            cur[nm] = tr.env.pilot_train_debug_conv(nm, "pack").reshape(3, 3, cin, cout).astype(f64)
        cur["dense1"] = tr.env.pilot_train_debug("pack1").reshape(F, 100).astype(f64)
    weights = tr.env.pilot_weights()
    assert len(weights) == 28 and all(np.abs(weights[i] - tr.env._pilot_arrays[i]).max() > 0 for i in range(6, 28))


@pytest.mark.gpu
def test_refusals_on_the_device(make_env):
    h, w = SMALL
    named, F = side_weights(h, w, seed=3)
    plain, _ = tail_weights(h, w, seed=3)
    house, _ = tail_weights(h, w, seed=3, kind="cnn_2d_full_house")
    env = make_env("hip", n_envs=8, img_h=h, img_w=w)
    api, hd = env.api, env._h
    w1 = np.ascontiguousarray(named["dense1"][0])
    arrs = (C.c_void_p * 14)(w1.ctypes.data, *([None] * 13))

    def refused(rc, code, text):
        assert rc == code, (rc, api.last_error())
        assert text in (api.last_error() or b"").decode(), api.last_error()

    refused(api.pilot_train_begin_ex(hd, None, arrs, 14), -2, "no pilot loaded")
    env.pilot_load(house)
    refused(api.pilot_train_begin_ex(hd, None, arrs, 14), -5, "42-array")
    refused(api.pilot_train_begin_ex(hd, None, arrs, 8), -5, "42-array")
    with pytest.raises(RuntimeError, match="42-array"):
        env.pilot_train_begin()
    env.pilot_load(plain)
    refused(api.pilot_train_begin_ex(hd, None, arrs, 14), -1, "does not match the loaded pilot")
    assert api.pilot_train_begin_ex(hd, None, arrs, 8) == 0                          # 8 arrays with a 22-array pilot is trs_pilot_train_begin
    refused(api.pilot_train_debug_side(hd, 0, w1.ctypes.data, 8), -2, "no side branch")
    refused(api.pilot_train_get_ex(hd, arrs, 14, None), -1, "does not match the session")
    env.pilot_train_end()
    env.pilot_load(named)
    refused(api.pilot_train_begin_ex(hd, None, arrs, 8), -1, "does not match the loaded pilot")
    refused(api.pilot_train_begin_ex(hd, None, arrs, 7), -1, "n_arrays")
    env.pilot_train_begin()
    refused(api.pilot_train_begin_ex(hd, None, arrs, 14), -2, "already open")
    frames = slice_frames(h, w, 8, seed=1)
    d_frames, d_y, d_f = env.scratch(20, (8, h, w, 3), np.uint8), env.scratch(21, (8, 2), np.float32), env.scratch(22, (8, 1), np.float32)
    env.upload(d_frames, frames); env.upload(d_y, labels_for(8, 1)); env.upload(d_f, features_of(speeds_for(8, 1)).reshape(-1, 1))
    pf, py, pq = (a.__cuda_array_interface__["data"][0] for a in (d_frames, d_y, d_f))
    refused(api.pilot_train_debug_side(hd, 0, w1.ctypes.data, 8), -2, "no training step yet")
    refused(api.pilot_train_step_ex(hd, pf, None, py, 8, None), -1, "d_features is NULL")
    refused(api.pilot_train_step(hd, pf, py, 8, None), -1, "trs_pilot_train_step_ex")
    refused(api.pilot_train_get(hd, arrs, None), -1, "trs_pilot_train_get_ex")
    for n in (0, 9):
        refused(api.pilot_train_step_ex(hd, pf, pq, py, n, None), -1, "n must be in [1, n_envs]")
    assert api.pilot_train_step_ex(hd, pf, pq, py, 8, None) == 0
    refused(api.pilot_train_debug_side(hd, 7, w1.ctypes.data, 8), -1, "unknown item")
    refused(api.pilot_train_debug_side(hd, 32, w1.ctypes.data, 8), -1, "unknown item")
    refused(api.pilot_train_debug_side(hd, 0, w1.ctypes.data, 7), -1, "size mismatch")
    refused(api.pilot_train_debug(hd, 35, w1.ctypes.data, 1), -1, "unknown item")
    env.step_pilot(2, {"model_type": KIND})                                          # the closed loop drives between steps, with the current weights
    assert api.pilot_train_step_ex(hd, pf, pq, py, 5, None) == 0
    env.pilot_train_end()
    env.pilot_load(plain)
    with pytest.raises(ValueError, match="layers must come from"):
        env.train_config(layers=("feature1",))                                       # the branch's names belong to a 28-array pilot


# ---- it learns --------------------------------------------------------------------------------------------------------------------------------
# The device's validation loss after the last epoch against the PyTorch fp32 mirror's, measured once on an MI355X (profiles/r37_train_side.txt): MIRROR_GAP is the
# relative gap |device - mirror| / mirror found there, and the margin is one plus twice it, as in tests/test_train_gpu.py.
MIRROR_GAP = 0.00848                            # device 0.031769 against the mirror's 0.032040 after 8 epochs (from 0.128822 and 0.128820)
MARGIN = 1.0 + 2.0 * MIRROR_GAP


def redrawn_side_fixture(seed=2024):
    """The trained fixture pilot's convolutions with a 28-array tail drawn anew (Glorot uniform kernels, zero biases: Keras's initialisers)"""
    from test_pilot_trained import trained_weights
    ws = list(trained_weights()[:14])
    rng = np.random.default_rng(seed)
    F = trained_weights()[14].shape[0]
    for a, b in ((F + 16, 100), (100, 50), (50, 25), (25, 2), (1, 4), (4, 8), (8, 16)):
        ws += [R.glorot(rng, a, b), np.zeros(b, f32)]
    return ws


def mirror_fit_side(ds, ws, epochs, batch):
    """tests/test_train_gpu.py's mirror_fit with the branch: the same network behind conv7 in PyTorch fp32 on the same GPU (frozen fp32 convolutions, the
    features taken once), the same 14 initial arrays, the same batches in the same order, 'mse' and Adam in Keras's form.  Returns the validation loss before
    training and per epoch."""
    import torch
    import torch.nn.functional as Fn
    from test_pilot import SPEC
    dev = ds.device
    with torch.no_grad():
        feats = []
        for a in range(0, len(ds), 128):
            x = ds.frames[a:a + 128].float().div(255.0).permute(0, 3, 1, 2)
            for i, (k, s, cin, cout) in enumerate(SPEC):
                wk = torch.from_numpy(ws[2 * i]).to(dev).permute(3, 2, 0, 1).contiguous()
                x = Fn.relu(Fn.conv2d(x, wk, torch.from_numpy(ws[2 * i + 1]).to(dev), stride=s))
            feats.append(x.permute(0, 2, 3, 1).reshape(x.shape[0], -1))
        X = torch.cat(feats)
    Y, S20 = torch.zeros((len(ds), 2), device=dev), torch.zeros((len(ds), 1), device=dev)
    for split, count in (("train", ds.n_train), ("val", ds.n_val)):                          # features and labels of every record, by the loader's own rule
        for _, fin, labels in ds.batches(count, 0, split, layout="nhwc", dtype="uint8"):
            idx = torch.as_tensor(ds.order(split, 0).astype(np.int64), device=dev)
            Y[idx], S20[idx] = labels, fin
    P = [torch.from_numpy(ws[14 + j].copy()).to(dev).requires_grad_(True) for j in range(14)]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]

    def model(x, s):
        for j in (4, 5, 6):
            s = Fn.relu(s @ P[2 * j] + P[2 * j + 1])
        z = torch.cat([x, s], 1)
        for j in range(4):
            z = z @ P[2 * j] + P[2 * j + 1]
            z = Fn.relu(z) if j < 3 else z
        return z

    val_idx = torch.as_tensor(ds.order("val", 0)[:ds.n_val // batch * batch].astype(np.int64), device=dev)

    def val_loss():
        with torch.no_grad():
            return float(((model(X[val_idx], S20[val_idx]).double() - Y[val_idx].double()) ** 2).mean().item())

    curve, t = [val_loss()], 0
    for epoch in range(epochs):
        order = torch.as_tensor(ds.order("train", epoch).astype(np.int64), device=dev)
        for b in range(ds.n_train // batch):
            idx = order[b * batch:(b + 1) * batch]
            loss = ((model(X[idx], S20[idx]) - Y[idx]) ** 2).sum() / (2 * batch)
            grads = torch.autograd.grad(loss, P)
            t += 1
            alpha = float(R.alpha_t(1e-3, 0.9, 0.999, t))
            with torch.no_grad():
                for p, g, m, v in zip(P, grads, M, V):
                    m.mul_(0.9).add_(g, alpha=1.0 - 0.9)
                    v.mul_(0.999).addcmul_(g, g, value=1.0 - 0.999)
                    p.sub_(alpha * m / (v.sqrt() + 1e-7))
        curve.append(val_loss())
    return curve


@pytest.mark.gpu
def test_it_learns(make_env):
    """tests/test_train_gpu.py's recipe with the speed_feature loader: 64 cars, the scripted expert, collect(ticks=120, every=5, skip=20): 1,280 records, 16
    training batches of 64 per epoch.  fit_tail for EPOCHS epochs from the fixture pilot's convolutions with a 28-array tail drawn anew, against the PyTorch
    fp32 mirror of the same run.  A speed_ctl set of the same records is refused."""
    t0 = time.perf_counter()
    ws = redrawn_side_fixture()
    env = make_env("hip", n_envs=64, img_h=120, img_w=160, auto_reset=True)
    env.set_expert()
    frames, rows = env.collect(ticks=120, every=5, skip=20)
    ds = env.dataset(frames, rows, loader="speed_feature", seed=7)
    assert len(ds) == 1280 and ds.n_train == 1024 and ds.n_val == 256
    env.pilot_load(ws)
    with pytest.raises(ValueError, match="speed_feature"):
        env.dataset(frames, rows, loader="speed_ctl", seed=7).fit_tail(1, BATCH)
    first = ds.pilot_loss("val", BATCH)
    history = ds.fit_tail(EPOCHS, BATCH)
    assert len(history) == EPOCHS
    last = history[-1][1]
    kept = ds.pilot_loss("val", BATCH)                                   # the best epoch's 14 arrays are in the handle
    assert kept == min(v for _, v in history)
    got = env.pilot_weights()
    assert len(got) == 28 and all(np.abs(got[14 + a] - ws[14 + a]).max() > 0 for a in range(14))     # every trained array moved, the branch's too
    mirror = mirror_fit_side(ds, ws, EPOCHS, BATCH)
    gap = abs(last - mirror[-1]) / mirror[-1]
    print(f"device: val loss {first:.6f} -> {last:.6f} (best {kept:.6f}), train losses {[round(a, 5) for a, _ in history]}, val {[round(v, 5) for _, v in history]}")
    print(f"mirror: val loss {mirror[0]:.6f} -> {mirror[-1]:.6f}, per epoch {[round(v, 5) for v in mirror[1:]]}; relative gap of the final losses {gap:.2e}; "
          f"{time.perf_counter() - t0:.2f} s")
    assert abs(first - mirror[0]) <= 1e-3 * mirror[0]                    # the same start
    assert mirror[-1] < 0.5 * mirror[0]                                  # the mirror learns too: the bound below is one on a trained network
    assert last < 0.5 * first
    assert last <= mirror[-1] * MARGIN, (last, mirror[-1], MARGIN)
