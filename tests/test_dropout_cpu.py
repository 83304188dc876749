"""Dropout behind conv7, without a GPU (include/trsim_spec.h, "training the pilot's tail, dropout"): a numpy restatement of the threshold T and the scale s of
a rate, the key chain and keep(), compared bit for bit with trs_train_dropout_keep and with the host-only rules of csrc/trsim_dropout.hpp under a stand-alone
sanitizer driver (tests/dropout_driver.cpp); what the flags depend on; the kept share; the restatement of the dropped forward and backward pass, built on
tests/test_train_cpu.py's, against torch.autograd in binary64 with the same masks as constants; the library's defaults and the refusals that need no device;
and the condition tests/test_dropout_gpu.py relies on: with the masks applied, the reference alone leaves at most CAP of the frames out.
tests/test_dropout_gpu.py imports the restatement and compares the kernels with it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import test_train_cpu as R
from conftest import ROOT
from triton_racer_sim_amd import _ffi

f32, u64 = np.float32, np.uint64
SALT = 0x64726F706F757421                                   # "dropout!"
WIDTHS = (None, 100, 50, 25)                                # units per frame at sites 1 .. 3 (site 0: F)
BELOW_ONE = float(np.nextafter(f32(1.0), f32(0.0)))         # the largest binary32 below 1
RATES = (0.0, 0.1, 0.5, 0.999, BELOW_ONE)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def mix(x):
    """mix of "training minibatches" on uint64 (arrays or scalars), arithmetic mod 2^64"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, u64) + u64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        return z ^ (z >> u64(31))


def threshold(rate):
    """T = floor((double)rate 65536), rate a binary32"""
    return int(math.floor(float(f32(rate)) * 65536.0))


def scale(T):
    """s = (float)(65536 / (65536 - T))"""
    return f32(65536.0 / (65536 - T))


def keep_flags(rate, seed, t, site, n, width):
    """bool[n][width]: unit k of frame slot i is kept at step t iff its 16-bit field is >= T"""
    T = threshold(rate)
    Dt = mix(mix(u64(seed) ^ u64(SALT)) ^ u64(t))
    key = mix(Dt ^ ((u64(site) << u64(32)) | np.arange(n, dtype=u64)))                       # [n]
    k = np.arange(width, dtype=u64)
    with np.errstate(over="ignore"):
        word = mix(key[:, None] + (k >> u64(2))[None, :])                                    # [n][width]: four units per word
    field = (word >> (u64(16) * (k & u64(3)))[None, :]) & u64(0xFFFF)
    return field >= u64(T)


def drop_x7(x7h, keep, s):
    """x7'[f] = keep ? binary16_rn(min((float)x7[f] s, 65504)) : +0"""
    x = (np.asarray(x7h, np.float16).astype(f32) * f32(s)).astype(f32)
    return np.where(keep, np.minimum(x, f32(65504.0)).astype(np.float16), np.float16(0.0))


def drop_act(z, keep, s):
    """a'(l) = keep ? f32(relu(z) s) : +0 from binary32 pre-activations: one rounding"""
    a = (np.maximum(np.asarray(z, f32), f32(0.0)) * f32(s)).astype(f32)
    return np.where(keep, a, f32(0.0))


def forward_masked(z1, P, keeps, s, dtype=np.float64):
    """(a1, z2, a2, z3, a3, out) of the dropped network behind z1; keeps = (keep1, keep2, keep3), s = (s1, s2, s3).  With every unit kept and s = 1 this is
    test_train_cpu.forward."""
    z1 = np.asarray(z1, dtype)
    a1 = np.maximum(z1, 0) * dtype(s[0]) * keeps[0]
    z2 = a1 @ P["w2"].astype(dtype) + P["b2"].astype(dtype)
    a2 = np.maximum(z2, 0) * dtype(s[1]) * keeps[1]
    z3 = a2 @ P["w3"].astype(dtype) + P["b3"].astype(dtype)
    a3 = np.maximum(z3, 0) * dtype(s[2]) * keeps[2]
    out = a3 @ P["w4"].astype(dtype) + P["b4"].astype(dtype)
    return a1, z2, a2, z3, a3, out


def backward_masked(z1, z2, z3, out, y, P, keeps, s):
    """loss and (delta1 .. delta4) of the dropped network through test_train_cpu.backward: delta(l) = ((W(l+1) delta(l+1)) s) . keep . [z(l) > 0] is the plain
    rule with W(l+1) s for W(l+1) and a pre-activation of -1 where the unit is dropped"""
    Ps = dict(P)
    for l in (1, 2, 3):
        Ps[f"w{l + 1}"] = P[f"w{l + 1}"].astype(np.float64) * float(s[l - 1])
    gate = [np.where(k, np.asarray(z, np.float64), -1.0) for k, z in zip(keeps, (z1, z2, z3))]
    return R.backward(gate[0], gate[1], gate[2], out, y, Ps)


def ones(n):
    return tuple(np.ones((n, w), bool) for w in WIDTHS[1:])


# ---- the draw against the library --------------------------------------------------------------------------------------------------------
def lib_keep(api, rate, seed, t, site, n, width, sites=0xF):
    cfg = _ffi.TrsDropoutConfig()
    api.default_dropout_config(C.byref(cfg))
    cfg.rate, cfg.seed, cfg.sites = rate, seed, sites
    out = np.full((n, width), 7, np.uint8)
    rc = api.train_dropout_keep(C.byref(cfg), t, site, n, width, out.ctypes.data)
    assert rc == 0, api.last_error()
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


def test_keep_matches_the_restatement_bit_for_bit(hip_api):
    for rate in RATES:
        for site, widths in ((0, (4608, 16640)), (1, (100,)), (2, (50,)), (3, (25,))):
            for width in widths:
                for t in (1, 2, 1000):
                    for n in (1, 70):
                        got = lib_keep(hip_api, rate, 5, t, site, n, width)
                        assert np.array_equal(got, keep_flags(rate, 5, t, site, n, width)), (rate, site, width, t, n)
    # widths that are no multiple of four, a seed with high bits, a late step
    for width in (1, 2, 3, 5, 25, 50, 101):
        assert np.array_equal(lib_keep(hip_api, 0.5, 0xFEDCBA9876543210, 2 ** 40, 3, 3, width), keep_flags(0.5, 0xFEDCBA9876543210, 2 ** 40, 3, 3, width))


def test_flags_depend_on_seed_step_site_slot_and_unit_alone(hip_api):
    base = lib_keep(hip_api, 0.1, 0, 1, 0, 70, 4608)
    assert np.array_equal(lib_keep(hip_api, 0.1, 0, 1, 0, 17, 4608), base[:17])                  # a batch of 70 has the batch of 17 as its prefix
    assert np.array_equal(lib_keep(hip_api, 0.1, 0, 1, 0, 70, 100), base[:, :100])               # and a narrower site's flags would be a prefix too
    assert np.array_equal(lib_keep(hip_api, 0.1, 0, 1, 0, 70, 4608, sites=0), base)              # cfg.sites is not consulted
    for other in (lib_keep(hip_api, 0.1, 1, 1, 0, 70, 4608), lib_keep(hip_api, 0.1, 0, 2, 0, 70, 4608), lib_keep(hip_api, 0.1, 0, 1, 1, 70, 4608)):
        assert 0.1 < (other != base).mean() < 0.3                                                 # seed, t, site: independent draws differ in 2 p (1 - p) = 0.18
    assert len({base[i].tobytes() for i in range(70)}) == 70                                     # every frame slot has its own mask


def test_rate_zero_keeps_everything_and_the_share_is_binomial(hip_api):
    assert lib_keep(hip_api, 0.0, 3, 1, 0, 70, 4608).all() and lib_keep(hip_api, 0.0, 3, 9, 2, 70, 50).all()
    assert threshold(0.0) == 0 and float(scale(0)) == 1.0
    T = threshold(0.1)
    assert T == 6553                                                                              # 0.1f is 0.100000001490116: 6553.6 and a little
    p, N = 1.0 - T / 65536.0, 70 * 4608
    share = float(lib_keep(hip_api, 0.1, 0, 1, 0, 70, 4608).mean())
    sd = math.sqrt(p * (1.0 - p) / N)
    print(f"kept share {share:.6f} against 1 - T / 65536 = {p:.6f}: {(share - p) / sd:+.2f} standard deviations")
    assert abs(share - p) <= 5.0 * sd
    assert share == 290315 / N                                                                    # deterministic: the observed figure


def test_threshold_and_scale_vectors():
    assert [threshold(r) for r in RATES] == [0, 6553, 32768, 65470, 65535]
    assert float(scale(32768)) == 2.0 and float(scale(65535)) == 65536.0
    assert R.bits_of(scale(6553)) == 0x3F8E3885
    for rate in RATES + (0.25, 0.3, 0.9, 1e-5, 2.0 ** -16, 2.0 ** -17):
        T = threshold(rate)
        assert 0 <= T <= 65535 and T / 65536.0 <= float(f32(rate)) < (T + 1) / 65536.0
        one = float(scale(T)) * (1.0 - T / 65536.0)                                                # s (1 - T / 65536) == 1 to one ulp of binary32
        assert abs(one - 1.0) <= 2.0 ** -23, (rate, one)


# ---- the dropped passes against autograd -------------------------------------------------------------------------------------------------
def test_all_kept_is_the_plain_restatement():
    rng = np.random.default_rng(1)
    P = R.small_tail(256, 4)
    z1 = rng.normal(0, 1, (5, 100))
    y = rng.uniform(-1, 1, (5, 2))
    a1, z2, a2, z3, a3, out = forward_masked(z1, P, ones(5), (1.0, 1.0, 1.0))
    z2r, z3r, outr = R.forward(z1, P)
    assert np.array_equal(z2, z2r) and np.array_equal(z3, z3r) and np.array_equal(out, outr)
    for a, b in zip(backward_masked(z1, z2, z3, out, y, P, ones(5), (1.0, 1.0, 1.0)), R.backward(z1, z2, z3, out, y, P)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("sites", [0xF, 0x1, 0x2, 0x4, 0x8, 0x6])
def test_dropped_restatement_matches_autograd_float64(sites):
    import torch
    F, n, rate, seed, t = 256, 5, 0.5, 9, 3
    rng = np.random.default_rng(3)
    P = R.small_tail(F, 4)
    x7 = np.maximum(rng.normal(0.0, 1.0, (n, F)), 0).astype(np.float16)
    y = rng.uniform(-1, 1, (n, 2))
    T = threshold(rate)
    on = [(sites >> j) & 1 for j in range(4)]
    keep = [keep_flags(rate, seed, t, j, n, F if j == 0 else WIDTHS[j]) if on[j] else np.ones((n, F if j == 0 else WIDTHS[j]), bool) for j in range(4)]
    s = [float(scale(T)) if on[j] else 1.0 for j in range(4)]
    assert all(0.3 < k.mean() < 0.7 for j, k in enumerate(keep) if on[j])
    x7d = drop_x7(x7, keep[0], s[0]).astype(np.float64)
    if on[0]:
        assert np.array_equal(x7d, x7.astype(np.float64) * 2.0 * keep[0])                          # rate 0.5: s = 2, exact in binary16 here
    Tn = {k: torch.tensor(P[k].astype(np.float64), requires_grad=True) for k in R.NAMES}
    K = [torch.tensor(k.astype(np.float64)) for k in keep]
    h = torch.tensor(x7d)
    a = h
    for l in (1, 2, 3):
        a = torch.relu(a @ Tn[f"w{l}"] + Tn[f"b{l}"]) * s[l] * K[l]
    out_t = a @ Tn["w4"] + Tn["b4"]
    loss_t = ((out_t - torch.tensor(y)) ** 2).sum() / (2 * n)
    loss_t.backward()
    z1 = x7d @ P["w1"].astype(np.float64) + P["b1"].astype(np.float64)
    a1, z2, a2, z3, a3, out = forward_masked(z1, P, keep[1:], s[1:])
    loss, d1, d2, d3, d4 = backward_masked(z1, z2, z3, out, y, P, keep[1:], s[1:])
    g = R.small_gradients(a1, a2, a3, d1, d2, d3, d4)                                             # relu(a') is a': the activations go where the pre-activations went
    g["w1"] = x7d.T @ d1
    assert abs(loss - float(loss_t.detach())) < 1e-13
    for k in R.NAMES:
        np.testing.assert_allclose(g[k], Tn[k].grad.numpy(), rtol=1e-11, atol=1e-14, err_msg=k)
    # the gradient at x7' (what G7 is before its gate) carries no s: the factor s of site 0 belongs to the step from x7' to x7
    h2 = torch.tensor(x7d, requires_grad=True)
    a = h2
    for l in (1, 2, 3):
        a = torch.relu(a @ Tn[f"w{l}"].detach() + Tn[f"b{l}"].detach()) * s[l] * K[l]
    (((a @ Tn["w4"].detach() + Tn["b4"].detach() - torch.tensor(y)) ** 2).sum() / (2 * n)).backward()
    np.testing.assert_allclose(d1 @ P["w1"].astype(np.float64).T, h2.grad.numpy(), rtol=1e-11, atol=1e-14)
    # and binary32 a' of the rule agrees with the binary64 one to one rounding
    a1f = drop_act(z1.astype(f32), keep[1], s[1])
    assert np.abs(a1f - np.maximum(z1.astype(f32).astype(np.float64), 0) * s[1] * keep[1]).max() <= 2.0 ** -24 * np.abs(a1f).max()


def test_site_zero_rule_vectors():
    x = np.array([0.0, 1.0, 0.333, 60000.0, 65504.0, 6e-8, 2.0 ** -14], np.float16)
    keep = np.array([1, 1, 1, 1, 0, 1, 1], bool)
    s = scale(threshold(0.1))
    got = drop_x7(x, keep, s)
    assert got[0] == 0 and got[4] == 0 and not np.signbit(got[4])
    assert float(got[3]) == 65504.0                                                                # 60000 s is beyond the range: the largest finite value
    assert float(got[1]) == float(np.float16(float(s)))
    assert (got[keep & (x > 0)] > 0).all()                                                         # a kept positive value stays positive: the gate carries the mask
    assert (got.astype(np.float64)[keep] >= x.astype(np.float64)[keep]).all()


# ---- the host-only rules under a sanitizer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drop_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dropout") / "dropout_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", ROOT, os.path.join(ROOT, "tests", "dropout_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.split()


def hexbits(x):
    return f"{R.bits_of(x):08x}"


def test_driver_defaults_and_refusals(drop_driver):
    assert run_driver(drop_driver, "defaults") == ["24", hexbits(0.1), "15", "0"]
    assert run_driver(drop_driver, "config") == ["ok"]


def test_driver_threshold_and_scale(drop_driver):
    rates = RATES + (0.25, 0.3, 0.9, 1e-5, 2.0 ** -16, 2.0 ** -17, -0.0)
    out = run_driver(drop_driver, "ts", *[hexbits(r) for r in rates])
    got = [(int(out[2 * i]), int(out[2 * i + 1], 16)) for i in range(len(rates))]
    assert got == [(threshold(r), R.bits_of(scale(threshold(r)))) for r in rates]


def test_driver_keep_against_the_restatement(drop_driver):
    for rate, seed, t, site, n, width in ((0.1, 0, 1, 0, 3, 4608), (0.5, 12345, 2, 1, 70, 100), (0.999, 2 ** 63 + 5, 1000, 2, 17, 50), (BELOW_ONE, 1, 7, 3, 5, 25),
                                          (0.0, 1, 1, 3, 2, 25), (0.3, 4, 3, 0, 2, 7), (0.1, 4, 3, 1, 0, 100)):
        lines = run_driver(drop_driver, "keep", hexbits(rate), seed, t, site, n, width)
        got = np.array([[c == "1" for c in line] for line in lines], bool).reshape(n, width)
        assert np.array_equal(got, keep_flags(rate, seed, t, site, n, width)), (rate, seed, t, site)


# ---- the library without a device ----------------------------------------------------------------------------------------------------------
def test_ffi_binds_the_dropout_symbols():
    assert _ffi.DROPOUT_SYMBOLS == ["default_dropout_config", "pilot_train_dropout", "train_dropout_keep"]
    assert all(s in _ffi.PILOT_SYMBOLS and s not in _ffi.SYMBOLS for s in _ffi.DROPOUT_SYMBOLS)
    assert (_ffi.TRAIN_DEBUG["a1"], _ffi.TRAIN_DEBUG["a2"], _ffi.TRAIN_DEBUG["a3"]) == (36, 37, 38)


def test_defaults_and_struct_size(hip_api):
    cfg = _ffi.TrsDropoutConfig()
    hip_api.default_dropout_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(_ffi.TrsDropoutConfig) == 24
    assert R.bits_of(cfg.rate) == R.bits_of(0.1) and cfg.sites == 0xF and cfg.seed == 0
    assert _ffi.TrsDropoutConfig.seed.offset == 16
    hip_api.default_dropout_config(None)                                                           # NULL is ignored
    assert np.array_equal(lib_keep(hip_api, 0.1, 0, 1, 1, 4, 100), keep_flags(0.1, 0, 1, 1, 4, 100))
    out = np.zeros((4, 100), np.uint8)                                                             # a NULL config: the defaults
    assert hip_api.train_dropout_keep(None, 1, 1, 4, 100, out.ctypes.data) == 0
    assert np.array_equal(out.astype(bool), keep_flags(0.1, 0, 1, 1, 4, 100))


def test_refusals_without_a_device(hip_api):
    def refused(rc, code, text):
        assert rc == code, (rc, hip_api.last_error())
        assert text in (hip_api.last_error() or b"").decode(), hip_api.last_error()

    def cfg(**kw):
        c = _ffi.TrsDropoutConfig()
        hip_api.default_dropout_config(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    out = np.zeros((2, 25), np.uint8)
    for kw, text in (({"struct_size": 8}, "struct_size"), ({"rate": 1.0}, "rate"), ({"rate": -0.5}, "rate"), ({"rate": float("nan")}, "rate"),
                     ({"rate": float("inf")}, "rate"), ({"sites": 0x10}, "sites"), ({"sites": 0x1F}, "sites")):
        refused(hip_api.pilot_train_dropout(None, C.byref(cfg(**kw))), -1, text)
        refused(hip_api.train_dropout_keep(C.byref(cfg(**kw)), 1, 3, 2, 25, out.ctypes.data), -1, text)
    refused(hip_api.pilot_train_dropout(None, None), -1, "null handle")
    refused(hip_api.pilot_train_dropout(None, C.byref(cfg())), -1, "null handle")
    ok = C.byref(cfg())
    refused(hip_api.train_dropout_keep(ok, 0, 3, 2, 25, out.ctypes.data), -1, "from 1")
    refused(hip_api.train_dropout_keep(ok, 1, 4, 2, 25, out.ctypes.data), -1, "site")
    refused(hip_api.train_dropout_keep(ok, 1, -1, 2, 25, out.ctypes.data), -1, "site")
    refused(hip_api.train_dropout_keep(ok, 1, 3, -1, 25, out.ctypes.data), -1, "out of range")
    refused(hip_api.train_dropout_keep(ok, 1, 3, 2, -1, out.ctypes.data), -1, "out of range")
    refused(hip_api.train_dropout_keep(ok, 1, 3, 2, 25, None), -1, "NULL")
    assert not out.any()                                                                           # nothing written by a refused call


# ---- the condition on the reference: the cap holds with the masks applied ------------------------------------------------------------------
def masked_reference(x7d, P, gps, keeps, s):
    """tests/test_train_gpu.py's pure_reference for the dropped network, from the dropped activation x7' alone: pre-activations, activations, their bounds
    (chain_bound over the activations the layer read), the frames to leave out"""
    import test_train_gpu as G
    z1, b1 = G.z1_reference(x7d, P, gps)
    a1, z2, a2, z3, a3, out = forward_masked(z1, P, keeps, s)
    b2 = G.chain_bound(a1, P["w2"], P["b2"], 100)
    b3 = G.chain_bound(a2, P["w3"], P["b3"], 50)
    near = (np.abs(z1) < 10 * b1).any(1) | (np.abs(z2) < 10 * b2).any(1) | (np.abs(z3) < 10 * b3).any(1)
    return {"z1": z1, "z2": z2, "z3": z3, "out": out, "a1": a1, "a2": a2, "a3": a3, "bound1": b1, "near": near}


# What tests/test_dropout_gpu.py trains with.  The seed is an input like the frames and the weights, and the cap is a condition on the reference alone: of
# seeds 0 .. 5 at step 1, seeds 1 and 5 keep it for every set of sites below at both frame sizes (seed 0 leaves 4 of the 70 frames out with site 1 on
# alone, one more than 5 %); the test below asserts it for the seed in use.
DROP_RATE, DROP_SEED = 0.1, 1
SITE_SETS = (0x1, 0x2, 0x4, 0x8, 0xE, 0xF)


def masks_for(sites, t, n, F, rate=DROP_RATE, seed=DROP_SEED):
    """(keep[4], s[4]) of a step: every unit kept and s = 1 at a site whose bit is clear"""
    T = threshold(rate)
    on = [bool((sites >> j) & 1) and T > 0 for j in range(4)]
    widths = (F, 100, 50, 25)
    keep = [keep_flags(rate, seed, t, j, n, widths[j]) if on[j] else np.ones((n, widths[j]), bool) for j in range(4)]
    return keep, [scale(T) if on[j] else f32(1.0) for j in range(4)]


from test_pilot_plan_cpu import driver                      # noqa: E402,F401  (a fixture)


@pytest.mark.parametrize("h,w,n,ksplit,sites", [(120, 160, 70, 0, m) for m in SITE_SETS] + [(130, 300, 37, 10, 0x1), (130, 300, 37, 10, 0xF)])
def test_the_reference_alone_keeps_the_cap_with_the_masks(driver, h, w, n, ksplit, sites):
    import test_train_gpu as G
    from test_pilot_plan_cpu import call_of
    from test_pilot_slices import slice_frames
    from test_pilot_types import conv_stack_pure
    named, F = G.tail_weights(h, w, seed=3)
    x7 = np.asarray(conv_stack_pure(slice_frames(h, w, n, seed=1), named), f32).astype(np.float16)
    call = call_of(driver, h, w, n, n, arrays=22, **({"ksplit": ksplit} if ksplit else {}))
    keep, s = masks_for(sites, 1, n, F)
    ref = masked_reference(drop_x7(x7, keep[0], s[0]), G.params_of(named), call["gps"], keep[1:], s[1:])
    active = float((ref["z1"] > 0).mean())
    print(f"{h}x{w}, {n} frames, sites {sites:#x}: {ref['near'].mean():.3f} of the frames left out, {active:.2f} of dense1's units active")
    assert ref["near"].mean() <= G.CAP
    assert 0.2 <= active <= 0.8
    assert 0.1 <= (ref["z2"] > 0).mean() <= 0.9 and 0.1 <= (ref["z3"] > 0).mean() <= 0.9
