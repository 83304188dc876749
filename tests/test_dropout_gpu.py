"""Dropout behind conv7 on the device (include/trsim_spec.h, "training the pilot's tail, dropout"; trs_train_drop7_kernel, trs_train_tail_drop_kernel and
trs_train_g7_drop_kernel) against the numpy restatement of tests/test_dropout_cpu.py.  The masks are the host's (trs_train_dropout_keep), compared bit for
bit with what the kernels did: the dropped x7 and the three a'(l) are exact rules.  Everything behind them is compared as tests/test_train_gpu.py compares a
plain step, from the values the kernel itself read, within that file's derived bounds.  Two bounds gain a term:
  delta(l), l = 1 .. 3, at a site that drops is fl(c s) for the chain c the plain kernel stores.  |fl(c s) - c s| <= 2^-24 |c s| (one rounding) and
  s |c - c_exact| <= s B, B the plain bound (terms + 1) 2^-24 sum |W delta|; with |c s| <= |ref| + s B the bound is s B + 2^-24 (|ref| + s B).  At a site
  that does not drop s = 1, the product is not taken and the bound is B as before.
  G7 takes s 2^-s1 where it took 2^-s1: the product of a binary32 and a power of two is exact, so the rounding count and tests/test_train_conv_gpu.py's bound
  stay, on a reference that carries the factor s.
The frames left out of the delta comparisons are the masked reference's (tests/test_dropout_cpu.py asserts the cap on the reference alone)."""
import ctypes as C
import time

import numpy as np
import pytest

import test_dropout_cpu as D
import test_train_conv_cpu as RC
import test_train_cpu as R
from test_dropout_cpu import DROP_RATE, DROP_SEED
from test_pilot import planner                                                              # noqa: F401  (a fixture)
from test_pilot_plan_cpu import call_of, driver                                             # noqa: F401  (driver is a fixture)
from test_pilot_slices import flatten_shape, slice_frames
from test_train_conv_gpu import ALL, LAYERS, ConvTrainer, halves
from test_train_gpu import BATCHES, CAP, SMALL, TAIL, WIDE, Trainer, U, bits, chain_bound, check_step, labels_for, params_of, tail_weights, worst, z1_reference
from triton_racer_sim_amd import _ffi

f32 = np.float32
SITES = _ffi.DROPOUT_SITES


def names_of(sites):
    return tuple(SITES[j] for j in range(4) if (sites >> j) & 1)


def drop_kw(sites=0xF, rate=DROP_RATE, seed=DROP_SEED):
    return {"dropout": rate, "dropout_sites": names_of(sites), "dropout_seed": seed}


def debug_of(tr, n):
    d = tr.debug(n)
    for l, w in ((1, 100), (2, 50), (3, 25)):
        d[f"a{l}"] = tr.env.pilot_train_debug(f"a{l}").reshape(n, w)
    return d


def host_masks(env, sites, t, n, F):
    """(keep[4], s[4]) of step t from the library's host flags, which are the restatement's"""
    keep, s = D.masks_for(sites, t, n, F)
    for j in range(4):
        if (sites >> j) & 1:
            assert np.array_equal(env.pilot_train_dropout_keep(t, j, n), keep[j]), (t, j)
    return keep, s


def half_bits(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def check_drop_step(P, y, d, gps, keep, s, tag):
    """One step's debug items against the dropped restatement; P: the weights the step read; keep, s: per site (every unit kept and 1 where it is off)"""
    n = len(y)
    x7, y64 = d["x7"], y.astype(np.float64)
    ref = D.masked_reference(x7, P, gps, keep[1:], s[1:])
    ok = ~ref["near"]
    W = {k: P[k].astype(np.float64) for k in ("w2", "w3", "w4")}
    ratios = {"z1": worst(d["z1"], ref["z1"], ref["bound1"])}
    for l in (1, 2, 3):                                                           # a'(l) = f32(relu(z_dev) s) . keep, bit for bit
        assert np.array_equal(bits(d[f"a{l}"]), bits(D.drop_act(d[f"z{l}"], keep[l], s[l]))), (tag, l)
    a1, a2, a3 = (d[k].astype(np.float64) for k in ("a1", "a2", "a3"))
    for k, a, l, terms in (("z2", a1, 2, 100), ("z3", a2, 3, 50), ("out", a3, 4, 25)):     # from the device's own a', chain_bound unchanged
        ratios[k] = worst(d[k], a @ W[f"w{l}"] + P[f"b{l}"].astype(np.float64), chain_bound(a, P[f"w{l}"], P[f"b{l}"], terms))
    out64 = d["out"].astype(np.float64)
    ratios["delta4"] = worst(d["delta4"], (out64 - y64) / n, 3 * U * (np.abs(out64) + np.abs(y64)) / n)
    dl = {l: d[f"delta{l}"].astype(np.float64) for l in (1, 2, 3, 4)}
    for l, terms in ((3, 2), (2, 25), (1, 50)):
        w = W[f"w{l + 1}"]
        sl = float(s[l])
        want = (dl[l + 1] @ w.T) * sl * (keep[l] & (ref[f"z{l}"] > 0))
        B = sl * (terms + 1) * U * (np.abs(dl[l + 1]) @ np.abs(w).T)
        bound = B + U * (np.abs(want) + B) if sl != 1.0 else B                     # the extra product's half ulp, where it is taken
        ratios[f"delta{l}"] = worst(d[f"delta{l}"], want, bound, ok)
        dropped = ~keep[l]
        assert not d[f"delta{l}"][dropped].any() and not d[f"a{l}"][dropped].any(), (tag, l)
    for l, a in ((2, a1), (3, a2), (4, a3)):
        ratios[f"gw{l}"] = worst(d[f"gw{l}"], a.T @ dl[l], (n + 1) * U * (np.abs(a).T @ np.abs(dl[l])))
    for l in (1, 2, 3, 4):
        ratios[f"gb{l}"] = worst(d[f"gb{l}"], dl[l].sum(0), (n + 1) * U * np.abs(dl[l]).sum(0))
    g_ref, tol, sexp = R.gw1_reference(x7, d["delta1"])
    assert d["s"] == sexp, (tag, d["s"], sexp)
    ratios["gw1"] = worst(d["gw1"], g_ref, tol)
    left = float(ref["near"].mean())
    print(f"{tag}: s = {sexp}, left out {left:.3f}; max |error| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)
    assert n < 20 or left <= CAP, (tag, left)
    return ref


# ---- 1. site 0 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,ksplit", [SMALL + (1, 0), SMALL + (17, 0), SMALL + (70, 0), WIDE + (37, 10)])
def test_site_zero_masks_x7_where_dense1_and_the_gw1_gemm_read_it(make_env, planner, h, w, n, ksplit):
    named, F = tail_weights(h, w, seed=3)
    P = params_of(named)
    frames, y = slice_frames(h, w, n, seed=1), labels_for(n, seed=n)
    call = planner.call(h, w, n, n, arrays=22, **({"ksplit": ksplit} if ksplit else {}))
    tr = Trainer(make_env, h, w, n, named, ksplit=ksplit, **drop_kw(0x1))
    fwd = tr.env.pilot_forward_host(frames)                                        # inference never drops
    x7 = tr.env.pilot_layer(6, (n,) + flatten_shape(h, w)).reshape(n, -1)
    tr.step(frames, y)
    d = debug_of(tr, n)
    keep, s = host_masks(tr.env, 0x1, 1, n, F)
    want = D.drop_x7(x7.astype(np.float16), keep[0], s[0])
    assert np.array_equal(half_bits(d["x7"]), half_bits(want)), int((half_bits(d["x7"]) != half_bits(want)).sum())
    assert 0.05 < (~keep[0]).mean() < 0.15 and (x7[~keep[0]] > 0).any()
    z1, b1 = z1_reference(d["x7"], P, call["gps"])
    assert worst(d["z1"], z1, b1) <= 1.0                                            # z1 of the dropped x7, within its existing bound
    assert not np.array_equal(bits(d["out"]), bits(fwd))
    check_step(P, y, d, call["gps"], f"{h}x{w} n = {n} site 0")                    # behind x7' the step is the plain one: the plain check, whole
    check_drop_step(P, y, d, call["gps"], keep, s, f"{h}x{w} n = {n} site 0 (dropped check)")


# ---- 2. sites 1 .. 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sites", [0x2, 0x4, 0x8, 0xE, 0xF], ids=["a1", "a2", "a3", "a1+a2+a3", "all"])
def test_the_dense_sites_one_at_a_time_and_together_at_every_batch_shape(make_env, planner, sites):
    t0 = time.perf_counter()
    h, w = SMALL
    named, F = tail_weights(h, w, seed=3)
    P = params_of(named)
    all_frames = slice_frames(h, w, max(BATCHES), seed=1)
    for n in BATCHES:
        frames, y = all_frames[:n], labels_for(n, seed=n)
        call = planner.call(h, w, n, n, arrays=22)
        tr = Trainer(make_env, h, w, n, named, **drop_kw(sites))
        fwd = tr.env.pilot_forward_host(frames)
        x7 = tr.env.pilot_layer(6, (n,) + flatten_shape(h, w)).reshape(n, -1)
        loss = tr.step(frames, y)
        d = debug_of(tr, n)
        keep, s = host_masks(tr.env, sites, 1, n, F)
        assert np.array_equal(half_bits(d["x7"]), half_bits(D.drop_x7(x7.astype(np.float16), keep[0], s[0]))), n
        assert abs(loss - float(((d["out"].astype(np.float64) - y) ** 2).sum() / (2 * n))) <= (2 * n + 1) * U * loss + 1e-12
        assert n == 1 or not np.array_equal(bits(d["out"]), bits(fwd))
        check_drop_step(P, y, d, call["gps"], keep, s, f"{h}x{w} n = {n} sites {sites:#x}")
    print(f"the six batch sizes took {time.perf_counter() - t0:.2f} s")


# ---- 3. off is the parent ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("convs", [None, ALL], ids=["tail", "convs"])
def test_rate_zero_no_sites_and_no_call_are_one_computation(make_env, convs):
    h, w = SMALL
    named, F = tail_weights(h, w, seed=3)
    frames = slice_frames(h, w, 34, seed=1)
    kws = ({}, {"dropout": 0.0, "dropout_seed": 5}, {"dropout": DROP_RATE, "dropout_sites": (), "dropout_seed": 5})
    trs = [ConvTrainer(make_env, h, w, 17, named, convs, **kw) for kw in kws]
    for t in (1, 2):
        sl, y = slice(17 * (t - 1), 17 * t), labels_for(17, seed=30 + t)
        states = []
        for tr in trs:
            fwd = tr.env.pilot_forward_host(frames[sl])
            tr.step(frames[sl], y)
            e = tr.env
            assert np.array_equal(bits(e.pilot_train_debug("out").reshape(17, 2)), bits(fwd)), t   # out equals trs_pilot_forward
            st = [e.pilot_train_debug(k) for k in ("gw1", "gb1", "gw2", "gb2", "gw3", "gb3", "gw4", "gb4", "delta1", "z1")]
            st += [e.pilot_train_debug(k, a) for k in ("m", "v") for a in range(8)] + list(e.pilot_train_weights()[0])
            for l in (1, 2, 3):                                                    # without dropout a(l) is relu(z(l))
                assert np.array_equal(bits(e.pilot_train_debug(f"a{l}")), bits(np.maximum(e.pilot_train_debug(f"z{l}"), 0))), (t, l)
            if convs:
                cs = tr.conv_state()
                st += [cs[nm][k] for nm in LAYERS for k in ("gw", "gb", "mw", "vw", "mb", "vb", "pack")] + list(e.pilot_train_conv_weights())
            states.append(st)
        for other in states[1:]:
            assert len(other) == len(states[0])
            for i, (a, b) in enumerate(zip(states[0], other)):
                assert np.array_equal(bits(a), bits(b)), (t, i)
        assert states[0][0].any()


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_handles_agree_another_seed_differs_and_every_step_draws_anew(make_env, planner):
    h, w = SMALL
    named, F = tail_weights(h, w, seed=3)
    frames = slice_frames(h, w, 48, seed=1)
    a, b, c = (Trainer(make_env, h, w, 16, named, **drop_kw(0xF, seed=sd)) for sd in (DROP_SEED, DROP_SEED, DROP_SEED + 1))
    for t in (1, 2, 3):
        sl, y = slice(16 * (t - 1), 16 * t), labels_for(16, seed=50 + t)
        la, lb, lc = (tr.step(frames[sl], y) for tr in (a, b, c))
        assert la == lb and la != lc
        keep, s = host_masks(a.env, 0xF, t, 16, F)
        for l in (1, 2, 3):                                                        # the masks of step t, not of step 1
            z = a.env.pilot_train_debug(f"z{l}").reshape(16, -1)
            assert np.array_equal(bits(a.env.pilot_train_debug(f"a{l}").reshape(16, -1)), bits(D.drop_act(z, keep[l], s[l]))), (t, l)
        if t > 1:
            prev, _ = D.masks_for(0xF, t - 1, 16, F)
            assert all(not np.array_equal(prev[j], keep[j]) for j in range(4))
    wa, wb, wc = (tr.env.pilot_train_weights()[0] for tr in (a, b, c))
    for x, y_, z in zip(wa, wb, wc):
        assert np.array_equal(bits(x), bits(y_)) and not np.array_equal(bits(x), bits(z))
    for x, y_ in zip(a.gradients() + sum(a.moments(), []), b.gradients() + sum(b.moments(), [])):
        assert np.array_equal(bits(x), bits(y_))


# ---- 5. with the convolutions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(96, 128), (120, 160)])
def test_delta7_takes_the_dropped_x7_as_gate_and_the_factor_s(make_env, h, w):
    n = 17
    named, F = tail_weights(h, w, seed=3)
    frames, y = slice_frames(h, w, n, seed=1), labels_for(n, seed=n)
    tr = ConvTrainer(make_env, h, w, n, named, ALL, lr=2e-3, **drop_kw(0xF))
    e = tr.env
    e.pilot_forward_host(frames)
    shape7 = tr.shape(4, n)
    x7 = e.pilot_layer(6, shape7).reshape(n, -1)
    tr.step(frames, y)
    keep, s = host_masks(e, 0xF, 1, n, F)
    x7d = e.pilot_layer(6, shape7).reshape(n, -1)
    assert np.array_equal(half_bits(x7d), half_bits(D.drop_x7(x7.astype(np.float16), keep[0], s[0])))
    d1, s1 = e.pilot_train_debug("delta1").reshape(n, 100), int(e.pilot_train_debug("scale_exp")[0])
    q1 = R.quantise(d1, s1).astype(np.float64)
    w1h = halves(named)["dense1"]
    G = RC.g7(x7d, w1h, q1, s1) * float(s[0])                                      # the gate is the dropped x7': it carries the mask
    G_abs = RC.g7_abs(w1h, q1, s1) * float(s[0])
    s7 = int(e.pilot_train_debug_conv("conv7", "scale_exp")[0])
    assert s7 == RC.scale_of(G), (s7, RC.scale_of(G))
    delta = e.pilot_train_debug_conv("conv7", "delta").reshape(n, -1).astype(np.float64)
    ratio = worst(delta, G, RC.stored_bound(G, G_abs, 128, s7))
    plain = worst(delta, G / float(s[0]), RC.stored_bound(G, G_abs, 128, s7))
    print(f"{h}x{w}: delta7 max |error| / bound {ratio:.3f} (without the factor s it would be {plain:.0f})")
    assert ratio <= 1.0 and plain > 10.0
    assert not delta[~keep[0]].any() and delta.any()
    # Adam, t = 1, bit for bit from the device's gradient: the convolutions and the tail
    st, masters = tr.conv_state(), e.pilot_train_conv_weights()
    for j, nm in enumerate(LAYERS):
        for k, (gk, mk, vk) in enumerate((("gw", "mw", "vw"), ("gb", "mb", "vb"))):
            prev = np.asarray(named[nm][k], f32).ravel()
            m, v, wn = R.adam(st[nm][gk], np.zeros_like(prev), np.zeros_like(prev), prev, 1, lr=2e-3)
            for got, ref in ((st[nm][mk], m), (st[nm][vk], v), (masters[2 * j + k].ravel(), wn)):
                assert np.array_equal(bits(got), bits(ref)), (nm, gk)
            assert st[nm][gk].any()
    g, (m, v), (tail, steps) = tr_gradients(e), tr_moments(e), e.pilot_train_weights()
    assert steps == 1
    for a in range(8):
        prev = np.asarray(named[TAIL[a // 2]][a % 2], f32).ravel()
        want = R.adam(g[a], np.zeros_like(prev), np.zeros_like(prev), prev, 1, lr=2e-3)
        for got, ref in zip((m[a], v[a], tail[a].ravel()), want):
            assert np.array_equal(bits(got), bits(ref)), R.NAMES[a]


def tr_gradients(e):
    return [e.pilot_train_debug(k).copy() for k in ("gw1", "gb1", "gw2", "gb2", "gw3", "gb3", "gw4", "gb4")]


def tr_moments(e):
    return [e.pilot_train_debug("m", a).copy() for a in range(8)], [e.pilot_train_debug("v", a).copy() for a in range(8)]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_on_the_device(make_env):
    h, w = SMALL
    named, F = tail_weights(h, w, seed=3)
    env = make_env("hip", n_envs=4, img_h=h, img_w=w)
    api, hd = env.api, env._h
    cfg = env.dropout_config(0.1)

    def refused(rc, code, text):
        assert rc == code, (rc, api.last_error())
        assert text in (api.last_error() or b"").decode(), api.last_error()

    refused(api.pilot_train_dropout(hd, C.byref(cfg)), -2, "no pilot loaded")
    env.pilot_load(named)
    refused(api.pilot_train_dropout(hd, C.byref(cfg)), -2, "trs_pilot_train_begin first")
    env.pilot_train_begin()
    bad = env.dropout_config(0.1)
    bad.sites = 0x10
    refused(api.pilot_train_dropout(hd, C.byref(bad)), -1, "sites")
    assert api.pilot_train_dropout(hd, C.byref(cfg)) == 0
    refused(api.pilot_train_dropout(hd, C.byref(cfg)), -2, "already called")
    env.pilot_train_end()
    env.pilot_train_begin()
    d_frames, d_y = env.scratch(20, (4, h, w, 3), np.uint8), env.scratch(21, (4, 2), np.float32)
    env.upload(d_frames, slice_frames(h, w, 4, seed=1)); env.upload(d_y, labels_for(4, 1))
    env.pilot_train_step(d_frames, d_y, 4)
    refused(api.pilot_train_dropout(hd, C.byref(cfg)), -2, "before the session's first step")
    refused(api.pilot_train_dropout(hd, None), -2, "before the session's first step")
    env.pilot_train_end()
    with pytest.raises(RuntimeError, match="rate"):
        env.pilot_train_begin(dropout=1.0)
    refused(api.pilot_train_end(hd), -2, "trs_pilot_train_begin first")              # no half-open session behind the refusal
    with pytest.raises(ValueError, match="dropout_sites"):
        env.pilot_train_begin(dropout=0.1, dropout_sites=("conv6",))
    env.pilot_train_begin(dropout=0.1)                                              # NULL-free path through the wrapper, and a session opens again
    env.pilot_train_end()


# ---- 7. the loop -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("alias", [False, True], ids=["fit_tail", "fit"])
def test_a_fit_with_dropout_equals_the_fit_driven_by_hand(make_env, alias):
    import test_fit_gpu as FG
    h, w = FG.SMALLEST
    epochs, batch = 2, FG.CARS                                                     # 160 training records: six batches of 24, 16 left over
    frames, rows = FG.noisy_set(h, w)
    loaded = FG.loaded_weights(h, w)
    convs = FG.ALL_CONVS if alias else None
    kw = dict(lr=FG.LR, dropout=DROP_RATE, dropout_seed=DROP_SEED)
    twin = FG.fresh(make_env, h, w, loaded)
    twin_history, twin_weights = FG.hand_fit(twin, frames, rows, epochs, batch, convs=convs, **kw)
    plain = FG.fresh(make_env, h, w, loaded)
    plain_history, _ = FG.hand_fit(plain, frames, rows, 1, batch, convs=convs, lr=FG.LR)
    assert plain_history[0][0] != twin_history[0][0]                               # (the dropout reached the step)
    epochs_run, best = FG.can_tell([v for _, v in twin_history], epochs, None, False)
    env = FG.fresh(make_env, h, w, loaded)
    ds = env.dataset(*FG.writable(frames, rows), seed=FG.SEED)
    history = ds.fit(epochs, batch, **kw) if alias else ds.fit_tail(epochs, batch, **kw)
    FG.compare(make_env, env, loaded, history, twin_history, twin_weights, epochs_run, best, FG.RECORDS, batch, None, FG.trained_arrays(convs, None), frames[:8])
    assert ds.pilot_loss("val") == history[best][1]                                # the validation loss is taken without dropout: a plain pilot_loss gives it


# ---- 8. it learns ------------------------------------------------------------------------------------------------------------------------------
EPOCHS, BATCH = 8, 64
# The device's validation loss after the last epoch against the PyTorch fp32 mirror's under the same masks, measured once (profiles/r36_dropout.txt):
# MIRROR_GAP is the relative gap |device - mirror| / mirror found there, and the margin is one plus twice it, as tests/test_train_gpu.py sets its own.
MIRROR_GAP = 0.0492                             # device 0.001520 against the mirror's 0.001599 after 8 epochs (the first GPU run of this test)
MARGIN = 1.0 + 2.0 * MIRROR_GAP


def mirror_fit_dropped(ds, ws, epochs, batch, keep_of, s):
    """tests/test_train_gpu.py's mirror_fit with the masks of the device's run as constants: site 0 on the fp32 features, sites 1 .. 3 behind the ReLUs, in
    the training steps alone.  keep_of(t, site) -> bool[batch][width]."""
    import torch
    import torch.nn.functional as Fn
    from test_pilot import SPEC
    dev = ds.device
    with torch.no_grad():
        feats = []
        for a in range(0, len(ds), 128):
            x = ds.frames[a:a + 128].float().div(255.0).permute(0, 3, 1, 2)
            for i, (k, st, cin, cout) in enumerate(SPEC):
                wk = torch.from_numpy(ws[2 * i]).to(dev).permute(3, 2, 0, 1).contiguous()
                x = Fn.relu(Fn.conv2d(x, wk, torch.from_numpy(ws[2 * i + 1]).to(dev), stride=st))
            feats.append(x.permute(0, 2, 3, 1).reshape(x.shape[0], -1))
        X = torch.cat(feats)
    Y = torch.zeros((len(ds), 2), device=dev)
    for split, count in (("train", ds.n_train), ("val", ds.n_val)):
        for _, _, labels in ds.batches(count, 0, split, layout="nhwc", dtype="uint8"):
            Y[torch.as_tensor(ds.order(split, 0).astype(np.int64), device=dev)] = labels
    P = [torch.from_numpy(ws[14 + j].copy()).to(dev).requires_grad_(True) for j in range(8)]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]

    def model(x, masks=None):
        z = x if masks is None else x * s * masks[0]
        for j in range(4):
            z = z @ P[2 * j] + P[2 * j + 1]
            if j < 3:
                z = Fn.relu(z) if masks is None else Fn.relu(z) * s * masks[j + 1]
        return z

    val_idx = torch.as_tensor(ds.order("val", 0)[:ds.n_val // batch * batch].astype(np.int64), device=dev)

    def val_loss():
        with torch.no_grad():
            return float(((model(X[val_idx]).double() - Y[val_idx].double()) ** 2).mean().item())

    curve, t = [val_loss()], 0
    for epoch in range(epochs):
        order = torch.as_tensor(ds.order("train", epoch).astype(np.int64), device=dev)
        for b in range(ds.n_train // batch):
            idx = order[b * batch:(b + 1) * batch]
            t += 1
            masks = [torch.as_tensor(keep_of(t, j), dtype=torch.float32, device=dev) for j in range(4)]
            loss = ((model(X[idx], masks) - Y[idx]) ** 2).sum() / (2 * batch)
            grads = torch.autograd.grad(loss, P)
            alpha = float(R.alpha_t(1e-3, 0.9, 0.999, t))
            with torch.no_grad():
                for p, g, m, v in zip(P, grads, M, V):
                    m.mul_(0.9).add_(g, alpha=1.0 - 0.9)
                    v.mul_(0.999).addcmul_(g, g, value=1.0 - 0.999)
                    p.sub_(alpha * m / (v.sqrt() + 1e-7))
        curve.append(val_loss())
    return curve


@pytest.mark.gpu
def test_it_learns_with_dropout(make_env):
    """tests/test_train_gpu.py's fixture and run (1,280 records, 16 training batches of 64 per epoch, EPOCHS epochs from the fixture pilot with its dense layers
    drawn again) at rate 0.1 on all four sites, against the PyTorch fp32 mirror fed the same masks."""
    from test_train_gpu import redrawn_fixture
    t0 = time.perf_counter()
    ws = redrawn_fixture()
    env = make_env("hip", n_envs=64, img_h=120, img_w=160, auto_reset=True)
    env.set_expert()
    frames, rows = env.collect(ticks=120, every=5, skip=20)
    ds = env.dataset(frames, rows, loader="speed_ctl", seed=7)
    assert len(ds) == 1280 and ds.n_train == 1024 and ds.n_val == 256
    env.pilot_load(ws)
    first = ds.pilot_loss("val", BATCH)
    history = ds.fit_tail(EPOCHS, BATCH, dropout=DROP_RATE, dropout_seed=DROP_SEED)
    assert len(history) == EPOCHS
    last = history[-1][1]
    kept = ds.pilot_loss("val", BATCH)
    assert kept == min(v for _, v in history)
    s = float(D.scale(D.threshold(DROP_RATE)))
    mirror = mirror_fit_dropped(ds, ws, EPOCHS, BATCH, lambda t, j: env.pilot_train_dropout_keep(t, j, BATCH, rate=DROP_RATE, seed=DROP_SEED), s)
    gap = abs(last - mirror[-1]) / mirror[-1]
    print(f"device: val loss {first:.6f} -> {last:.6f} (best {kept:.6f}), train losses {[round(a, 5) for a, _ in history]}, val {[round(v, 5) for _, v in history]}")
    print(f"mirror: val loss {mirror[0]:.6f} -> {mirror[-1]:.6f}, per epoch {[round(v, 5) for v in mirror[1:]]}; relative gap of the final losses {gap:.4e}; "
          f"{time.perf_counter() - t0:.2f} s")
    assert abs(first - mirror[0]) <= 1e-3 * mirror[0]                              # the same start
    assert mirror[-1] < 0.25 * mirror[0]                                           # the bound below has room
    assert last < 0.5 * first
    assert last <= mirror[-1] * MARGIN, (last, mirror[-1], MARGIN)
