"""The pilot's split-K slabs at every slice shape, through the kernels that add them: trs_pilot_dense_kernel writes one fp32 slab per K slice of dense1 (and of
dense4, the second head of cnn_2d_full_house); trs_pilot_tail_kernel adds them in padded groups of 8 (KS <= 8) or 16, trs_pilot_tail_ex_kernel in whole groups
of 8 and a scalar remainder loop, once per head.  The other pilot tests reach KS = 8 and 123 only, and dense1 alone through a getter that adds the slabs on the
host; here trs_pilot_tuning.ksplit forces KS = 1, 3, 6, 8, 10, 15, 29 at 130x300 for all three model types (sweep 1), and 150 frames of 240x320 run dense1 and
dense4 on trs_pilot_dense_kernel<2> with KS = 62, then 40 frames (KS = 123) and another tuning on the same handle (sweep 2).  The planner says which shapes a case
reaches, and the cases assert it.

The reference: everything behind conv7 on the kernel's own conv7 activation, pilot_layer(6).  The flatten rows of dense1 / dense4 and the activation are rounded
to fp16 (what the matrix cores multiply: the products are exact in binary32), their sums are taken in binary64, the rest is tests/test_pilot_types.py's
torch_heads in fp32.  Nothing of it comes from pilot_layer(7) or from the call under test.  Tolerances are the project's: 5e-4 against this reference
(tests/test_pilot_types.py), 1e-4 between two summation orders of the same products (tests/test_pilot.py).

Two conditions make those figures mean something, checked on the CPU (PyTorch's conv stack as conv7) and again on the GPU on the kernel's activation:
  * a reference with ONE slice's K range left out, or counted twice, differs from the right one by >= 5e-3 (10 x the tolerance) in some output of some frame:
    every slice of every case, both heads.  Glorot weights do not get there (dense1's sums are ~0.03 on these frames and its bias decides the ReLUs), so the
    flatten rows are scaled up (FLATTEN_GAIN): sums of order 1, of which a slice is a visible part, and outputs of order 1.  max |reference| <= 4.
  * the reference itself, accumulated in binary32 slice by slice in slice order instead of binary64, moves by no more than 1/8 of either tolerance (the
    headroom covers the MFMA's order inside a slice too).  Measured figures: profiles/r30_pilot_tail_slices.txt.
The frames are coarse random patterns with a gain per frame, not noise, so that a slab row read at another frame's offset does not pass: of all pairs of
frames fewer than 1 % have outputs within 2 x 5e-4 of each other, where one could stand for the other (asserted)."""
import time

import numpy as np
import pytest

from test_pilot import pilot_postprocess, planner                                           # noqa: F401  (planner is a fixture)
from test_pilot_plan_cpu import SPEC, call_of, driver                                       # noqa: F401  (driver is a fixture)
from test_pilot_types import conv_stack_pure, make_named_weights, torch_heads

KINDS = ["cnn_2d_speed_control", "cnn_2d_speed_as_feature", "cnn_2d_full_house"]
ARRAYS = {"cnn_2d_speed_control": 22, "cnn_2d_speed_as_feature": 28, "cnn_2d_full_house": 42}
KSPLITS = (1, 3, 6, 8, 10, 15, 29)
SWEEP1 = (130, 300, 37)                       # G = 2080 granules = 29 LDS chunks, the last of 64 granules; two frame groups of 32, ten tail workgroups
SWEEP2 = (240, 320, 150)                      # G = 8816 = 123 chunks, the last of 32; three frame groups of 64
CHUNK = 72                                    # granules (of 8 fp16 values) per LDS chunk of trs_pilot_dense_kernel: a slice is whole chunks
TOL_REF, TOL_ORDER, SENSITIVITY = 5e-4, 1e-4, 5e-3
FLATTEN_GAIN = 40.0                           # on the Glorot flatten rows of dense1 / dense4: chosen on the CPU so that the outputs are of order 1
NO_MISTAKE = "the cases no longer reach the kernels their docstrings name"


def flatten_shape(h, w):
    for k, s, _, _ in SPEC:
        h, w = (h - k) // s + 1, (w - k) // s + 1
    return h, w, 128


def slice_frames(h, w, n, seed):
    """Coarse random colour patterns (5 x 10 cells) under a gain per frame and fine noise: frames that differ from each other as a whole."""
    rng = np.random.default_rng(seed)
    cells = np.kron(rng.uniform(0.0, 1.0, (n, 5, 10, 3)), np.ones((1, -(-h // 5), -(-w // 10), 1)))[:, :h, :w]
    gain = rng.uniform(0.3, 1.0, (n, 1, 1, 1))
    return (255.0 * cells * gain * rng.uniform(0.6, 1.0, (n, h, w, 3))).astype(np.uint8)


def slice_weights(h, w, kind, seed):
    """make_named_weights with the flatten rows of dense1 / dense4 scaled up: dense1's sums, ~0.03 with Glorot rows on these frames, become of order 1, and
    the Glorot layers behind carry that to the outputs."""
    named, F = make_named_weights(h, w, kind, seed=seed)
    for nm in heads_of(kind):
        named[nm][0][:F] *= np.float32(FLATTEN_GAIN)
    return named, F


def side_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 20, n).astype(np.float32), rng.uniform(0, 10, n).astype(np.float32)


def heads_of(kind):
    return ("dense1", "dense4") if kind == "cnn_2d_full_house" else ("dense1",)


def chunk_products(x7, named, kind):
    """{head: float64[chunks][n][100]}: per LDS chunk of 72 granules the products of the fp16-rounded activation with the fp16-rounded flatten rows, summed
    in binary64.  Every K slice is a run of whole chunks, so every slice's partial sum is a sum of these."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(x7, dtype=np.float32)).half().double()
    F, step = x.shape[1], CHUNK * 8
    out = {}
    for nm in heads_of(kind):
        k = torch.from_numpy(named[nm][0][:F]).half().double()
        out[nm] = np.stack([(x[:, a:a + step] @ k[a:a + step]).numpy() for a in range(0, F, step)])
    return out


def slice_sums(chunks, gps):
    """float64[KS][n][100]: the partial sums of the K slices [s gps, min(G, (s + 1) gps)) granules"""
    per = gps // CHUNK
    assert per * CHUNK == gps
    return np.stack([chunks[a:a + per].sum(0) for a in range(0, len(chunks), per)])


def reference(prods, speed, segment, named, kind, reps=1):
    """The two outputs from the products of the flatten, {head: [reps n][100]}; the side inputs are repeated to match."""
    flat = {nm: np.asarray(p, np.float32) for nm, p in prods.items()}
    return torch_heads(None, np.tile(speed, reps), np.tile(segment, reps), named, kind, flat=flat)


def wrong_references(sums, speed, segment, named, kind):
    """float32[heads][2][KS][n][2]: the outputs with slice s of one head left out ([0]) or counted twice ([1]), the other head right"""
    total = {nm: s.sum(0) for nm, s in sums.items()}
    n = len(speed)
    res = []
    for nm, s in sums.items():
        ks = len(s)
        per_sign = []
        for sign in (-1.0, 1.0):
            prods = {o: np.tile(total[o], (ks, 1)) for o in sums}
            prods[nm] = (total[nm][None] + sign * s).reshape(ks * n, 100)
            per_sign.append(reference(prods, speed, segment, named, kind, reps=ks).reshape(ks, n, 2))
        res.append(per_sign)
    return np.asarray(res)


def least_notice(sums, speed, segment, named, kind):
    """(max |right reference|, the smallest over heads, slices and {left out, twice} of max over frames and outputs of |wrong - right|, the right reference)"""
    right = reference({nm: s.sum(0) for nm, s in sums.items()}, speed, segment, named, kind)
    wrong = wrong_references(sums, speed, segment, named, kind)
    return float(np.abs(right).max()), float(np.abs(wrong - right).max(axis=(3, 4)).min()), right


def frames_alike(ref):
    """the share of the pairs of frames whose outputs lie within 2 x TOL_REF of each other in both outputs"""
    d = np.abs(ref[:, None, :] - ref[None, :, :]).max(2)[np.triu_indices(len(ref), 1)]
    return float(np.mean(d <= 2 * TOL_REF))


def float32_in_slice_order(x7, named, kind, gps):
    """{head: float32[n][100]}: the same products added as the kernels do at the coarsest level: every slice by itself in binary32, the slices in order in binary32"""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(x7, dtype=np.float32)).half().float()
    F, step = x.shape[1], gps * 8
    out = {}
    for nm in heads_of(kind):
        k = torch.from_numpy(named[nm][0][:F]).half().float()
        acc = torch.zeros(x.shape[0], 100)
        for a in range(0, F, step):
            acc = acc + x[:, a:a + step] @ k[a:a + step]
        out[nm] = acc.numpy()
    return out


# ---- on the CPU -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("arrays", [22, 28, 42])
def test_ksplit_gives_the_seven_slice_counts(driver, arrays, cus):
    h, w, n = SWEEP1
    calls = {ks: call_of(driver, h, w, n, n, cus=cus, arrays=arrays, ksplit=ks) for ks in KSPLITS}
    assert {ks: c["KS"] for ks, c in calls.items()} == {ks: ks for ks in KSPLITS}, NO_MISTAKE
    for ks, c in calls.items():
        assert (c["G"], c["nf"], c["groups"]) == (2080, 1, 2) and c["gps"] % CHUNK == 0, (ks, c)
        assert c["dense_grid"] == 2 * ((ks + 7) // 8) * 8
    assert 2080 - 2 * calls[3]["gps"] == 640 and 2080 % CHUNK == 64          # KS = 3: the last slice is the short one and ends in the ragged chunk


def test_sweep_2_plans_both_frame_groupings_on_one_handle(driver):
    h, w, n = SWEEP2
    big, small, plain = (call_of(driver, h, w, n, m, cus=256, arrays=42, **t) for m, t in ((n, {}), (40, {}), (n, {"dense": 2})))
    assert (big["G"], big["nf"], big["KS"], big["groups"]) == (8816, 2, 62, 3) and big["KS"] % 8 == 6          # 7 x 8 + 6 in the ex tail; the last group has 22 frames
    assert (small["nf"], small["KS"], small["groups"]) == (1, 123, 2)                                          # 15 x 8 + 3
    assert (plain["nf"], plain["KS"], plain["groups"]) == (1, 41, 5)                                           # 5 x 8 + 1
    assert small["KS"] * 40 < big["KS"] * n                                  # rows of a slab: the 40 frames fit what the first call reserved


@pytest.mark.parametrize("kind", KINDS)
def test_the_reference_notices_a_slice_left_out_or_counted_twice(driver, kind):
    """Sweep 1's reference on PyTorch's fp32 conv stack: the sensitivity condition for every slice of every slice count, outputs of order 1, frames that
    differ, side inputs that matter, and the distance between binary64 and slice-ordered binary32 accumulation against the two tolerances."""
    h, w, n = SWEEP1
    named, F = slice_weights(h, w, kind, seed=3)
    frames = slice_frames(h, w, n, seed=1)
    speed, segment = side_inputs(n, seed=2)
    x7 = conv_stack_pure(frames, named)
    assert x7.shape == (n, F) and F == 2080 * 8
    chunks = chunk_products(x7, named, kind)
    worst = 0.0
    for ks in KSPLITS:
        gps = call_of(driver, h, w, n, n, arrays=ARRAYS[kind], ksplit=ks)["gps"]
        sums = {nm: slice_sums(c, gps) for nm, c in chunks.items()}
        assert all(len(s) == ks for s in sums.values())
        top, least, right = least_notice(sums, speed, segment, named, kind)
        f32 = reference(float32_in_slice_order(x7, named, kind, gps), speed, segment, named, kind)
        worst = max(worst, float(np.abs(f32 - right).max()))
        print(f"{kind} KS {ks}: max |reference| {top:.3f}, a slice left out or doubled moves it by >= {least:.3e}, binary32 in slice order - binary64 {np.abs(f32 - right).max():.2e}")
        assert top <= 4.0, (ks, top)
        assert least >= SENSITIVITY, (ks, least)
    assert 8 * worst <= TOL_ORDER < TOL_REF, worst
    assert frames_alike(right) < 0.01, frames_alike(right)
    if kind != "cnn_2d_speed_control":
        other = reference({nm: s.sum(0) for nm, s in sums.items()}, speed[::-1].copy(), segment[::-1].copy(), named, kind)
        assert np.abs(other - right).max() > 10 * 1e-3


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------

def forward(env, kind, frames, speed, segment):
    return env.pilot_forward_host(frames, speed=None if kind == "cnn_2d_speed_control" else speed, segment=segment if kind == "cnn_2d_full_house" else None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_every_slice_count_through_both_tails(make_env, planner, kind):
    """Sweep 1.  KS = 1: a single slab; 3, 6: a padded group of 8 in trs_pilot_tail_kernel, the remainder loop alone in trs_pilot_tail_ex_kernel (at 3 the last
    slice is shorter and ends in the ragged chunk); 8: one whole group; 10, 15: a padded group of 16, 8 + 2 and 8 + 7; 29: 16 + 13, 3 x 8 + 5.  One handle, reloaded
    per slice count.  37 frames: two frame groups, the second of 5; ten tail workgroups, the last with one live wave."""
    from triton_racer_sim_amd.env import SLOT_JPEG_IN, SLOT_PILOT_IN
    t0 = time.perf_counter()
    h, w, n = SWEEP1
    named, F = slice_weights(h, w, kind, seed=3)
    frames = slice_frames(h, w, n, seed=1)
    speed, segment = side_inputs(n, seed=2)
    calls = {ks: planner.call(h, w, n, n, arrays=ARRAYS[kind], ksplit=ks) for ks in KSPLITS}
    assert sorted(c["KS"] for c in calls.values()) == list(KSPLITS) and all(c["nf"] == 1 and c["groups"] == 2 for c in calls.values()), NO_MISTAKE
    env = make_env("hip", n_envs=n, img_h=h, img_w=w)
    outs, x7, chunks, base6 = {}, None, None, None
    for ks in (29, 1, 3, 6, 8, 10, 15):
        env.pilot_tuning(ksplit=ks)
        env.pilot_load(named)                                                # the choice is read when the weights are loaded
        out = forward(env, kind, frames, speed, segment)
        l6 = env.pilot_layer(6, (n,) + flatten_shape(h, w))
        if x7 is None:
            base6, x7 = l6, l6.reshape(n, -1)
            assert x7.shape[1] == F
            chunks = chunk_products(x7, named, kind)                         # the reference's sums: once per model type
        assert np.array_equal(l6.view(np.uint32), base6.view(np.uint32)), ks
        sums = {nm: slice_sums(c, calls[ks]["gps"]) for nm, c in chunks.items()}
        assert all(len(s) == calls[ks]["KS"] == ks for s in sums.values())
        top, least, right = least_notice(sums, speed, segment, named, kind)
        assert top <= 4.0 and least >= SENSITIVITY, (ks, top, least)
        assert frames_alike(right) < 0.01
        dev = float(np.abs(out - right).max())
        outs[ks] = out
        order = float(np.abs(out - outs[29]).max())
        print(f"{kind} KS {ks}: max |reference| {top:.3f}, least notice {least:.3e}, max |HIP - reference| {dev:.2e}, max |HIP - HIP at KS 29| {order:.2e}")
        assert dev <= TOL_REF, (ks, dev)
        assert order <= TOL_ORDER, (ks, order)
        again = forward(env, kind, frames, speed, segment)
        assert np.array_equal(again.view(np.uint32), out.view(np.uint32)), ks
        if kind != "cnn_2d_speed_control":                                   # the side inputs are read at every slice count
            other = forward(env, kind, frames, speed[::-1].copy(), segment[::-1].copy())
            assert np.abs(other - out).max() > 1e-3, ks

    # KerasPilot.step on the device at KS = 15 (the handle's last load): the slab sums reach the controls as well
    cfg = {"model_type": kind}
    raw, act_speed = outs[15], speed
    if kind != "cnn_2d_speed_as_feature":
        # the speed head reads no speed: speeds chosen from its output put the throttle at full, small, in the (-0.2, 0) dead zone and in reverse
        delta = np.resize(np.array([3.0, 0.05, -0.08, -3.0]), n)
        act_speed = (raw[:, 1].astype(np.float64) * 20 * 1.1 - delta).astype(np.float32)
        if kind == "cnn_2d_full_house":
            raw = forward(env, kind, frames, act_speed, segment)
            assert np.array_equal(raw[:, 1].view(np.uint32), outs[15][:, 1].view(np.uint32))
        thr64 = np.arctan((raw[:, 1].astype(np.float64) * 20 * 1.1 - act_speed) * 2) / (np.pi / 2)
        assert min(np.abs(thr64 + 0.2).min(), np.abs(thr64).min()) >= 1e-3
        assert (thr64 > 0.8).any() and ((thr64 > -0.2) & (thr64 < 0)).any() and (thr64 < -0.8).any()
    d_frames = env.scratch(SLOT_JPEG_IN, (n, h, w, 3), np.uint8)
    d_speed, d_segment = (env.scratch(s, (n,), np.float32) for s in SLOT_PILOT_IN)
    env.upload(d_frames, frames); env.upload(d_speed, act_speed); env.upload(d_segment, segment)
    ai = env.pilot_act_device(frames=d_frames, speed=d_speed, cfg=cfg, segment=d_segment if kind == "cnn_2d_full_house" else None)
    steer, thr, brk = (env.to_host(a) for a in ai)
    for i in range(n):
        if kind == "cnn_2d_speed_as_feature":                                # both outputs capped, no breaking (keras_pilot.py:67-76)
            want = (np.clip(raw[i, 0], -1, 1), np.clip(raw[i, 1], -1, 1), 0.0)
            assert (steer[i], thr[i], brk[i]) == want, (i, steer[i], thr[i], brk[i], want)
        else:
            want = pilot_postprocess(raw[i], float(act_speed[i]), cfg)
            assert steer[i] == np.float32(want[0]) and abs(float(thr[i]) - want[1]) <= 1e-5 and brk[i] == want[2] == 0.0, (i, steer[i], thr[i], brk[i], want)
            assert want[1] != 0.0 or thr[i] == 0.0
    print(f"{kind}: sweep 1 took {time.perf_counter() - t0:.2f} s")


@pytest.mark.gpu
def test_two_heads_at_64_frames_per_workgroup_and_a_batch_change_on_one_handle(make_env, planner):
    """Sweep 2.  150 frames of 240x320 plan trs_pilot_dense_kernel<2> (the smallest such shape in the suite) for dense1 and dense4: three frame groups, the last
    of 22 frames, KS = 62.  Then the first 40 frames on the same handle (NF = 1, KS = 123: smaller slabs, another stride and slice count, nothing reallocated),
    the 150 again, and the 150 after a reload with dense = 2 (NF = 1, KS = 41; the reload makes a new context, so both slabs are reserved anew)."""
    t0 = time.perf_counter()
    kind = "cnn_2d_full_house"
    h, w, n = SWEEP2
    named, F = slice_weights(h, w, kind, seed=7)
    frames = slice_frames(h, w, n, seed=5)
    speed, segment = side_inputs(n, seed=6)
    big, small, plain = planner.call(h, w, n, n, arrays=42), planner.call(h, w, n, 40, arrays=42), planner.call(h, w, n, n, arrays=42, dense=2)
    assert big["nf"] == 2 and big["KS"] % 8 != 0 and big["groups"] == 3, NO_MISTAKE
    assert small["nf"] == 1 and small["KS"] % 8 != 0 and small["KS"] != big["KS"] and small["KS"] * 40 < big["KS"] * n, NO_MISTAKE
    assert plain["nf"] == 1 and plain["KS"] % 8 != 0 and plain["KS"] != big["KS"], NO_MISTAKE
    env = make_env("hip", n_envs=n, img_h=h, img_w=w)
    env.pilot_load(named)
    first = forward(env, kind, frames, speed, segment)
    x7 = env.pilot_layer(6, (n,) + flatten_shape(h, w)).reshape(n, -1)
    assert x7.shape[1] == F
    chunks = chunk_products(x7, named, kind)
    right = None
    for call, m in ((big, n), (small, 40), (plain, n)):                       # the condition on the reference, for the slices of each call
        sums = {nm: slice_sums(c[:, :m], call["gps"]) for nm, c in chunks.items()}
        assert all(len(s) == call["KS"] for s in sums.values())
        top, least, ref = least_notice(sums, speed[:m], segment[:m], named, kind)
        print(f"sweep 2, {m} frames in {call['KS']} slices: max |reference| {top:.3f}, least notice {least:.3e}")
        assert top <= 4.0 and least >= SENSITIVITY, (m, top, least)
        right = ref if right is None else right
    assert frames_alike(right) < 0.01
    few = forward(env, kind, frames[:40], speed[:40], segment[:40])
    third = forward(env, kind, frames, speed, segment)
    env.pilot_tuning(dense=2)
    env.pilot_load(named)
    fourth = forward(env, kind, frames, speed, segment)
    dev = {"150 frames": np.abs(first - right).max(), "40 frames": np.abs(few - right[:40]).max(), "150 again": np.abs(third - right).max(),
           "150 at dense = 2": np.abs(fourth - right).max()}
    order = {"40 frames": np.abs(few - first[:40]).max(), "150 at dense = 2": np.abs(fourth - first).max()}
    print(f"sweep 2: max |HIP - reference| {dev}, max |HIP - first call| {order}")
    assert all(d <= TOL_REF for d in dev.values()), dev
    assert all(d <= TOL_ORDER for d in order.values()), order
    assert np.array_equal(third.view(np.uint32), first.view(np.uint32))
    print(f"sweep 2 took {time.perf_counter() - t0:.2f} s")
