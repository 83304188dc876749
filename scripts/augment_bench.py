#!/usr/bin/env python3
"""The augmented minibatches (trs_sample_batch_aug, include/trsim_spec.h "training minibatches, augmentation") on one box: a set of 1024 frames of
120x160 RGB from BatchedEnv.collect, minibatches of 128 and 1024 records, mirror 0.5 with a per-channel jitter of 0.25 / 32, the legs alternating three
times inside one run:
  main     trs_sample_batch_aug, float32 NCHW, against trs_sample_batch on the same set and shape (HIP events on the handle's stream around the calls):
           the plain gather moves the same bytes, so the standing pass line applies at batch 1024: at most 1.25 x the plain call.  At batch 128 both
           calls carry the fixed part of a call (README, "Training minibatches"): the ratio is reported, it is no pass line.
  others   float32 NHWC, binary16 NCHW and NHWC, uint8 NHWC, each against the plain call of its own layout and type
  torch    context, no pass line: the passes a user runs behind the plain float32 NCHW batch today — flip where flagged, x * gain + bias, clamp, the
           label's sign — on the same device with the flags and parameters already there (torch events), alone and on top of the plain call
Run from the repository root: python scripts/augment_bench.py [> profiles/rNN_augment.txt]"""
import ctypes as C
import sys
sys.path.insert(0, ".")
import numpy as np
import torch
from triton_racer_sim_amd import Augment
from triton_racer_sim_amd.env import BatchedEnv

N, H, W, ROUNDS = 1024, 120, 160, 3
BATCHES = [(128, 400), (1024, 100)]                       # (batch size, calls per timing)
LEGS = [("nchw", "float32"), ("nhwc", "float32"), ("nchw", "float16"), ("nhwc", "float16"), ("nhwc", "uint8")]
AUG = Augment(mirror=0.5, gain=0.25, bias=32.0, per_channel=True, seed=29)


def timed(env, calls, fn):
    env.sync()
    env.event_record(0)
    for _ in range(calls):
        fn()
    env.event_record(1)
    env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / calls


def sampler(ds, cfg, aug, batch, images, feats, labels, index):
    """The epoch's first batch with the arguments converted once: the timed loop is the library call alone (aug None: trs_sample_batch)."""
    ptr = lambda t: int(t.data_ptr()) or None
    tail = (ptr(ds.frames), ptr(ds.rows), 0, 0, 0, batch, ptr(images), ptr(feats) if feats.numel() else None, ptr(labels), ptr(index))
    if aug is None:
        fn, args = ds.env.api.sample_batch, (ds.env._h, C.byref(cfg)) + tail
    else:
        fn, args = ds.env.api.sample_batch_aug, (ds.env._h, C.byref(cfg), C.byref(aug)) + tail
    return lambda: fn(*args)


def torch_timed(calls, fn):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def show(name, runs):
    print(f"  {name:64s} {min(runs):10.3f} us  (runs: {', '.join(f'{v:.3f}' for v in runs)})", flush=True)


env = BatchedEnv(n_envs=N, img_h=H, img_w=W, auto_reset=True)
env.set_expert(sigma=1.5)
env.step_expert(30)
frames, rows = env.collect(1, every=1, skip=0)
ds = env.dataset(frames, rows, split=1.0, seed=1)
assert len(ds) == ds.n_train == N
aug = AUG.config(env.api)
R1 = H * W * 3
print(f"== {N} records of {H}x{W} RGB ({N * R1 / 1e6:.1f} MB as uint8), one MI355X; {AUG!r}; figures are the minimum of {ROUNDS} alternating runs ==")
for batch, calls in BATCHES:
    bufs = {leg: ds._buffers(batch, *leg) for leg in LEGS}
    cfgs = {leg: ds.config(*leg) for leg in LEGS}
    _, mirror, params = ds.augmentation(AUG, "train", 0, 0, batch)
    m = torch.as_tensor(mirror, device="cuda")
    g = torch.as_tensor(params[:, 0:3].copy(), device="cuda")[:, :, None, None]
    b = torch.as_tensor(params[:, 4:7].copy() / np.float32(255), device="cuda")[:, :, None, None]
    x, _, lab, _ = bufs["nchw", "float32"]

    def expr():
        y = torch.where(m[:, None, None, None], x.flip(3), x)
        y = (y * g + b).clamp_(0, 1)
        steer = torch.where(m, -lab[:, 0], lab[:, 0])
        return y, steer

    # what the kernel computes against the torch passes on the plain batch: the kernel rounds to a byte before it divides by 255, so half a byte apart at most
    sampler(ds, cfgs["nchw", "float32"], None, batch, *bufs["nchw", "float32"])()
    env.sync()
    want, steer = expr()
    torch.cuda.synchronize()                               # the env's stream does not wait for torch's
    sampler(ds, cfgs["nchw", "float32"], aug, batch, *bufs["nchw", "float32"])()
    env.sync()
    diff = (want - x).abs().max().item()
    assert diff <= 0.51 / 255 and torch.equal(steer, lab[:, 0]), diff
    res = {}
    for _ in range(ROUNDS):
        for leg in LEGS:
            res.setdefault(("plain", leg), []).append(timed(env, calls, sampler(ds, cfgs[leg], None, batch, *bufs[leg])))
            res.setdefault(("aug", leg), []).append(timed(env, calls, sampler(ds, cfgs[leg], aug, batch, *bufs[leg])))
        res.setdefault("torch", []).append(torch_timed(calls, expr))
    print(f"== batch {batch}: {int(mirror.sum())} of {batch} records mirrored; max |torch passes - trs_sample_batch_aug| = {diff * 255:.3f} / 255 ==")
    for leg in LEGS:
        lay, dt = leg
        show(f"trs_sample_batch, {dt} {lay.upper()}", res["plain", leg])
        show(f"trs_sample_batch_aug, {dt} {lay.upper()}", res["aug", leg])
        r = min(res["aug", leg]) / min(res["plain", leg])
        line = f"pass line 1.25 x: {'met' if r <= 1.25 else '**MISSED**'}" if batch == 1024 else "no pass line at this batch: both calls carry the fixed part of a call"
        print(f"  {dt} {lay.upper()}: augmented / plain = {r:.3f} x ({line})", flush=True)
    show("torch: where(flip) , x * g + b, clamp, label sign on the float32 NCHW batch", res["torch"])
    t, p, a = min(res["torch"]), min(res["plain", LEGS[0]]), min(res["aug", LEGS[0]])
    print(f"  context: plain call + torch passes = {p + t:.3f} us, {(p + t) / a:.2f} x the augmented call", flush=True)
env.close()
