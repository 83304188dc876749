#!/usr/bin/env python3
"""The minibatch loader (trs_sample_batch, include/trsim_spec.h "training minibatches") on one box: a set of 1024 frames of 120x160 RGB from
BatchedEnv.collect, minibatches of 128 (the reference's default) and 1024 records, the legs alternating three times inside one run:
  main     trs_sample_batch, float32 NCHW (HIP events on the handle's stream around the calls), against the torch expression it replaces,
           frames[idx].float().div(255).permute(0, 3, 1, 2).contiguous() on the same device with idx already there (torch events); pass line: faster
  hbm      a plain device-to-device copy moving the same traffic: a float32 batch reads R bytes and writes 4 R, a copy of 2.5 R bytes reads and writes
           2.5 R; target: the gather takes at most 1.25 x that copy
  others   float32 NHWC, binary16 NCHW and NHWC, uint8 NHWC, each against the copy of its own traffic (binary16: 1.5 R, uint8: R)
  fixed    where a call's fixed part goes: the host's own time per call (the clock around the same loop before the stream is waited for: ctypes, the
           library's checks, the launch) beside the stream's time per call, and a batch of ONE record (no traffic to speak of: the launch alone)
Run from the repository root: python scripts/loader_bench.py [> profiles/rNN_loader.txt]"""
import ctypes as C
import sys
import time
sys.path.insert(0, ".")
import numpy as np
import torch
from triton_racer_sim_amd.env import BatchedEnv

N, H, W, ROUNDS = 1024, 120, 160, 3
BATCHES = [(128, 400), (1024, 100)]                       # (batch size, calls per timing)
LEGS = [("nchw", "float32", 2.5), ("nhwc", "float32", 2.5), ("nchw", "float16", 1.5), ("nhwc", "float16", 1.5), ("nhwc", "uint8", 1.0)]


HOST = []                                                 # the host's time per call of the latest timed(), us


def timed(env, calls, fn):
    env.sync()
    env.event_record(0)
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    HOST[:] = [(time.perf_counter() - t0) * 1e6 / calls]
    env.event_record(1)
    env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / calls


def sampler(ds, cfg, batch, images, feats, labels, index):
    """trs_sample_batch of the epoch's first batch with its arguments converted once: the timed loop is the library call alone."""
    ptr = lambda t: int(t.data_ptr()) or None
    fn, args = ds.env.api.sample_batch, (ds.env._h, C.byref(cfg), ptr(ds.frames), ptr(ds.rows), 0, 0, 0, batch, ptr(images), ptr(feats) if feats.numel() else None,
                                         ptr(labels), ptr(index))
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
R1 = H * W * 3
print(f"== {N} records of {H}x{W} RGB ({N * R1 / 1e6:.1f} MB as uint8), one MI355X; figures are the minimum of {ROUNDS} alternating runs ==")
for batch, calls in BATCHES:
    R = batch * R1
    bufs = {(lay, dt): ds._buffers(batch, lay, dt) for lay, dt, _ in LEGS}
    cfgs = {(lay, dt): ds.config(lay, dt) for lay, dt, _ in LEGS}
    idx = torch.as_tensor(ds.order("train", 0)[:batch].astype(np.int64), device="cuda")
    expr = lambda: ds.frames[idx].float().div(255).permute(0, 3, 1, 2).contiguous()
    ours = next(iter(ds.batches(batch, 0)))[0]
    diff = (expr() - ours).abs().max().item()            # torch divides by a scalar by multiplying with its reciprocal: the same batch to one ulp, not to the bit
    assert diff <= 2.0 ** -24, diff
    copies = {}
    for traffic in sorted({t for _, _, t in LEGS}):
        a = torch.randint(0, 255, (int(traffic * R),), dtype=torch.uint8, device="cuda")
        copies[traffic] = (a, torch.empty_like(a))
    res = {}
    for _ in range(ROUNDS):
        for lay, dt, traffic in LEGS:
            b, c = bufs[lay, dt], cfgs[lay, dt]
            res.setdefault((lay, dt), []).append(timed(env, calls, sampler(ds, c, batch, *b)))
            if (lay, dt) == ("nchw", "float32"):
                res.setdefault("host", []).append(HOST[0])
                res.setdefault("one", []).append(timed(env, calls, sampler(ds, c, 1, *b)))
                res.setdefault("one host", []).append(HOST[0])
                res.setdefault("torch", []).append(torch_timed(calls, expr))
        for traffic, (a, b) in copies.items():
            res.setdefault(("copy", traffic), []).append(torch_timed(calls, lambda: b.copy_(a)))
    print(f"== batch {batch}: R = {R / 1e6:.2f} MB read per batch; max |torch expression - trs_sample_batch| = {diff:.3g} ==")
    show("trs_sample_batch, float32 NCHW", res["nchw", "float32"])
    show("torch: frames[idx].float().div(255).permute(0,3,1,2).contiguous()", res["torch"])
    ratio = min(res["torch"]) / min(res["nchw", "float32"])
    print(f"  torch expression / trs_sample_batch: {ratio:.2f} x (pass line: the kernel is faster: {'met' if ratio > 1 else 'MISSED'})")
    show("  the host's own time per call, the stream not waited for", res["host"])
    show("trs_sample_batch, float32 NCHW, a batch of ONE record", res["one"])
    show("  the host's own time per call, the stream not waited for", res["one host"])
    for traffic in sorted(copies):
        show(f"plain device-to-device copy of {traffic} R = {traffic * R / 1e6:.2f} MB", res["copy", traffic])
    for lay, dt, traffic in LEGS:
        r = min(res[lay, dt]) / min(res["copy", traffic])
        if (lay, dt) != ("nchw", "float32"):
            show(f"trs_sample_batch, {dt} {lay.upper()}", res[lay, dt])
        print(f"  {dt} {lay.upper()} / copy of {traffic} R: {r:.3f} x (target 1.25 x: {'met' if r <= 1.25 else 'MISSED'})", flush=True)
env.close()
