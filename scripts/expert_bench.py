#!/usr/bin/env python3
"""The scripted expert (trs_set_expert / trs_step_expert, include/trsim_spec.h "scripted expert") on one box, launch mode, at 1024 envs x 120x160 and
256 envs x 240x320 RGB, the legs alternating three times:
  tick     trs_step_expert, one tick per call, against trs_step with device controls, one step per call, on the same handle (HIP events on the handle's
           stream around the calls): the difference is the expert's launch
  capture  the same ticks with every tick captured (rows + frames, device to device) against the plain tick, and the difference against a plain
           device-to-device copy of one frame set (torch copy_ of a uint8 tensor of img_bytes); pass line: difference <= 1.25 x copy
  collect  BatchedEnv.collect per captured record against the host loop it replaces: fetch four state arrays, the numpy rule, trs_step_host, and the
           frames fetched on the captured ticks (wall clock); pass line: the device loop is faster
Run from the repository root: python scripts/expert_bench.py [> profiles/rNN_expert.txt]"""
import os, sys, time
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import numpy as np
import torch
from triton_racer_sim_amd.env import BatchedEnv
from test_expert_cpu import Driver, expert_rule, track_yaw_of

SHAPES = [(1024, 120, 160), (256, 240, 320)]
TICKS, CAP_TICKS, LOOP_TICKS, EVERY, ROUNDS = 1000, 40, 200, 5, 3
CFG = {"sigma": 1.5}


def timed(env, calls, fn):
    env.sync()
    env.event_record(0)
    for _ in range(calls):
        fn()
    env.event_record(1)
    env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / calls


def tick_legs(env):
    env.step_expert(50)
    st, th, br = (o.__cuda_array_interface__["data"][0] for o in env.expert_act())
    env.sync()
    plain = timed(env, TICKS, lambda: env.step_device(st, th, br))
    expert = timed(env, TICKS, lambda: env.step_expert(1))
    return plain, expert


def capture_leg(env, frames, rows):
    cap = {"every": 1, "skip": 0, "capacity": 1, "rows": rows, "frames": frames}      # every call fills slot 0 of the call
    env.step_expert(5, dict(cap, capacity=5))
    return timed(env, CAP_TICKS * 5, lambda: env.step_expert(1, cap))


def copy_us(nbytes):
    a = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(20):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(CAP_TICKS * 5):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (CAP_TICKS * 5)


def collect_leg(env):
    env.sync()
    t0 = time.perf_counter()
    frames, rows = env.collect(LOOP_TICKS, every=EVERY, skip=0)
    env.sync()
    dt = time.perf_counter() - t0
    return dt * 1e6 / rows.__cuda_array_interface__["shape"][0]


def host_leg(env, ty):
    drv = Driver(env.n, CFG)
    frames, labels = [], []
    env.sync()
    t0 = time.perf_counter()
    for t in range(LOOP_TICKS):
        steer, thr, brk = expert_rule(env.fetch("seg_idx"), env.fetch("yaw"), env.fetch("cte"), env.fetch("speed"), ty, CFG)
        if t % EVERY == 0:
            frames.append(env.fetch("img"))
            labels.append(steer)
        env.step(drv.applied(steer), thr, brk)
    env.sync()
    dt = time.perf_counter() - t0
    return dt * 1e6 / (len(frames) * env.n)


def show(name, runs, unit="us"):
    print(f"  {name:44s} {min(runs):10.3f} {unit}  (runs: {', '.join(f'{v:.3f}' for v in runs)})", flush=True)


for n, H, W in SHAPES:
    res = {k: [] for k in ("step", "expert", "capture", "copy", "collect", "host")}
    img_bytes = n * H * W * 3
    for _ in range(ROUNDS):
        env = BatchedEnv(n_envs=n, img_h=H, img_w=W, auto_reset=True)
        env.set_expert(**CFG)
        env.step(0.0, 0.0, 0.0)
        ty = track_yaw_of(env.fetch("tangent"))
        d_frames = torch.empty((5, n, H, W, 3), dtype=torch.uint8, device="cuda")
        d_rows = torch.empty((5, n, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        plain, expert = tick_legs(env)
        res["step"].append(plain); res["expert"].append(expert)
        res["capture"].append(capture_leg(env, d_frames, d_rows))
        res["copy"].append(copy_us(img_bytes))
        del d_frames, d_rows
        res["collect"].append(collect_leg(env))
        res["host"].append(host_leg(env, ty))
        env.close()
    print(f"== {n} envs x {H}x{W} RGB, launch mode, sigma = 1.5; {img_bytes / 1e6:.1f} MB of frames per tick ==")
    show("trs_step, device controls, one step per call", res["step"])
    show("trs_step_expert, one tick per call", res["expert"])
    print(f"  the expert's launch: {min(res['expert']) - min(res['step']):.3f} us per tick")
    show("trs_step_expert, every tick captured", res["capture"])
    show("plain device-to-device copy of the frames", res["copy"])
    extra = min(res["capture"]) - min(res["expert"])
    print(f"  capture - plain tick: {extra:.3f} us = {extra / min(res['copy']):.3f} x the copy (pass line 1.25 x: {'met' if extra <= 1.25 * min(res['copy']) else 'MISSED'})")
    show(f"collect, {LOOP_TICKS} ticks, every {EVERY}th captured: per record", res["collect"])
    show("host loop (4 fetches, numpy rule, step_host, frame fetch)", res["host"])
    ratio = min(res["host"]) / min(res["collect"])
    print(f"  host loop / device loop: {ratio:.1f} x (pass line: the device loop is faster: {'met' if ratio > 1 else 'MISSED'})", flush=True)
