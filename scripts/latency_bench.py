#!/usr/bin/env python3
"""Observation latency (trs_set_latency, include/trsim_spec.h "observation latency") against a handle without one on the same box: 1024 envs x 120x160
RGB in launch mode, one step per call (HIP events on the handle's stream around 2000 steps), the settings alternating five times:
  step        off | one latency for all (L = 3: the view points into the ring, no frame byte moved) | per-env latencies 0..6 (trs_obs_kernel gathers frames)
  copy        a plain device-to-device copy of one frame set (torch copy_ of a uint8 tensor of img_bytes), the yardstick of the gather:
              gather = per-env step - step with one latency for all; target gather <= 1.25 x copy
  closed loop trs_step_pilot per tick: off | L = 2 for all | per-env 0..3
Run from the repository root: python scripts/latency_bench.py [> profiles/r11_latency.txt]"""
import os, sys
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import numpy as np
import torch
from triton_racer_sim_amd.env import BatchedEnv

N, H, W = 1024, 120, 160
STEPS, TICKS, ROUNDS = 2000, 300, 5


def step_us(env):
    env.step_synthetic(200, 1); env.sync()
    env.event_record(0)
    env.step_synthetic(STEPS, 1)
    env.event_record(1)
    env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / STEPS


def loop_us(env):
    env.step_pilot(30); env.sync()
    env.event_record(0)
    env.step_pilot(TICKS)
    env.event_record(1)
    env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / TICKS


def copy_us(nbytes):
    a = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(50):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(STEPS):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / STEPS


def show(title, res, base):
    for name, runs in res.items():
        print(f"{title:12s} {name:18s} {min(runs):8.2f} us  ratio to {base} {min(runs) / min(res[base]):5.3f}  (runs: {', '.join(f'{v:.2f}' for v in runs)})", flush=True)


SETTINGS = {"off": None, "L = 3 for all": 3, "per-env 0..6": np.arange(N) % 7}
res = {k: [] for k in SETTINGS}
res["copy"] = []
for _ in range(ROUNDS):
    for name, ticks in SETTINGS.items():
        env = BatchedEnv(n_envs=N, img_h=H, img_w=W, auto_reset=True)
        if ticks is not None:
            env.set_latency(ticks, max_ticks=6)
        res[name].append(step_us(env))
        env.close()
    res["copy"].append(copy_us(N * H * W * 3))
print(f"{N} envs x {H}x{W} RGB, launch mode, one step per call, {STEPS} steps; ring at max_ticks = 6: 8 slots x {N * H * W * 3 / 1e6:.1f} MB")
show("step", res, "off")
gather = min(res["per-env 0..6"]) - min(res["L = 3 for all"])
print(f"gather       per-env - one for all {gather:8.2f} us = {gather / min(res['copy']):5.3f} x the plain copy of {N * H * W * 3} B ({min(res['copy']):.2f} us; target 1.25 x)", flush=True)

from test_pilot import make_weights
ws = make_weights(H, W, seed=1)
LOOP = {"off": None, "L = 2 for all": 2, "per-env 0..3": np.arange(N) % 4}
res = {k: [] for k in LOOP}
for _ in range(ROUNDS):
    for name, ticks in LOOP.items():
        env = BatchedEnv(n_envs=N, img_h=H, img_w=W, auto_reset=True)
        env.pilot_load(ws)
        if ticks is not None:
            env.set_latency(ticks, max_ticks=3)
        res[name].append(loop_us(env))
        env.close()
show("closed loop", res, "off")
