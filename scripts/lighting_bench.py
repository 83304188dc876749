#!/usr/bin/env python3
"""Scene lighting (trs_set_lighting, include/trsim_spec.h "scene lighting") against unlit frames on the same box: 1024 envs x 120x160 RGB and
512 envs x 240x320 RGB + depth, one launch per step (HIP events on the handle's stream around 2000 steps) and the resident worker (every step
posted on its own; host wall clock between completion flags, as scripts/lens_bench.py).  Unlit and lit alternate per configuration; the lit
handle's parameters are a torch CUDA tensor drawn by lighting_params (gain 0.6-1.4, bias -30..30 per env and channel)."""
import sys, time
sys.path.insert(0, ".")
import torch
from triton_racer_sim_amd.env import BatchedEnv, lighting_params

STEPS = 2000
CONFIGS = [(1024, 120, 160, False), (512, 240, 320, True)]


def per_step_us(env, resident):
    env.set_step_mode(resident, 100000)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:                       # warm-up
        env.step_synthetic(200, 1); env.sync()
    if resident:
        t1 = time.perf_counter()
        env.step_synthetic(STEPS, 1); env.sync()
        return (time.perf_counter() - t1) * 1e6 / STEPS
    env.sync()
    env.event_record(0)
    env.step_synthetic(STEPS, 1)
    env.event_record(1)
    env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / STEPS


for n, h, w, depth in CONFIGS:
    params = torch.as_tensor(lighting_params(n, seed=1), device="cuda")
    torch.cuda.synchronize()
    for resident in (False, True):
        res = {}
        for lit in (False, True, False, True):
            env = BatchedEnv(n_envs=n, img_h=h, img_w=w, auto_reset=True, depth=depth)
            if lit:
                env.set_lighting(params)
            us = per_step_us(env, resident)
            res.setdefault("lit" if lit else "unlit", []).append(us)
            env.close()
        u, l = min(res["unlit"]), min(res["lit"])
        print(f"{n:5d} x {h}x{w} {'rgb+depth' if depth else 'rgb      '} {'resident' if resident else 'launch  '}  unlit {u:7.2f} us  lit {l:7.2f} us  "
              f"ratio {l / u:5.3f}  (runs: unlit {', '.join(f'{v:.2f}' for v in res['unlit'])}; lit {', '.join(f'{v:.2f}' for v in res['lit'])})", flush=True)
