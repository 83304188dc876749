#!/usr/bin/env python3
"""The lens camera (trs_set_camera, include/trsim_spec.h "lens camera") against the pinhole camera on the same box: 1024 envs x 120x160 RGB and
512 envs x 240x320 RGB + depth, one launch per step (HIP events on the handle's stream around 2000 steps) and the resident worker (every step
posted on its own; host wall clock between completion flags, as scripts/hills_bench.py).  Pinhole and lens alternate per configuration."""
import sys, time
sys.path.insert(0, ".")
from triton_racer_sim_amd.env import BatchedEnv

STEPS = 2000
LENS = (0.8, 0.4, 0.3)
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
    for resident in (False, True):
        res = {}
        for cam in (None, LENS, None, LENS):
            env = BatchedEnv(n_envs=n, img_h=h, img_w=w, auto_reset=True, depth=depth, camera=cam)
            us = per_step_us(env, resident)
            res.setdefault("lens" if cam else "pinhole", []).append(us)
            env.close()
        p, l = min(res["pinhole"]), min(res["lens"])
        print(f"{n:5d} x {h}x{w} {'rgb+depth' if depth else 'rgb      '} {'resident' if resident else 'launch  '}  pinhole {p:7.2f} us  lens {l:7.2f} us  "
              f"ratio {l / p:5.2f}  (runs: pinhole {', '.join(f'{v:.2f}' for v in res['pinhole'])}; lens {', '.join(f'{v:.2f}' for v in res['lens'])})", flush=True)
