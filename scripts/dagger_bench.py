#!/usr/bin/env python3
"""The pilot in the loop with the expert's labels (trs_step_dagger, include/trsim_spec.h "pilot in the loop with the expert's labels") on one box, launch
mode, at 1024 envs x 120x160 and 256 envs x 240x320 RGB, the legs alternating ROUNDS times on one handle (HIP events on the handle's stream around the calls):
  (a) tick     trs_step_dagger without capture, one tick per call, minus trs_step_pilot, one tick per call: the price of trs_dagger_kernel's launch.
               Yardstick from the same run: trs_step_expert minus trs_step with device controls (the price of trs_expert_kernel's launch).
               Pass line: (a) <= yardstick + the spread (max - min) the run's own repeats of the yardstick show.
  (b) capture  the same ticks with every tick captured (rows + frames, device to device) minus the plain dagger tick, against a plain device-to-device
               copy of one frame set (torch copy_ of a uint8 tensor of img_bytes); pass line: difference <= 1.25 x copy
  (c) bench    python bench.py --gpus 1, the parent commit's library (scripts/ab_bin/libtrsim_prev.so, built by scripts/build_prev.sh <parent>) and the
               in-tree build alternating ROUNDS times; pass line: the new runs lie inside the parent's spread (skipped when that library is absent)
Run from the repository root: python scripts/dagger_bench.py [--out profiles/rNN_dagger.txt] [--skip-bench]"""
import argparse, json, os, subprocess, sys
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import numpy as np

SHAPES = [(1024, 120, 160), (256, 240, 320)]
TICKS, CAP_TICKS, ROUNDS = 300, 100, 3
PCFG = {"spd_ctl_threshold": 1.1, "spd_ctl_reverse_multiplier": 1.0}
PREV_LIB = os.path.join("scripts", "ab_bin", "libtrsim_prev.so")
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def timed(env, calls, fn):
    env.sync()
    env.event_record(0)
    for _ in range(calls):
        fn()
    env.event_record(1)
    env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / calls


def copy_us(torch, nbytes):
    a = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(20):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(CAP_TICKS):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CAP_TICKS


def show(name, runs, unit="us"):
    say(f"  {name:58s} {min(runs):10.3f} {unit}  (runs: {', '.join(f'{v:.3f}' for v in runs)})")


def loops():
    import torch
    from triton_racer_sim_amd.env import BatchedEnv
    from test_pilot import make_weights
    for n, H, W in SHAPES:
        res = {k: [] for k in ("step", "expert", "pilot", "dagger", "capture", "copy")}
        img_bytes = n * H * W * 3
        env = BatchedEnv(n_envs=n, img_h=H, img_w=W, auto_reset=True)
        env.pilot_load(make_weights(H, W, seed=5))
        env.set_expert()
        env.step_expert(50)                                    # moving cars and a frame
        st, th, br = (o.__cuda_array_interface__["data"][0] for o in env.expert_act())
        d_frames = torch.empty((1, n, H, W, 3), dtype=torch.uint8, device="cuda")
        d_rows = torch.empty((1, n, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        cap = {"every": 1, "skip": 0, "capacity": 1, "rows": d_rows, "frames": d_frames}      # every call fills slot 0 of the call
        env.step_pilot(20, PCFG); env.step_dagger(20, PCFG, capture=dict(cap))               # warm every path
        for _ in range(ROUNDS):
            res["step"].append(timed(env, TICKS, lambda: env.step_device(st, th, br)))
            res["expert"].append(timed(env, TICKS, lambda: env.step_expert(1)))
            res["pilot"].append(timed(env, TICKS, lambda: env.step_pilot(1, PCFG)))
            res["dagger"].append(timed(env, TICKS, lambda: env.step_dagger(1, PCFG)))
            res["capture"].append(timed(env, CAP_TICKS, lambda: env.step_dagger(1, PCFG, capture=cap)))
            res["copy"].append(copy_us(torch, img_bytes))
        env.close()
        say(f"== {n} envs x {H}x{W} RGB, launch mode, beta 0.5; {img_bytes / 1e6:.1f} MB of frames per tick ==")
        show("trs_step, device controls, one step per call", res["step"])
        show("trs_step_expert, one tick per call", res["expert"])
        show("trs_step_pilot, one tick per call", res["pilot"])
        show("trs_step_dagger, one tick per call, no capture", res["dagger"])
        yard = [e - s for e, s in zip(res["expert"], res["step"])]
        mine = [d - p for d, p in zip(res["dagger"], res["pilot"])]
        spread = max(yard) - min(yard)
        a, y = min(res["dagger"]) - min(res["pilot"]), min(res["expert"]) - min(res["step"])
        say(f"  (a) dagger - pilot: {a:.3f} us per tick (per round: {', '.join(f'{v:.3f}' for v in mine)})")
        say(f"      yardstick expert - step: {y:.3f} us per tick (per round: {', '.join(f'{v:.3f}' for v in yard)}; spread {spread:.3f})")
        say(f"      pass line (a) <= yardstick + spread = {y + spread:.3f} us: {'met' if a <= y + spread else 'MISSED'}")
        show("trs_step_dagger, every tick captured", res["capture"])
        show("plain device-to-device copy of the frames", res["copy"])
        extra = min(res["capture"]) - min(res["dagger"])
        say(f"  (b) capture - plain tick: {extra:.3f} us = {extra / min(res['copy']):.3f} x the copy (pass line 1.25 x: {'met' if extra <= 1.25 * min(res['copy']) else 'MISSED'})")


def bench(steps, warmup):
    if not os.path.exists(PREV_LIB):
        say(f"== (c) python bench.py: skipped, {PREV_LIB} is absent (scripts/build_prev.sh <parent commit>) ==")
        return
    new_lib = os.path.join("triton-racer-sim_amd", "csrc", "libtrsim.so")
    vals = {"parent": [], "new": []}
    for _ in range(ROUNDS):
        for tag, lib in (("parent", PREV_LIB), ("new", new_lib)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], capture_output=True, text=True,
                                 env=dict(os.environ, TRS_HIP_LIB=os.path.abspath(lib)), timeout=600)
            if out.returncode != 0:
                raise SystemExit(f"bench.py failed with the {tag} library ({out.returncode}): {out.stderr[-2000:]}")
            line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
            vals[tag].append(float(json.loads(line)["value"]))
    say(f"== (c) python bench.py --gpus 1 --steps {steps} --warmup {warmup}, the parent's library and the in-tree build alternating ==")
    show("parent", [v / 1e6 for v in vals["parent"]], "M env-steps/s (first column: min)")
    show("new", [v / 1e6 for v in vals["new"]], "M env-steps/s (first column: min)")
    lo, hi = min(vals["parent"]), max(vals["parent"])
    inside = all(lo <= v <= hi for v in vals["new"])
    slower = any(v < lo for v in vals["new"])
    say(f"  the parent's spread: {lo / 1e6:.3f} .. {hi / 1e6:.3f}; every new run inside it: {'yes' if inside else 'NO'}"
        + ("" if inside else f" ({'a new run is SLOWER than every parent run' if slower else 'no new run is slower than the slowest parent run'})"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--skip-bench", action="store_true", help="leave out (c)")
    ap.add_argument("--skip-loops", action="store_true", help="leave out (a) and (b)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    if not args.skip_bench:
        bench(args.steps, args.warmup)                         # first: its child processes open the GPU by themselves, before this process does
    if not args.skip_loops:
        loops()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
