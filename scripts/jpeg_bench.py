#!/usr/bin/env python3
"""trs_encode_jpeg on the env's own rendered frames (device resident, quality 75) beside its two yardsticks, per workload:

  encode        us per batch of trs_encode_jpeg (HIP events around steady-state repeats after a warm-up), and of trs_encode_jpeg_host
                (host clock around calls that end in their one synchronisation: encode + pack + the two copies)
  trim          us per batch of trs_preprocess's trim kernel on the same frames: one read plus one write of the frames, the image path's
                HBM yardstick on this box
  fetch+Pillow  wall time per tick of the path the encoder replaces, for the same frames: fetch('img'), then Image.save per frame on at
                most 16 host threads ("not measured" where Pillow does not import)

Usage: jpeg_bench.py [out_file]        (workloads: 1024 x 120x160 and 256 x 240x320)"""
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, ".")
import ctypes as C

import numpy as np

from triton_racer_sim_amd.env import BatchedEnv

WARMUP, REPEATS, QUALITY = 10, 100, 75
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def events(env, call, repeats=REPEATS):
    for _ in range(WARMUP):
        call()
    env.sync(); env.event_record(0)
    for _ in range(repeats):
        call()
    env.event_record(1); env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / repeats


hip = C.CDLL(None)                                      # hipMalloc of the runtime libtrsim.so already uses (no torch import: slow on a fresh box)
say(f"trs_encode_jpeg, quality {QUALITY}: {WARMUP} warm-up + {REPEATS} timed calls per figure, rendered frames after 20 synthetic steps")
for n, h, w in ((1024, 120, 160), (256, 240, 320)):
    env = BatchedEnv(n_envs=n, auto_reset=True, img_h=h, img_w=w)
    env.step_synthetic(20, 1)
    frame = h * w * 3
    cap = env.jpeg_default_cap(QUALITY)
    dst, ln = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dst), C.c_size_t(n * cap)) == 0 and hip.hipMalloc(C.byref(ln), C.c_size_t(4 * n)) == 0
    say()
    say(f"== {n} x {h}x{w}: {n * frame / 1e6:.1f} MB of frames, slots of {cap} bytes ==")
    enc = lambda: env.api.check(env.api.encode_jpeg(env._h, None, n, QUALITY, dst, cap, ln), "encode_jpeg")
    spread = [events(env, enc) for _ in range(3)]
    files = env.encode_jpeg(quality=QUALITY)
    total = int(files.offsets[-1])
    assert (files.lengths > 0).all()
    us = min(spread)
    say(f"trs_encode_jpeg                  {us:9.2f} us per batch  (three windows: {', '.join(f'{x:.2f}' for x in spread)})   "
        f"{n * frame / us / 1e3:7.1f} GB/s of frames read, {total / 1e6:.2f} MB of files ({total / n:.0f} B per frame), {n * h * w / us:.0f} pixels/us")
    t0 = time.perf_counter()
    for _ in range(20):
        env.encode_jpeg(quality=QUALITY)
    say(f"BatchedEnv.encode_jpeg (host)    {(time.perf_counter() - t0) / 20 * 1e6:9.2f} us per call, wall (encode + pack + copies of offsets and min(blob, n * cap) = {n * cap / 1e6:.1f} MB + one sync)")
    pc = env.pre_config({})
    trim = [events(env, lambda: env.preprocess_latest(pc)) for _ in range(3)]
    say(f"trs_preprocess identity trim     {min(trim):9.2f} us per batch  (three windows: {', '.join(f'{x:.2f}' for x in trim)})   {2 * n * frame / min(trim) / 1e3:7.1f} GB/s (read + write once)")
    try:
        from PIL import Image

        def save(img):
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="JPEG")
            return buf.getvalue()

        threads = min(16, os.cpu_count() or 1)
        with ThreadPoolExecutor(threads) as pool:
            walls, fetches = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                imgs = env.fetch("img")
                t1 = time.perf_counter()
                ref = list(pool.map(save, imgs))
                walls.append(time.perf_counter() - t0); fetches.append(t1 - t0)
        same = all(ref[i] == files[i] for i in range(n))
        say(f"fetch + Pillow on {threads} threads     {min(walls) * 1e6:9.0f} us per tick, wall (best of 5; the fetch alone {min(fetches) * 1e6:.0f} us; one thread per save call, "
            f"{'the same bytes as the kernel' if same else 'BYTES DIFFER FROM THE KERNEL'})")
    except ImportError:
        say("fetch + Pillow                   not measured (Pillow does not import here)")
    hip.hipFree(dst); hip.hipFree(ln)
    env.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
