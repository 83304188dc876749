#!/usr/bin/env python3
"""trs_decode_jpeg on the files of the env's own rendered frames (quality 75, made by trs_encode_jpeg, device resident) beside the encoder, the HBM
yardstick and the host path it replaces, per workload, on one box in one run:

  decode        us per batch of trs_decode_jpeg from the encoder's slots (HIP events around steady-state repeats after a warm-up), and of
                BatchedEnv.decode_jpeg (host clock: upload of the packed files, the kernel, copies of statuses and frames, one call)
  encode        us per batch of trs_encode_jpeg on the same frames
  trim          us per batch of trs_preprocess's trim kernel on the same frames: one read plus one write of the frames
  Pillow+upload wall time of the path the decoder replaces for the same files: Image.open per file on at most 16 host threads, then one
                upload of the frames ("not measured" where Pillow does not import)

Usage: jpeg_decode_bench.py [out_file]        (workloads: 1024 x 120x160 and 256 x 240x320)"""
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, ".")
import ctypes as C

import numpy as np

from triton_racer_sim_amd.env import SLOT_JPEG_IN, BatchedEnv

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
say(f"trs_decode_jpeg, files of quality {QUALITY}: {WARMUP} warm-up + {REPEATS} timed calls per figure, rendered frames after 20 synthetic steps")
for n, h, w in ((1024, 120, 160), (256, 240, 320)):
    env = BatchedEnv(n_envs=n, auto_reset=True, img_h=h, img_w=w)
    env.step_synthetic(20, 1)
    frame = h * w * 3
    cap = env.jpeg_default_cap(QUALITY)
    slots, ln, off, dst, status = (C.c_void_p() for _ in range(5))
    for ptr, size in ((slots, n * cap), (ln, 4 * n), (off, 8 * n), (dst, n * frame), (status, 4 * n)):
        assert hip.hipMalloc(C.byref(ptr), C.c_size_t(size)) == 0
    offsets = np.arange(n, dtype=np.int64) * cap
    env.api.check(env.api.upload(env._h, off, offsets.ctypes.data, offsets.nbytes), "upload")
    enc = lambda: env.api.check(env.api.encode_jpeg(env._h, None, n, QUALITY, slots, cap, ln), "encode_jpeg")
    dec = lambda: env.api.check(env.api.decode_jpeg(env._h, slots, off, ln, n, dst, status), "decode_jpeg")
    enc()
    files = env.encode_jpeg(quality=QUALITY)
    total = int(files.offsets[-1])
    assert (files.lengths > 0).all()
    say()
    say(f"== {n} x {h}x{w}: {n * frame / 1e6:.1f} MB of frames, {total / 1e6:.2f} MB of files ({total / n:.0f} B per file) in slots of {cap} bytes ==")
    spread = [events(env, dec) for _ in range(3)]
    us = min(spread)
    say(f"trs_decode_jpeg                  {us:9.2f} us per batch  (three windows: {', '.join(f'{x:.2f}' for x in spread)})   "
        f"{n * frame / us / 1e3:7.1f} GB/s of frames written, {total / us / 1e3:.2f} GB/s of files read, {n * h * w / us:.0f} pixels/us")
    t0 = time.perf_counter()
    for _ in range(20):
        frames, st = env.decode_jpeg(files)
    host_us = (time.perf_counter() - t0) / 20 * 1e6
    assert (st == 0).all()
    say(f"BatchedEnv.decode_jpeg (host)    {host_us:9.2f} us per call, wall (join + upload of the files, the kernel, copies of statuses and of {n * frame / 1e6:.1f} MB of frames)")
    spread = [events(env, enc) for _ in range(3)]
    say(f"trs_encode_jpeg                  {min(spread):9.2f} us per batch  (three windows: {', '.join(f'{x:.2f}' for x in spread)})   decode / encode = {us / min(spread):.2f}")
    pc = env.pre_config({})
    trim = [events(env, lambda: env.preprocess_latest(pc)) for _ in range(3)]
    say(f"trs_preprocess identity trim     {min(trim):9.2f} us per batch  (three windows: {', '.join(f'{x:.2f}' for x in trim)})   {2 * n * frame / min(trim) / 1e3:7.1f} GB/s (read + write once)   decode / trim = {us / min(trim):.1f}")
    try:
        from PIL import Image

        blobs = [files[i] for i in range(n)]
        threads = min(16, os.cpu_count() or 1)
        d = C.c_void_p()
        env.api.check(env.api.scratch(env._h, SLOT_JPEG_IN, n * frame, C.byref(d)), "scratch")
        with ThreadPoolExecutor(threads) as pool:
            walls, decodes = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                ref = np.stack(list(pool.map(lambda b: np.asarray(Image.open(io.BytesIO(b))), blobs)))
                t1 = time.perf_counter()
                env.api.check(env.api.upload(env._h, d, ref.ctypes.data, ref.nbytes), "upload")
                env.sync()
                walls.append(time.perf_counter() - t0); decodes.append(t1 - t0)
        same = np.array_equal(ref, frames)
        say(f"Pillow on {threads} threads + upload     {min(walls) * 1e6:9.0f} us per batch, wall (best of 5; the decoding alone {min(decodes) * 1e6:.0f} us; "
            f"{'the same frames as the kernel' if same else 'FRAMES DIFFER FROM THE KERNEL'})")
        verdict = "beats" if us < min(walls) * 1e6 and host_us < min(walls) * 1e6 else "**DOES NOT BEAT**"
        say(f"the device call {verdict} the host path: {min(walls) * 1e6 / us:.0f} x (trs_decode_jpeg), {min(walls) * 1e6 / host_us:.1f} x (BatchedEnv.decode_jpeg, files and frames through the host)")
    except ImportError:
        say("Pillow + upload                  not measured (Pillow does not import here)")
    for ptr in (slots, ln, off, dst, status):
        hip.hipFree(ptr)
    env.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
