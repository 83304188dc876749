#!/usr/bin/env python3
"""trs_jpeg_roundtrip (the camera codec, include/trsim_spec.h "camera codec (JPEG round trip)") on the env's own rendered frames (device resident,
quality 75) beside what it replaces and its yardsticks, on one box in one run, the calls alternating ROUNDS times, per workload:

  round trip     us per batch of trs_jpeg_roundtrip (HIP events around steady-state repeats after a warm-up)
  encode+decode  trs_encode_jpeg followed by trs_decode_jpeg of its slots: the way to the same bytes without the codec kernel (compared once)
  encode         trs_encode_jpeg alone.  PASS LINE: the round trip is faster than this — it does the encoder's transform stage without the entropy
                 stage, and adds an inverse transform of the same arithmetic size
  trim           trs_preprocess's identity trim kernel on the same frames: one read plus one write of them, the image path's HBM yardstick
  closed loop    trs_step_pilot per tick without and with trs_set_camera_codec(75) (no target: reported)

Usage: jpeg_codec_bench.py [out_file]        (workloads: 1024 x 120x160 and 256 x 240x320)"""
import os
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import ctypes as C

import numpy as np

from triton_racer_sim_amd.env import BatchedEnv

WARMUP, REPEATS, ROUNDS, QUALITY, TICKS = 10, 100, 3, 75, 200
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def events(env, call, repeats=REPEATS, warmup=WARMUP):
    for _ in range(warmup):
        call()
    env.sync(); env.event_record(0)
    for _ in range(repeats):
        call()
    env.event_record(1); env.sync()
    return env.event_elapsed_ms(0, 1) * 1e3 / repeats


def fetch(hip, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), ptr, C.c_size_t(nbytes), 2) == 0       # hipMemcpyDeviceToHost
    return out


hip = C.CDLL(None)                                      # hipMalloc of the runtime libtrsim.so already uses (no torch import: slow on a fresh box)
say(f"trs_jpeg_roundtrip, quality {QUALITY}: {WARMUP} warm-up + {REPEATS} timed calls per window, {ROUNDS} windows per call, alternating; rendered frames after 20 synthetic steps")
ok = True
for n, h, w in ((1024, 120, 160), (256, 240, 320)):
    env = BatchedEnv(n_envs=n, auto_reset=True, img_h=h, img_w=w)
    env.step_synthetic(20, 1)
    frame = h * w * 3
    cap = env.jpeg_default_cap(QUALITY)
    bufs = {k: C.c_void_p() for k in ("slots", "len", "off", "status", "two", "one")}
    sizes = {"slots": n * cap, "len": 4 * n, "off": 8 * n, "status": 4 * n, "two": n * frame, "one": n * frame}
    for k, p in bufs.items():
        assert hip.hipMalloc(C.byref(p), C.c_size_t(sizes[k])) == 0
    off = np.arange(n, dtype=np.int64) * cap
    assert hip.hipMemcpy(bufs["off"], C.c_void_p(off.ctypes.data), C.c_size_t(off.nbytes), 1) == 0
    api, hd = env.api, env._h
    enc = lambda: api.check(api.encode_jpeg(hd, None, n, QUALITY, bufs["slots"], cap, bufs["len"]), "encode_jpeg")
    dec = lambda: api.check(api.decode_jpeg(hd, bufs["slots"], bufs["off"], bufs["len"], n, bufs["two"], bufs["status"]), "decode_jpeg")
    rt = lambda: api.check(api.jpeg_roundtrip(hd, None, n, QUALITY, bufs["one"], None), "jpeg_roundtrip")
    both = lambda: (enc(), dec())
    pc = env.pre_config({})
    calls = {"trs_jpeg_roundtrip": rt, "trs_encode_jpeg + trs_decode_jpeg": both, "trs_encode_jpeg": enc, "trs_preprocess identity trim": lambda: env.preprocess_latest(pc)}
    res = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, call in calls.items():
            res[k].append(events(env, call))
    env.sync()
    same = np.array_equal(fetch(hip, bufs["one"], n * frame), fetch(hip, bufs["two"], n * frame))
    lens = fetch(hip, bufs["len"], 4 * n).view(np.int32)
    say()
    say(f"== {n} x {h}x{w}: {n * frame / 1e6:.1f} MB of frames; the round trip's frames are {'the same bytes as' if same else 'NOT THE BYTES OF'} decode(encode()) "
        f"({int((lens > 0).sum())} of {n} files fitted their slots) ==")
    for k, runs in res.items():
        us = min(runs)
        say(f"{k:36s} {us:9.2f} us per batch  (windows: {', '.join(f'{x:.2f}' for x in runs)})   {2 * n * frame / us / 1e3:7.1f} GB/s of frames read + written once, {n * h * w / us:.0f} pixels/us")
    r, e, t = min(res["trs_jpeg_roundtrip"]), min(res["trs_encode_jpeg"]), min(res["trs_preprocess identity trim"])
    passed = max(res["trs_jpeg_roundtrip"]) < e and same
    ok = ok and passed
    say(f"pass line (round trip faster than trs_encode_jpeg alone, every window against its best): {'PASS' if passed else 'FAIL'}: {r:.2f} us = {r / e:.3f} x the encoder, "
        f"{r / min(res['trs_encode_jpeg + trs_decode_jpeg']):.3f} x encode + decode, {r / t:.2f} x the identity trim")
    for p in bufs.values():
        hip.hipFree(p)
    env.close()
    # the closed loop, a fresh handle per window
    from test_pilot import make_weights
    ws = make_weights(h, w, seed=1)
    loop = {"off": [], f"codec {QUALITY}": []}
    for _ in range(ROUNDS):
        for name in loop:
            env = BatchedEnv(n_envs=n, auto_reset=True, img_h=h, img_w=w)
            env.pilot_load(ws)
            if name != "off":
                env.set_camera_codec(QUALITY)
            env.step_pilot(30); env.sync()
            env.event_record(0)
            env.step_pilot(TICKS)
            env.event_record(1); env.sync()
            loop[name].append(env.event_elapsed_ms(0, 1) * 1e3 / TICKS)
            env.close()
    for name, runs in loop.items():
        say(f"trs_step_pilot, camera codec {name:9s} {min(runs):9.2f} us per tick  (windows: {', '.join(f'{x:.2f}' for x in runs)})")
    say(f"closed-loop overhead of the codec: {min(loop[f'codec {QUALITY}']) - min(loop['off']):.2f} us per tick (the kernel alone: {r:.2f} us)")
say()
say("pass line over both workloads: " + ("PASS" if ok else "FAIL"))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
