"""Uniform rows (sky, ground beyond the far plane) are stored once per frame buffer and palette, in every step path (trsim_plan.hpp, UniformRows).

Two things are checked through the C ABI against the CPU oracle.  The rows really are skipped: a marker byte written over them through the zero-copy
view survives later steps into the same buffer.  And nobody can tell: every byte a step does store equals the oracle's, and after any event that
changes those rows (another palette, another track, a whole-frame kernel variant) both buffers are the oracle's frames in every byte again."""
import time

import numpy as np
import pytest

from conftest import track_points
from test_gpu_parity import assert_state_equal

pytestmark = pytest.mark.gpu

STATIC = {"preprocessing_color_filter_enabled": True, "preprocessing_contrast_enhancement_ratio": 1.3}
DYNAMIC = {"preprocessing_dynamic_brightness_enabled": True, "preprocessing_contrast_enhancement_ratio": 1.2}


def leading_uniform_rows(env):
    pal = env.fetch("palette")
    u = 0
    while u < pal.shape[0] and (pal[u] == pal[u, 0]).all():
        u += 1
    return u


class Pair:
    """The library's env and the oracle's, stepped together; a marker byte no uniform row of the oracle's frames holds."""

    def __init__(self, make_env, torch, n, resident, kind="hip", **kw):
        self.torch = torch
        self.g, self.o = make_env(kind, n_envs=n, auto_reset=True, **kw), make_env("oracle", n_envs=n, auto_reset=True, **kw)
        if resident:
            self.g.set_step_mode(True, idle_us=300)
        self.u = leading_uniform_rows(self.o)
        assert self.u > 0 and (self.g.H != 120 or self.u == 49)
        self.mark = None

    def step(self, k=1, per_launch=1):
        for env in (self.g, self.o):
            env.step_synthetic(k, per_launch)

    def poison_latest(self):
        """Overwrite the uniform rows of the latest frame buffer from torch's stream, beside a worker that stays resident (trs_sync does not end it)."""
        t = self.torch.as_tensor(self.g.device_array("img"), device="cuda")
        if self.mark is None:
            used = np.unique(self.o.fetch("img")[:, :self.u])
            self.mark = int(next(v for v in range(0x5B, 0x5B + 256) if (v & 255) not in used)) & 255
        t[:, :self.u].fill_(self.mark)
        self.torch.cuda.current_stream().synchronize()              # the stream, not the device: a device-wide wait would wait for the worker

    def poison_both(self):
        self.poison_latest(); self.step(); self.poison_latest()

    def kept(self, where):
        """The latest buffer still holds the marker in its uniform rows; every other byte is the oracle's."""
        a, b = self.g.fetch("img"), self.o.fetch("img")
        assert not (b[:, :self.u] == self.mark).any(), where
        assert (a[:, :self.u] == self.mark).all(), f"{where}: uniform rows were stored again in envs {np.flatnonzero((a[:, :self.u] != self.mark).reshape(a.shape[0], -1).any(axis=1))[:8]}"
        assert np.array_equal(a[:, self.u:], b[:, self.u:]), where

    def whole(self, where):
        a, b = self.g.fetch("img"), self.o.fetch("img")
        assert np.array_equal(a, b), f"{where}: envs {np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[:8]}"

    def both_buffers(self, check, where):
        self.step(); check(f"{where}, first step")
        self.step(); check(f"{where}, second step")


@pytest.mark.parametrize("n,resident", [(301, True), (1024, True), (301, False), (1021, False)])     # 301, 1021: a ragged last workgroup; 1024: the benchmark's shard
def test_uniform_rows_are_skipped_and_nobody_can_tell(make_env, n, resident):
    torch = pytest.importorskip("torch")
    p = Pair(make_env, torch, n, resident)
    g, o = p.g, p.o
    p.step(4); g.sync()
    p.whole("four steps")
    p.poison_latest()
    p.step(2); g.sync()
    p.kept("two steps after the marker")                               # the same buffer is latest again: nothing stored its uniform rows
    p.poison_both()

    # ---- events that leave the rows as they are: the marker stays, everything else is the oracle's
    g.quiesce()
    p.both_buffers(p.kept, "after trs_quiesce")
    mask = np.random.default_rng(5).uniform(0, 1, n) < 0.3
    for env in (g, o):
        env.reset(mask)
    p.both_buffers(p.kept, "after trs_reset")
    pose = {k: o.fetch(k) for k in ("pos_x", "pos_y", "pos_z", "yaw", "vel")}
    for env in (g, o):
        env.set_pose(pose["pos_x"] + np.float32(0.25), pose["pos_y"], pose["pos_z"], pose["yaw"] + np.float32(0.1), pose["vel"])
    p.both_buffers(p.kept, "after trs_set_pose")
    if resident:
        g.sync(); time.sleep(0.05)                                     # the worker leaves by itself (idle_us = 300)
        p.both_buffers(p.kept, "after an idle exit")
    assert_state_equal(g, o, "after the events that keep the rows")

    # ---- events that change the rows or what writes them: the marker goes, both buffers are the oracle's frames
    for env in (g, o):
        env.set_frame_filter(STATIC)
    p.both_buffers(p.whole, "static frame filter on")
    p.poison_both()
    for env in (g, o):
        env.set_frame_filter(enabled=False)
    p.both_buffers(p.whole, "static frame filter off")
    p.poison_both()
    g.set_camera(0.4, 0.3, 0.1); p.step(); g.set_camera(None)          # (the oracle has no lens camera: its physics is the same)
    p.both_buffers(p.whole, "lens camera on and off")
    p.poison_both()
    for env in (g, o):
        env.set_frame_filter(DYNAMIC)
    p.step(); p.whole("one step with dynamic brightness")
    for env in (g, o):
        env.set_frame_filter(enabled=False)
    p.both_buffers(p.whole, "dynamic brightness on and off")
    p.poison_both()
    light = np.tile(np.float32([0.7, 1.2, 0.9, 0, 10, -20, 5, 0]), (n, 1))
    g.set_lighting(light); p.step(); g.set_lighting(None)             # (the oracle has no lighting: its physics is the same)
    p.both_buffers(p.whole, "lighting on and off")
    p.poison_both()
    for env in (g, o):
        env.load_track(track_points("generated"))
    p.both_buffers(p.whole, "after trs_load_track")
    p.step(2); g.sync()
    p.poison_latest()
    p.step(2); g.sync()
    p.kept("skipping again after the reload")
    assert_state_equal(g, o, "at the end")
    assert int(g.fetch("stats")[2]) == 0


def test_worker_generations_keep_skipping(make_env):
    """A worker that leaves because its lifetime is spent, under load: the next generation starts from the host's flags, so the marker survives dozens
    of generations."""
    torch = pytest.importorskip("torch")
    p = Pair(make_env, torch, 301, True, kind="hip_hooks")
    g, o = p.g, p.o
    p.step(5); g.sync()
    p.poison_both()
    g.resident_lifetime(300)
    p.step(600); g.sync()                                              # even: the buffer poisoned last is latest
    p.kept("after 600 steps in 0.3 ms generations")
    p.step(); g.sync()
    p.kept("the other buffer")
    assert_state_equal(g, o, "generations")


@pytest.mark.parametrize("depth", [False, True])
def test_alternating_step_paths_and_variants(make_env, depth):
    """One handle through every way a frame gets written, each whole-frame variant directly in front of a skipping one; after each segment both frame
    buffers (fetch, one more step, fetch) equal the oracle bit for bit."""
    from test_lighting_gpu import light_frames, params_for
    from test_pilot import make_weights
    n, h, w = 70, 120, 160
    kw = dict(n_envs=n, img_h=h, img_w=w, depth=depth, auto_reset=True)
    g, o = make_env("hip", **kw), make_env("oracle", **kw)

    def both(where, lit=None):
        for k in range(2):
            a, b = g.fetch("img"), o.fetch("img")
            if lit is not None:
                b = light_frames(b, lit)
            assert np.array_equal(a, b), f"{where}, buffer {k}: envs {np.flatnonzero((a != b).reshape(n, -1).any(axis=1))[:8]}"
            if depth:
                assert np.array_equal(g.fetch("depth").view(np.uint32), o.fetch("depth").view(np.uint32)), f"{where}, buffer {k}"
            if k == 0:
                for env in (g, o):
                    env.step_synthetic(1, 1)

    def steps(k, per_launch=1):
        for env in (g, o):
            env.step_synthetic(k, per_launch)

    g.set_step_mode(True); steps(5); both("resident")
    g.set_step_mode(False); steps(1); both("single-step launches")
    steps(17, 8); both("8 steps per launch")
    g.set_step_mode(True); steps(3); both("resident again")
    # the closed pilot loop steps by launch; the oracle has no pilot: it is given the loop's controls
    g.pilot_load(make_weights(h, w, seed=5))
    for k in range(3):
        g.step_pilot(1)
        o.step(g.fetch("ctl_steer"), g.fetch("ctl_thr"), g.fetch("ctl_brk"))
    both("trs_step_pilot")
    for env in (g, o):
        env.set_frame_filter(STATIC)
    steps(3); both("static filter on")
    for env in (g, o):
        env.set_frame_filter(DYNAMIC)
    steps(3); both("dynamic brightness on")
    for env in (g, o):
        env.set_frame_filter(enabled=False)
    steps(1); both("dynamic brightness off")
    lp = params_for(n, 2)
    g.set_lighting(lp); steps(3); both("lighting on", lit=lp)
    g.set_lighting(None); steps(1); both("lighting off")
    g.set_step_mode(False)
    g.set_lighting(lp); steps(1); g.set_lighting(None); steps(1); both("one lit launch between plain ones")
    g.set_camera(0.5, 0.5, 0.0); steps(3)                              # (lens frames: tests/test_lens_gpu.py; here what follows them)
    g.set_camera(None); steps(1); both("lens off, launches")
    g.set_step_mode(True)
    g.set_camera(0.0, 0.0, 0.2); steps(3)
    g.set_camera(None); steps(1); both("lens off, resident")
    g.set_step_mode(False)
    for env in (g, o):
        env.set_frame_filter(DYNAMIC)
    steps(2)
    for env in (g, o):
        env.set_frame_filter(enabled=False)
    steps(4, 3); both("dynamic brightness, then several steps per launch")
    assert_state_equal(g, o, "at the end")
