"""Observation latency without a GPU: the ring arithmetic of triton-racer-sim_amd/csrc/trsim_plan.hpp (ObsRing, through tests/latency_driver.cpp:
host compiler, AddressSanitizer + UBSan) against a deque model of HipGymInterface's delay line, the bytes of the rings (obs_bytes) against the same sums here, the ms -> ticks rule of BatchedGymInterface, and the
oracle's function table, which has no observation latency."""
import collections
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 200


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("latency") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "latency_driver.cpp")])
    return str(exe)


def ring(driver, max_ticks, steps, ticks):
    out = subprocess.run([driver, "ring", str(max_ticks), str(steps), *[str(t) for t in ticks]], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    rows = [line.split(" ") for line in out.stdout.splitlines()]
    slots = int(rows[0][1])
    step = {int(r[1]): (int(r[2]), int(r[3])) for r in rows if r[0] == "step"}
    obs = {(int(r[1]), int(r[2])): (int(r[3]), int(r[4])) for r in rows if r[0] == "obs"}
    return slots, step, obs


@pytest.mark.parametrize("max_ticks", range(1, 31))
def test_ring_slots_deliver_the_delay_lines_record_and_the_next_step_never_lands_on_one(driver, max_ticks):
    rng = np.random.default_rng(100 + max_ticks)
    ticks = [0, max_ticks] + [int(t) for t in rng.integers(0, max_ticks + 1, 6)]
    slots, step, obs = ring(driver, max_ticks, STEPS, ticks)
    assert slots == max_ticks + 2
    mem = [0] * slots                                        # what each slot holds: the step that rendered into it, 0 = the zeros the history began with
    lines = [collections.deque() for _ in ticks]             # HipGymInterface's delay line per env (components.py)
    for T in range(0, STEPS + 1):
        if T >= 1:
            assert 0 <= step[T][0] < slots
            assert step[T][0] == step[T - 1][1]              # "slot of step T + 1" as seen from T is where step T + 1 goes
            mem[step[T][0]] = T
        for e, L in enumerate(ticks):
            told = 0                                         # the constructor's state
            if T >= 1:
                lines[e].append(T)
                if L == 0:
                    told = lines[e].popleft()
                elif len(lines[e]) > L:
                    told = lines[e].popleft()
            arrived, slot = obs[(T, e)]
            assert arrived == (1 if told else 0), (T, e, L)
            assert 0 <= slot < slots
            assert mem[slot] == told, (T, e, L, slot)        # the slot the view points into holds the delay line's record (or still zeros)
            assert slot != step[T][1], (T, e, L)             # and step T + 1 does not render into it: the view stays intact while the next step runs


def test_ring_driver_refuses_a_ring_outside_the_abi(driver):
    for bad in (0, 31):
        assert subprocess.run([driver, "ring", str(bad), "3", "0"], capture_output=True).returncode == 2


@pytest.mark.parametrize("n,h,w,depth,render,max_ticks", [(1, 2, 4, 0, 1, 1), (5, 30, 44, 1, 1, 3), (1281, 16, 24, 0, 1, 30), (7, 120, 160, 1, 0, 2),
                                                          (65536, 240, 320, 1, 1, 30)])     # the last one's frame ring is past 4 GiB: nothing is computed in int
def test_ring_bytes_are_the_sums_trs_set_latency_allocates(driver, n, h, w, depth, render, max_ticks):
    out = subprocess.run([driver, "bytes", *[str(v) for v in (n, h, w, depth, render, max_ticks)]], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    got = {k: int(v) for k, v in (line.split(" ") for line in out.stdout.splitlines())}
    up256 = lambda b: (b + 255) // 256 * 256
    slots = max_ticks + 2
    img_env = h * w * 3 if render else 0
    dep_env = h * w * 4 if render and depth else 0
    want = {"img_env": img_env, "dep_env": dep_env, "img_stride": up256(n * img_env), "dep_stride": up256(n * dep_env),
            "ring_img": slots * up256(n * img_env), "ring_dep": slots * up256(n * dep_env),
            "ring_tel": slots * 6 * n * 4, "tel": 6 * n * 4, "flag": 2 * n, "ticks": n * 4}
    assert got == want
    if n == 65536:
        assert got["ring_img"] > 2**32 and got["img_stride"] > 2**31


def test_sim_latency_becomes_ticks_by_the_one_car_rule():
    from triton_racer_sim_amd.components import sim_latency_ticks
    for ms in (0, 1, 49, 50, 51, 100, 120, 150, 333.3, 1500):
        for hz in (20, 10, 60):
            want = int(math.ceil(float(ms) * float(hz) / 1000.0)) if ms else 0     # HipGymInterface.__init__
            assert sim_latency_ticks(ms, hz).tolist() == [want]
            assert sim_latency_ticks(ms, hz, n=4).tolist() == [want] * 4
    assert sim_latency_ticks(120).tolist() == [3] and sim_latency_ticks(None).tolist() == [0]
    got = sim_latency_ticks([0, 50, 51, 120, 300], 20, n=5)
    assert got.dtype == np.int32 and got.tolist() == [0, 1, 2, 3, 6]
    with pytest.raises(ValueError):
        sim_latency_ticks([0, 50], 20, n=5)
    with pytest.raises(ValueError):
        sim_latency_ticks(-1)


def test_the_oracle_has_no_observation_latency(make_env):
    from triton_racer_sim_amd import _ffi
    assert _ffi.LATENCY_SYMBOLS == ["set_latency", "get_latency", "get_observation", "fetch_observation"]
    assert all(s in _ffi.PILOT_SYMBOLS and s not in _ffi.SYMBOLS for s in _ffi.LATENCY_SYMBOLS)
    o = make_env("oracle", n_envs=2, render=False)
    assert not o.api.has_latency
    with pytest.raises(RuntimeError, match="oracle has no observation latency"):
        o.set_latency(2)
    with pytest.raises(RuntimeError, match="oracle has no observation latency"):
        o.set_latency(None)
