"""The pilot in the loop with the expert's labels without a GPU (include/trsim_spec.h, "pilot in the loop with the expert's labels"; trs_step_dagger): a
numpy float32 restatement of the gate, of one tick and of the stats, written from the spec text; the gate's properties (never / always, blocks of `hold`
ticks, keyed by the global env id, its share of expert ticks); the CPU oracle driven with the restatement and a biased stand-in pilot; and the host side of
the library (triton-racer-sim_amd/csrc/trsim_expert.hpp through tests/dagger_driver.cpp: host compiler, AddressSanitizer + UBSan) against the restatement.
tests/test_dagger_gpu.py imports the restatement and compares trs_step_dagger with it bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_expert_cpu import Driver, F, expert_rule, splitmix_u, track_yaw_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(beta=0.5, hold=1, expert_speed=1, seed=0)
STATS = ("ticks", "expert_ticks", "sum_abs_cte", "max_abs_cte", "sum_abs_steering_diff", "done_ticks")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def gate_u(seed, gid, k, hold):
    """u of the block k // hold for the global env ids `gid`."""
    return splitmix_u(seed, np.asarray(gid, np.uint64), int(k) // int(hold))


def gate(seed, gid, k, hold, beta):
    """True where the expert drives: u < beta in binary32."""
    return gate_u(seed, gid, k, hold) < F(beta)


def dagger_tick(pilot, label, drives, expert_speed=True):
    """The applied (steering, throttle, brake) of one tick from the pilot's controls, the expert's label and the gate."""
    (ps, pt, pb), (es, et, eb) = [[np.asarray(a, F) for a in t] for t in (pilot, label)]
    steer = np.where(drives, es, ps)
    if expert_speed:
        return steer, et, eb
    return steer, np.where(drives, et, pt), np.where(drives, eb, pb)


class Stats:
    """float32 [n, 6]: one binary32 operation per field and tick, in tick order."""

    def __init__(self, n):
        self.a = np.zeros((n, 6), F)

    def update(self, drives, cte, ps, es, done):
        a, one = self.a, F(1)
        acte = np.abs(np.asarray(cte, F))
        a[:, 0] = a[:, 0] + one
        a[:, 1] = a[:, 1] + np.where(drives, one, F(0))
        a[:, 2] = a[:, 2] + acte
        a[:, 3] = np.maximum(a[:, 3], acte)
        a[:, 4] = a[:, 4] + np.abs(np.asarray(ps, F) - np.asarray(es, F))
        a[:, 5] = a[:, 5] + np.where(np.asarray(done) != 0, one, F(0))
        assert a.dtype == np.float32


# ---- the gate ------------------------------------------------------------------------------------------------------------------------------------------
def gates(n, ticks, base, hold, beta, seed=0):
    gid = np.arange(n) + base
    return np.stack([gate(seed, gid, k, hold, beta) for k in range(ticks)])          # [ticks, n]


def test_beta_zero_is_never_and_beta_one_is_always_the_expert():
    for base in (0, 5, 1024):
        for hold in (1, 8):
            assert not gates(64, 256, base, hold, 0.0).any()
            assert gates(64, 256, base, hold, 1.0).all()
    u = np.stack([gate_u(0, np.arange(4096), k, 1) for k in range(64)])
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() <= F(1) - F(2.0 ** -24)   # u <= 1 - 2^-24 < 1: beta = 1 is always


def test_the_gate_holds_over_blocks_and_is_keyed_by_the_global_env_id():
    g = gates(64, 256, 0, 8, 0.5)
    blocks = g.reshape(32, 8, 64)
    assert np.all(blocks == blocks[:, :1])                                         # constant over blocks of `hold` ticks
    assert np.array_equal(blocks[:, 0], gates(64, 32, 0, 1, 0.5))                   # block b of hold 8 is tick b of hold 1: the key is k // hold
    assert np.any(blocks[1:, 0] != blocks[:-1, 0])
    big = gates(1024 + 64, 40, 0, 3, 0.5)
    assert np.array_equal(gates(64, 40, 1024, 3, 0.5), big[:, 1024:])               # a shard at base 1024 = rows 1024.. of one big run
    assert np.array_equal(gates(59, 40, 5, 3, 0.5), big[:, 5:64])                   # env_id_base + e only
    assert np.any(gates(64, 40, 0, 3, 0.5, seed=1) != big[:, :64])                  # the seed is the dagger config's


@pytest.mark.parametrize("beta", [0.25, 0.5])
@pytest.mark.parametrize("hold", [1, 8])
@pytest.mark.parametrize("base", [0, 5, 1024])
def test_the_share_of_expert_ticks_is_beta(base, hold, beta):
    """64 envs x 256 ticks, seed 0.  The share of expert ticks lies within 0.015 of beta (the restatement gives 0.2402 to 0.2534 and 0.4926 to 0.5021 over
    these cases) and every env sees both drivers."""
    g = gates(64, 256, base, hold, beta)
    share = float(g.mean())
    print(f"base {base} hold {hold} beta {beta}: share of expert ticks {share:.4f}")
    assert abs(share - beta) <= 0.015
    assert g.any(axis=0).all() and (~g).any(axis=0).all()


# ---- the restatement drives the oracle --------------------------------------------------------------------------------------------------------------------
def drive_oracle(make_env, beta, hold=1, expert_speed=True, n=16, ticks=200, base=0, seed=0):
    """The oracle under the restated loop with a biased stand-in pilot: steering clamp(label + 0.3), throttle 0.3, brake 0.  Returns the stats, the per-tick
    records the stats are made of and the final state."""
    env = make_env("oracle", n_envs=n, track="generated_track", render=False, auto_reset=True, env_id_base=base)
    ty = track_yaw_of(env.fetch("tangent"))
    gid = np.arange(n) + base
    stats, rec = Stats(n), []
    for k in range(ticks):
        seg, yaw, cte, speed, done = (env.fetch(name) for name in ("seg_idx", "yaw", "cte", "speed", "done"))
        label = expert_rule(seg, yaw, cte, speed, ty)
        pilot = (np.clip(label[0] + F(0.3), F(-1), F(1)), np.full(n, 0.3, F), np.zeros(n, F))
        drives = gate(seed, gid, k, hold, beta)
        applied = dagger_tick(pilot, label, drives, expert_speed)
        stats.update(drives, cte, pilot[0], label[0], done)
        rec.append((drives, np.abs(cte), np.abs(pilot[0] - label[0]), done != 0, applied))
        env.step(*applied)
    state = {name: env.fetch(name) for name in ("pos_x", "pos_z", "yaw", "speed", "cte", "seg_idx")}
    return stats.a, rec, state


@pytest.mark.parametrize("expert_speed", [True, False])
def test_stats_equal_a_recomputation_by_hand(make_env, expert_speed):
    got, rec, _ = drive_oracle(make_env, 0.5, hold=4, expert_speed=expert_speed)
    drives, acte, diff, done = (np.stack([r[i] for r in rec]) for i in range(4))   # [ticks, n]
    assert np.array_equal(got[:, 0], np.full(16, 200, F))
    assert np.array_equal(got[:, 1], drives.sum(0).astype(F)) and np.array_equal(got[:, 5], done.sum(0).astype(F))   # counts: exact
    assert np.array_equal(got[:, 3], acte.max(0))
    for col, terms in ((2, acte), (4, diff)):                                      # sums: binary32 additions in tick order
        want = np.zeros(16, F)
        for t in range(200):
            want = (want.astype(np.float64) + terms[t].astype(np.float64)).astype(F)   # one rounding per addition (a binary64 sum of two binary32 rounds the same way)
        assert np.array_equal(got[:, col].view(np.uint32), want.view(np.uint32)), col
        assert np.array_equal(want, np.cumsum(terms, axis=0, dtype=F)[-1])
    assert 0 < got[:, 1].min() and got[:, 1].max() < 200 and np.all(got[:, 4] > 0)   # both drivers held the wheel, and the pilot is biased
    throttle = np.stack([r[4][1] for r in rec])
    assert np.any(throttle == F(0.3)) != expert_speed                             # the pilot's own throttle reaches the car only with expert_speed = 0


def test_at_beta_one_the_trajectory_is_the_experts(make_env):
    got, rec, state = drive_oracle(make_env, 1.0)
    assert np.array_equal(got[:, 1], got[:, 0]) and np.all(got[:, 4] > 0)          # the expert drove every tick; the pilot's disagreement is still counted
    env = make_env("oracle", n_envs=16, track="generated_track", render=False, auto_reset=True)
    ty, drv = track_yaw_of(env.fetch("tangent")), Driver(16, {"sigma": 0.0})
    for _ in range(200):
        steer, thr, brk = expert_rule(env.fetch("seg_idx"), env.fetch("yaw"), env.fetch("cte"), env.fetch("speed"), ty)
        env.step(drv.applied(steer), thr, brk)
    for name, want in state.items():
        assert np.array_equal(env.fetch(name), want), name
    biased = drive_oracle(make_env, 0.0)[2]
    assert np.any(biased["pos_x"] != state["pos_x"])                                # ... and at beta = 0 it is not


# ---- the host side of the library ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("dagger") / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "dagger_driver.cpp")])
    return str(exe)


def run(driver, *args):
    out = subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return out.stdout


def test_host_gate_equals_the_restatement(driver):
    rng = np.random.default_rng(11)
    cases = [(0, 0, 0, 1, 0.5), (0, 5, 11, 1, 0.5), (0, 1024, 255, 8, 0.25), (2 ** 64 - 1, 2 ** 31 - 1, 2 ** 32 - 1, 1, 1.0), (7, 3, 9, 4, 0.0),
             (0x5EED, 2 ** 31 + 5, 17, 3, 0.75)]
    cases += [(int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 32)), int(rng.integers(1, 50)), float(F(rng.uniform())))
              for _ in range(200)]
    lines = run(driver, "gate", *[repr(v) if isinstance(v, float) else v for c in cases for v in c]).split("\n")[:-1]
    assert len(lines) == len(cases)
    seen = set()
    for (seed, gid, k, hold, beta), line in zip(cases, lines):
        u_bits, drives = line.split()
        want_u = gate_u(seed, [gid], k, hold)
        assert int(u_bits, 16) == int(want_u.view(np.uint32)[0]), (seed, gid, k, hold)
        assert int(drives) == int(gate(seed, [gid], k, hold, beta)[0]), (seed, gid, k, hold, beta)
        seen.add(int(drives))
    assert seen == {0, 1}


def test_config_refusals_and_defaults(driver):
    from triton_racer_sim_amd import _ffi
    import ctypes
    ok = [(0.0, 1, 0, 0), (1.0, 1, 1, 0), (0.5, 2 ** 31 - 1, 1, 0)]
    assert run(driver, "config", *[v for c in ok for v in c]).split() == ["ok"] * 3
    bad = [(("nan", 1, 1, 0), "beta"), (("inf", 1, 1, 0), "beta"), ((-0.001, 1, 1, 0), "beta"), ((1.001, 1, 1, 0), "beta"),
           ((0.5, 0, 1, 0), "hold"), ((0.5, -3, 1, 0), "hold"), ((0.5, 1, 2, 0), "expert_speed"), ((0.5, 1, -1, 0), "expert_speed"),
           ((0.5, 1, 1, 4), "struct_size"), ((0.5, 1, 1, -8), "struct_size")]
    lines = run(driver, "config", *[v for c, _ in bad for v in c]).split("\n")[:-1]
    assert len(lines) == len(bad)
    for (case, word), line in zip(bad, lines):
        assert word in line and line != "ok", (case, line)
    got = dict(line.split() for line in run(driver, "defaults").splitlines())
    assert got.pop("null") == "refused"
    assert int(got.pop("struct_size")) == ctypes.sizeof(_ffi.TrsDaggerConfig) == 24
    assert set(got) == set(DEFAULTS)
    for k, v in DEFAULTS.items():
        assert F(got[k]) == F(v), k
    assert _ffi.DAGGER_STATS == STATS


def test_the_oracle_has_no_dagger_loop(make_env):
    from triton_racer_sim_amd import _ffi
    assert _ffi.DAGGER_SYMBOLS == ["default_dagger_config", "step_dagger", "dagger_stats"]
    assert all(s in _ffi.PILOT_SYMBOLS and s not in _ffi.SYMBOLS for s in _ffi.DAGGER_SYMBOLS)
    o = make_env("oracle", n_envs=2, render=False)
    assert not o.api.has_dagger
    with pytest.raises(RuntimeError, match="oracle has no"):
        o.step_dagger(1)
    with pytest.raises(RuntimeError, match="oracle has no"):
        o.dagger_stats()
