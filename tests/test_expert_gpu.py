"""The scripted expert on the GPU (trs_set_expert, trs_expert_act, trs_step_expert; include/trsim_spec.h, "scripted expert") against the numpy restatement
of tests/test_expert_cpu.py, bit for bit: the pure rule at every wave shape, its edges, the closed loop with the disturbance keyed by the global env id, the
capture of (frame, row) records into device memory, and how the loop composes with trs_step, latency and resident mode.  Frames are 8 x 8 or absent."""

import numpy as np
import pytest

from test_expert_cpu import DEFAULTS, Driver, F, expert_row, expert_rule, track_yaw_of

pytestmark = pytest.mark.gpu

STATE = ("pos_x", "pos_y", "pos_z", "yaw", "vel", "speed", "cte", "seg_idx", "done", "ep_return", "ep_len")
SMALL = dict(img_h=8, img_w=8)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def truth(env):
    return env.fetch("seg_idx"), env.fetch("yaw"), env.fetch("cte"), env.fetch("speed")


def acted(env, n=None):
    return [env.to_host(o) for o in env.expert_act(n)]


def assert_same_state(a, b, image=True):
    for name in STATE:
        assert same(a.fetch(name), b.fetch(name)), name
    if image:
        assert np.array_equal(a.fetch("img"), b.fetch("img"))


# ---- act ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track", ["generated_track", "mountain_track"])
@pytest.mark.parametrize("n", [1, 3, 65, 130])      # a single thread, a partial wave, one wave plus one thread, a partial second workgroup of waves
def test_act_equals_the_restatement(make_env, n, track):
    env = make_env("hip", n_envs=n, track=track, render=False, auto_reset=True)
    env.step_synthetic(12, 1)
    env.set_expert()
    ty = track_yaw_of(env.fetch("tangent"))
    want = expert_rule(*truth(env), ty)
    got = acted(env)
    for g, w, name in zip(got, want, ("steering", "throttle", "breaking")):
        assert same(g, w), name
    assert np.any(want[0] != 0) or n == 1
    if n > 1:                                       # n < n_envs: the first n cars
        for g, w in zip(acted(env, n - 1), want):
            assert same(g, w[:n - 1])
    before = [env.fetch(k) for k in STATE]
    acted(env)                                      # the pure rule moves nothing: not the state, not the driver
    assert all(same(a, env.fetch(k)) for a, k in zip(before, STATE))


# ---- edges -------------------------------------------------------------------------------------------------------------------------------------------------
def test_edges_of_the_rule(make_env):
    n = 6
    env = make_env("hip", n_envs=n, track="generated_track", render=False)
    pts, np_ = env.track, env.n_points
    tan = env.fetch("tangent")
    ty = track_yaw_of(tan)
    look = DEFAULTS["look"]
    neg = int(np.flatnonzero((np.roll(ty, -look) < -0.5) & (np.arange(np_) < np_ - 50) & (np.arange(np_) > 50))[0])    # track_yaw[p + look] < -0.5
    pos = int(np.flatnonzero((np.roll(ty, -look) > 0.5) & (np.arange(np_) < np_ - 50) & (np.arange(np_) > 50))[0])
    mid = np_ // 2
    at = np.array([np_ - 3, neg, pos, mid, mid + 40, mid + 80])
    x, y, z = (pts[at, k].astype(F) for k in range(3))
    yaw = ty[at].copy()
    yaw[1] = ty[(neg + look) % np_] + F(np.pi) + F(0.3)          # yaw - track_yaw[j] beyond +pi (yaw itself stays below pi)
    yaw[2] = ty[(pos + look) % np_] - F(np.pi) - F(0.3)          # ... and beyond -pi
    x[3] += F(2.5) * tan[mid, 1]; z[3] -= F(2.5) * tan[mid, 0]   # 2.5 units to the right of the centre line: cte = +2.5
    v = np.array([3, 0, 0, 3, 5, 5], F)
    env.step(0.0, 0.0, 0.0)                                      # the placing step
    env.set_pose(x, y, z, yaw, v)
    env.step(0.0, 0.0, 0.0)                                      # one step with zero controls: cte and the index belong to the pose
    seg, yaw_t, cte, speed = truth(env)
    assert not env.fetch("done").any()
    j = (seg + look) % np_
    assert seg[0] + look >= np_ and j[0] < look                  # the index wraps
    assert yaw_t[1] - ty[j[1]] > np.pi and yaw_t[2] - ty[j[2]] < -np.pi
    assert 2.0 < cte[3] < 3.0
    target = np.array([8, 8, 8, 8, speed[4], 8], F)              # env 4: speed == v_ref exactly
    profile = np.full(np_, 100, F)
    profile[j[5]] = 2.0                                          # env 5: the profile undercuts its target at its look-ahead point
    env.set_expert(target_speed=target, profile=profile)
    want = expert_rule(seg, yaw_t, cte, speed, ty, None, target, profile)
    got = acted(env)
    for g, w, name in zip(got, want, ("steering", "throttle", "breaking")):
        assert same(g, w), (name, g, w)
    st, th, br = got
    assert st[1] == F(1) and st[2] == F(-1)                      # the wrapped errors are -(pi - 0.3) and +(pi - 0.3): without the wrap the locks would be the other way round
    assert st[3] == F(-1)                                        # clamped
    assert th[4] == F(0.1) and br[4] == 0                        # strict <: at the target the throttle is low
    assert th[0] == F(0.6) and th[3] == F(0.6) and br[0] == 0
    assert th[5] == F(0.1) and br[5] == F(0.5)                   # 4.86 > 2 * 1.15
    # refusals leave the expert as it is
    with pytest.raises(RuntimeError, match="look"):
        env.set_expert(look=np_)
    with pytest.raises(RuntimeError, match="look"):
        env.set_expert(look=-1)
    assert same(acted(env)[0], want[0])
    with pytest.raises(RuntimeError, match="camera"):
        env.step_expert(1, {"capacity": 1, "rows": env.scratch(20, (n, 8)), "frames": env.scratch(21, (n, 8, 8, 3), np.uint8)})
    with pytest.raises(RuntimeError, match="every"):
        env.step_expert(1, {"every": 0, "capacity": 1, "rows": env.scratch(20, (n, 8))})
    with pytest.raises(RuntimeError, match="n_steps"):
        env.step_expert(0)
    assert env.counters()[2] == 2                                # no refused call stepped
    env.load_track("generated_track")                            # a new track switches the expert off
    with pytest.raises(RuntimeError, match="no expert set"):
        env.expert_act()
    with pytest.raises(RuntimeError, match="no expert set"):
        env.step_expert(1)
    env.set_expert()
    env.set_expert(False)
    with pytest.raises(RuntimeError, match="no expert set"):
        env.expert_act()


# ---- loop --------------------------------------------------------------------------------------------------------------------------------------------------
def rows_of(env, ticks, **kw):
    """(rows [ticks, n, 8], captured) of one step_expert(ticks) call that captures every tick's row."""
    import torch
    d_rows = torch.zeros((ticks, env.n, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = env.step_expert(ticks, dict({"every": 1, "skip": 0, "capacity": ticks, "rows": d_rows}, **kw))
    env.sync()
    return d_rows.cpu().numpy(), got


def test_the_loop_applies_the_disturbed_rule_and_is_keyed_by_the_global_env_id(make_env):
    n, ticks, cfg = 65, 16, {"sigma": 1.5}
    kw = dict(track="generated_track", auto_reset=True, **SMALL)
    a = make_env("hip", n_envs=n, **kw)
    a.set_expert(**cfg)
    ty = track_yaw_of(a.fetch("tangent"))
    drv = Driver(n, cfg)
    rows = []
    for t in range(ticks):
        seg, yaw, cte, speed = truth(a)
        done = a.fetch("done")
        steer, thr, brk = expert_rule(seg, yaw, cte, speed, ty, cfg)
        applied = drv.applied(steer)
        rows.append(expert_row(steer, thr, brk, applied, speed, cte, seg, done, a.n_points))
        assert a.step_expert(1) == 0
        assert same(a.fetch("ctl_steer"), applied) and same(a.fetch("ctl_thr"), thr) and same(a.fetch("ctl_brk"), brk), t
    assert np.any(np.stack(rows)[:, :, 0] != np.stack(rows)[:, :, 3])        # the disturbance is there
    b = make_env("hip", n_envs=n, **kw)                                     # the same 16 ticks in one call
    b.set_expert(**cfg)
    b_rows, got = rows_of(b, ticks)
    assert got == ticks and same(b_rows, np.stack(rows))
    assert_same_state(a, b)
    parts = []                                                               # 32 + 33 envs: the generator is keyed by the global id
    for base, m in ((0, 32), (32, 33)):
        s = make_env("hip", n_envs=m, env_id_base=base, **kw)
        s.set_expert(**cfg)
        parts.append(rows_of(s, ticks)[0])
    assert same(np.concatenate(parts, axis=1), b_rows)


# ---- capture -----------------------------------------------------------------------------------------------------------------------------------------------
def test_collect_equals_records_gathered_by_hand(make_env):
    import torch
    n, cfg = 3, {"sigma": 1.5}
    kw = dict(n_envs=n, track="mountain_track", **SMALL)
    a, twin = make_env("hip", **kw), make_env("hip", **kw)
    for env in (a, twin):
        env.set_expert(**cfg)
    frames, rows = a.collect(ticks=23, every=5, skip=3, to_host=True)
    want_f, want_r = [], []
    for k in range(23):
        due = k >= 3 and (k - 3) % 5 == 0
        if due:
            label = acted(twin)
            img, state = twin.fetch("img"), [twin.fetch(name) for name in ("speed", "cte", "seg_idx", "done")]
        assert twin.step_expert(1) == 0
        if due:
            assert same(twin.fetch("ctl_thr"), label[1]) and same(twin.fetch("ctl_brk"), label[2])
            want_f.append(img)
            want_r.append(expert_row(*label, twin.fetch("ctl_steer"), *state, twin.n_points))
    assert len(want_r) == 4 and rows.shape == (4 * n, 8) and frames.shape == (4 * n, 8, 8, 3)
    assert same(rows, np.concatenate(want_r)) and np.array_equal(frames, np.concatenate(want_f))
    assert np.any(rows[:, 0] != rows[:, 3]) and np.all(rows[n:, 4] > 0)
    assert_same_state(a, twin)
    # a capacity smaller than the due ticks: two slots are filled, not a byte behind them is touched
    c = make_env("hip", **kw)
    c.set_expert(**cfg)
    d_rows = torch.full((4, n, 8), float("nan"), dtype=torch.float32, device="cuda")
    d_frames = torch.full((4, n, 8, 8, 3), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert c.step_expert(23, {"every": 5, "skip": 3, "capacity": 2, "rows": d_rows, "frames": d_frames}) == 2
    c.sync()
    h_rows, h_frames = d_rows.cpu().numpy(), d_frames.cpu().numpy()
    assert same(h_rows[:2].reshape(-1, 8), rows[:2 * n]) and np.array_equal(h_frames[:2].reshape(-1, 8, 8, 3), frames[:2 * n])
    assert np.all(np.isnan(h_rows[2:])) and np.all(h_frames[2:] == 0xA5)
    assert_same_state(c, a)                                  # the capture changes nothing the cars do


def test_a_tick_without_a_frame_is_not_captured(make_env):
    seen = make_env("hip", n_envs=2, **SMALL)
    seen.set_expert()
    frames, rows = seen.collect(ticks=6, every=5, skip=0, to_host=True)      # k = 0 has no frame yet; k = 5 has
    assert rows.shape == (2, 8) and frames.shape == (2, 8, 8, 3)
    blind = make_env("hip", n_envs=2, render=False)
    blind.set_expert()
    frames, rows2 = blind.collect(ticks=6, every=5, skip=0, to_host=True)    # rows alone: both ticks
    assert frames is None and rows2.shape == (4, 8) and np.all(rows2[2:, 4] > 0)
    assert np.all(rows2[:2, 4:6] == 0)                                       # the start pose: speed 0, cte 0


# ---- composition -------------------------------------------------------------------------------------------------------------------------------------------
def test_without_disturbance_the_loop_is_act_then_step(make_env):
    kw = dict(n_envs=5, track="generated_track", **SMALL)
    a, twin = make_env("hip", **kw), make_env("hip", **kw)
    for env in (a, twin):
        env.set_expert()
    a.step_expert(8)
    for _ in range(8):
        st, th, br = twin.expert_act()
        twin.step_device(*[o.__cuda_array_interface__["data"][0] for o in (st, th, br)])
    assert_same_state(a, twin)
    assert same(a.fetch("ctl_steer"), twin.to_host(st))


def test_with_a_latency_the_expert_still_acts_on_the_truth(make_env):
    kw = dict(n_envs=4, track="generated_track", **SMALL)
    a, late = make_env("hip", **kw), make_env("hip", **kw)
    late.set_latency([0, 1, 3, 3])
    for env in (a, late):
        env.set_expert(sigma=1.5)
    for t in range(10):
        a.step_expert(1), late.step_expert(1)
        for name in ("ctl_steer", "ctl_thr", "ctl_brk"):
            assert same(a.fetch(name), late.fetch(name)), (t, name)
    assert_same_state(a, late)
    assert late.observation()[7].tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("kw", [dict(n_envs=9, render=False), dict(n_envs=5)], ids=["physics", "camera"])
def test_in_resident_mode_the_call_succeeds_and_equals_launch_mode(make_env, kw):
    a, r = make_env("hip", **kw), make_env("hip", **kw)
    r.set_step_mode(True)
    for env in (a, r):
        env.step_synthetic(3, 1)                             # (r: posted to the worker, which the expert then asks to leave)
        env.set_expert(sigma=1.5)
        env.step_expert(8)
    assert r.step_mode()[0] == "resident"
    assert_same_state(a, r, image=bool(kw.get("render", True)))
    for name in ("ctl_steer", "ctl_thr", "ctl_brk"):
        assert same(a.fetch(name), r.fetch(name)), name


# ---- drive -------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_expert_stays_on_the_mountain_track(make_env):
    """64 cars x 600 ticks with the disturbance: no off-track event (the oracle run of tests/test_expert_cpu.py leaves no car within 1e-3 of the threshold,
    so a pose difference of 1e-5 cannot flip one)."""
    env = make_env("hip", n_envs=64, track="mountain_track", render=False, auto_reset=True)
    env.set_expert(sigma=1.5)
    env.step_expert(600)
    assert int(env.fetch("stats")[0]) == 0
    assert env.fetch("speed").min() > 4 and np.abs(env.fetch("cte")).max() < 1.0


# ---- the part ------------------------------------------------------------------------------------------------------------------------------------------------
def test_scripted_driver_part_feeds_the_gym_interfaces(make_env):
    from triton_racer_sim_amd.components import BatchedGymInterface, HipGymInterface, HipScriptedDriver
    one = HipGymInterface(gym_config={"img_w": 8, "img_h": 8})
    drv = HipScriptedDriver(one, target_speed=5.0)
    assert drv.step_outputs == ["usr/steering", "usr/throttle", "usr/breaking"] and drv.step_inputs == []
    one.step(0.0, 0.0, 0.0, False)
    ty = track_yaw_of(one.env.fetch("tangent"))
    for _ in range(3):
        out = drv.step()
        want = expert_rule(*truth(one.env), ty, {"target_speed": 5.0})
        assert all(isinstance(o, float) for o in out) and [F(o) for o in out] == [w[0] for w in want]
        one.step(*out, False)
    one.onShutdown()
    many = BatchedGymInterface(3, gym_config={"img_w": 8, "img_h": 8})
    drv = HipScriptedDriver(many)
    many.step(0.0, 0.0, 0.0, None)
    out = drv.step()                                         # device handles: the gym interface takes them as they are
    want = expert_rule(*truth(many.env), track_yaw_of(many.env.fetch("tangent")))
    assert all(same(many.env.to_host(o), w) for o, w in zip(out, want))
    many.step(*out, None)
    assert int(many.env.counters()[2]) == 2
    many.onShutdown()
