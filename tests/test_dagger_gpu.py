"""The pilot in the loop with the expert's labels on the GPU (trs_step_dagger, trs_dagger_stats; include/trsim_spec.h, "pilot in the loop with the expert's
labels").  The reference is always a composition of calls that existed before it — trs_pilot_act for the pilot's controls, the numpy restatement of the
expert's rule (tests/test_expert_cpu.py) on the fetched truth, the restated gate, tick and stats (tests/test_dagger_cpu.py), trs_step_host for the step,
trs_jpeg_roundtrip and trs_get_observation for the frame the pilot is fed — never the new call; everything is compared bit for bit.  Frames are 120 x 160,
the pilot is the trained fixture (tests/golden/pilot_trained_120x160.npz)."""

import numpy as np
import pytest

from test_dagger_cpu import STATS, Stats, dagger_tick, gate
from test_expert_cpu import F, expert_row, expert_rule, track_yaw_of
from test_pilot_trained import H, W, trained_weights

pytestmark = pytest.mark.gpu

STATE = ("pos_x", "pos_y", "pos_z", "yaw", "vel", "speed", "cte", "seg_idx", "done", "ep_return", "ep_len")
PCFG = {"spd_ctl_threshold": 1.1, "spd_ctl_reverse_multiplier": 1.0}
CTL = ("ctl_steer", "ctl_thr", "ctl_brk")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def assert_same_state(a, b):
    for name in STATE:
        assert same(a.fetch(name), b.fetch(name)), name
    assert np.array_equal(a.fetch("img"), b.fetch("img"))


@pytest.fixture(scope="module")
def weights():
    return trained_weights()


def make(make_env, weights, n, base=0, expert=True, **kw):
    env = make_env("hip", n_envs=n, img_h=H, img_w=W, env_id_base=base, auto_reset=True, **kw)
    env.pilot_load(weights)
    if expert:
        env.set_expert()
    return env


def dev_np(env, handle):
    return env.to_host(handle)


class Reference:
    """One tick of the spec paragraph on a twin env from calls that existed before trs_step_dagger.  `k` is the driver's counter the twin would have."""

    def __init__(self, env, base=0, codec=None, late=False, **dagger):
        import torch
        self.env, self.k, self.codec, self.late = env, 0, codec, late
        self.d = dict(dict(beta=0.5, hold=1, expert_speed=True, seed=0), **dagger)
        self.gid = np.arange(env.n) + base
        self.ty = track_yaw_of(env.fetch("tangent"))
        self.stats = Stats(env.n)
        self.codec_buf = torch.empty((env.n, H, W, 3), dtype=torch.uint8, device="cuda") if codec else None
        torch.cuda.synchronize()

    def pilot(self):
        """(controls, fed frame or None) of trs_pilot_act on what trs_step_pilot would read now; two calls must agree in bits."""
        import torch
        env = self.env
        if env.counters()[2] == 0:                               # no frame yet: (0, 0, 0)
            return [np.zeros(env.n, F) for _ in range(3)], None
        frames, kw = None, {}
        if self.late:
            frames = env.device_observation("img")
            arrived = torch.as_tensor(env.device_observation("arrived"), device="cuda")
            self.mode = torch.where(arrived != 0, 2, 0).to(torch.uint8)               # AI where the observation has arrived, else HUMAN
            torch.cuda.synchronize()
            kw = dict(speed=env.device_observation("speed"), mode=self.mode)
        fed = dev_np(env, frames) if frames is not None else env.fetch("img")
        if self.codec:
            frames = env.device_jpeg_roundtrip(frames, quality=self.codec, d_dst=self.codec_buf)
            fed = dev_np(env, frames)
        first = [dev_np(env, o) for o in env.pilot_act_device(frames=frames, cfg=PCFG, **kw)]
        again = [dev_np(env, o) for o in env.pilot_act_device(frames=frames, cfg=PCFG, **kw)]
        assert all(same(x, y) for x, y in zip(first, again))
        return first, fed

    def tick(self, step=True):
        """Returns (pilot controls, label, gate, applied controls, row, fed frame) and steps the twin with the applied controls."""
        env, d = self.env, self.d
        seg, yaw, cte, speed, done = (env.fetch(name) for name in ("seg_idx", "yaw", "cte", "speed", "done"))
        label = expert_rule(seg, yaw, cte, speed, self.ty)
        pilot, fed = self.pilot()
        drives = gate(d["seed"], self.gid, self.k, d["hold"], d["beta"])
        applied = dagger_tick(pilot, label, drives, d["expert_speed"])
        row = expert_row(*label, applied[0], speed, cte, seg, done, env.n_points)
        self.stats.update(drives, cte, pilot[0], label[0], done)
        self.k += 1
        if step:
            env.step(*applied)
        return pilot, label, drives, applied, row, fed


def tick_by_tick(make_env, weights, n, ticks, base, warm=6, **dagger):
    """step_dagger(1) on one env against the reference tick on a twin: controls, state and frames after every tick.  Returns the gates drawn."""
    a, twin = make(make_env, weights, n, base), make(make_env, weights, n, base)
    for env in (a, twin):
        env.step_synthetic(warm, 1)                             # cars that have moved off the start pose, and a frame for the pilot
        env.set_expert()                                       # k = 0 from here
    ref = Reference(twin, base, **dagger)
    gates = []
    for t in range(ticks):
        pilot, label, drives, applied, _, _ = ref.tick()
        assert np.all(pilot[0][~drives] != label[0][~drives]), t      # a pilot-driven car shows the pilot's steering, not the label by accident
        assert a.step_dagger(1, PCFG, **dagger) == 0
        for name, want in zip(CTL, applied):
            assert same(a.fetch(name), want), (t, name)
        assert_same_state(a, twin)
        gates.append(drives)
    got = a.dagger_stats()
    for i, name in enumerate(STATS):
        assert same(got[name], ref.stats.a[:, i]), name
    return np.stack(gates)


# ---- 1. tick by tick -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expert_speed", [True, False])
def test_tick_by_tick_equals_pilot_act_the_rule_and_the_gate(make_env, weights, expert_speed):
    from test_dagger_cpu import gates as restated
    want = restated(12, 12, 5, 1, 0.5)
    assert want.sum() == 71 and want.any(0).all() and (~want).any(0).all() and want.any(1).all() and (~want).any(1).all()
    got = tick_by_tick(make_env, weights, 12, 12, 5, beta=0.5, seed=0, expert_speed=expert_speed)
    assert np.array_equal(got, want)


# ---- 2. limiting cases -----------------------------------------------------------------------------------------------------------------------------------
def test_beta_zero_is_step_pilot_and_beta_one_is_step_expert(make_env, weights):
    n = 12
    a, twin = make(make_env, weights, n, 5), make(make_env, weights, n, 5, expert=False)
    for _ in range(2):
        assert a.step_dagger(4, PCFG, beta=0.0, expert_speed=False) == 0
    twin.step_pilot(8, PCFG)
    assert_same_state(a, twin)
    for name in CTL:
        assert same(a.fetch(name), twin.fetch(name)), name
    st = a.dagger_stats()
    assert np.all(st["ticks"] == 8) and np.all(st["expert_ticks"] == 0)
    b, twin = make(make_env, weights, n, 5), make(make_env, weights, n, 5)
    twin.set_expert(sigma=0.0)
    b.step_dagger(8, PCFG, beta=1.0)
    twin.step_expert(8)
    assert_same_state(b, twin)
    for name in CTL:
        assert same(b.fetch(name), twin.fetch(name)), name
    st = b.dagger_stats()
    assert np.all(st["expert_ticks"] == 8) and np.any(st["sum_abs_steering_diff"] > 0)
    assert np.any(a.fetch("pos_x") != b.fetch("pos_x"))          # the two limits are different drives


# ---- 3. workgroup edge -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 1])                          # one thread in a second workgroup; a single thread
def test_workgroup_edges(make_env, weights, n):
    got = tick_by_tick(make_env, weights, n, 2, 0, beta=0.5)
    assert np.array_equal(got[:, n - 1], np.concatenate([gate(0, [n - 1], k, 1, 0.5) for k in range(2)]))   # the last thread drew its own gate
    assert got.any() and (~got).any()


# ---- 4. capture ------------------------------------------------------------------------------------------------------------------------------------------
def sentinel_buffers(slots, n):
    import torch
    d_rows = torch.full((slots, n, 8), float("nan"), dtype=torch.float32, device="cuda")
    d_frames = torch.full((slots, n, H, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d_rows, d_frames


def test_capture_equals_records_gathered_by_hand(make_env, weights):
    n, ticks = 3, 9
    a, twin = make(make_env, weights, n, 5), make(make_env, weights, n, 5)
    ref = Reference(twin, 5, beta=0.5, hold=2)
    due = [k for k in range(ticks) if k >= 1 and (k - 1) % 2 == 0]
    assert due == [1, 3, 5, 7]
    d_rows, d_frames = sentinel_buffers(4, n)
    got = a.step_dagger(ticks, PCFG, beta=0.5, hold=2, capture={"every": 2, "skip": 1, "capacity": 3, "rows": d_rows, "frames": d_frames})
    assert got == 3                                            # capacity one less than the due ticks
    a.sync()
    want_rows, want_frames = [], []
    for k in range(ticks):
        _, _, _, _, row, fed = ref.tick()
        if k in due[:3]:
            want_rows.append(row); want_frames.append(fed)
    h_rows, h_frames = d_rows.cpu().numpy(), d_frames.cpu().numpy()
    assert same(h_rows[:3], np.stack(want_rows)) and np.array_equal(h_frames[:3], np.stack(want_frames))
    assert np.all(np.isnan(h_rows[3:])) and np.all(h_frames[3:] == 0xA5)             # not a byte behind the slots filled
    assert np.any(h_rows[:3, :, 0] != h_rows[:3, :, 3]) and np.any(h_rows[:3, :, 0] == h_rows[:3, :, 3])   # pilot-driven and expert-driven rows
    assert_same_state(a, twin)
    # a first tick without a frame is not captured: k = 0 of a fresh env is due, and has no frame for the pilot
    c, twin = make(make_env, weights, n), make(make_env, weights, n)
    ref = Reference(twin)
    d_rows, d_frames = sentinel_buffers(3, n)
    assert c.step_dagger(3, PCFG, capture={"every": 1, "skip": 0, "capacity": 3, "rows": d_rows, "frames": d_frames}) == 2
    c.sync()
    recs = [ref.tick() for _ in range(3)]
    assert recs[0][5] is None and not any(x.any() for x in recs[0][0])               # the reference's pilot had no frame either: (0, 0, 0)
    h_rows, h_frames = d_rows.cpu().numpy(), d_frames.cpu().numpy()
    assert same(h_rows[:2], np.stack([r[4] for r in recs[1:]])) and np.array_equal(h_frames[:2], np.stack([r[5] for r in recs[1:]]))
    assert np.all(np.isnan(h_rows[2:])) and np.all(h_frames[2:] == 0xA5)
    assert np.all(c.dagger_stats()["ticks"] == 3)              # the tick without a frame was driven and counted all the same
    # collect(driver="pilot") is the same capture through the env's own scratch slots
    e = make(make_env, weights, n, 5)
    frames, rows = e.collect(ticks, every=2, skip=1, to_host=True, driver="pilot", cfg=PCFG, beta=0.5, hold=2)
    assert rows.shape == (4 * n, 8) and frames.shape == (4 * n, H, W, 3)
    assert same(rows[:3 * n], np.concatenate(want_rows)) and np.array_equal(frames[:3 * n], np.concatenate(want_frames))


# ---- 5. camera codec -------------------------------------------------------------------------------------------------------------------------------------
def test_with_a_camera_codec_the_captured_frame_is_the_codecs(make_env, weights):
    n = 3
    a, twin = make(make_env, weights, n), make(make_env, weights, n)
    for env in (a, twin):
        env.step_synthetic(4, 1)
        env.set_expert()
    a.set_camera_codec(75)
    ref = Reference(twin, codec=75, beta=0.5)
    d_rows, d_frames = sentinel_buffers(2, n)
    for k in range(2):
        rendered = a.fetch("img")
        pilot, label, drives, applied, row, fed = ref.tick()
        assert np.any(fed != rendered) and np.array_equal(twin.jpeg_roundtrip(rendered, 75), fed)   # the codec changes the frame; the twin read the same truth
        assert a.step_dagger(1, PCFG, beta=0.5, capture={"every": 1, "skip": 0, "capacity": 1, "rows": d_rows[k:], "frames": d_frames[k:]}) == 1
        for name, want in zip(CTL, applied):
            assert same(a.fetch(name), want), (k, name)
        a.sync()
        assert np.array_equal(d_frames[k].cpu().numpy(), fed) and same(d_rows[k].cpu().numpy(), row), k
    assert_same_state(a, twin)


# ---- 6. latency ------------------------------------------------------------------------------------------------------------------------------------------
def test_with_a_latency_the_pilot_and_the_captured_frame_are_delayed_and_the_label_is_not(make_env, weights):
    n = 6
    late = np.asarray([0, 1, 2, 3, 0, 2], np.int32)
    a, twin = make(make_env, weights, n), make(make_env, weights, n)
    for env in (a, twin):
        env.set_latency(late)
    ref = Reference(twin, late=True, beta=0.5)
    d_rows, d_frames = sentinel_buffers(3, n)
    skip = 5                                                   # past the largest delay: every car's observation has arrived
    assert a.step_dagger(8, PCFG, beta=0.5, capture={"every": 1, "skip": skip, "capacity": 3, "rows": d_rows, "frames": d_frames}) == 3
    a.sync()
    h_rows, h_frames = d_rows.cpu().numpy(), d_frames.cpu().numpy()
    for k in range(8):
        waiting = (k - late) < 1                                # the controls of tick k + 1 come from the observation after step k
        truth_frame = twin.fetch("img") if k else None
        pilot, label, drives, applied, row, fed = ref.tick()
        if k:
            assert not any(x[waiting].any() for x in pilot) and not fed[waiting].any()   # nothing has reached them: (0, 0, 0) and a frame of zeros
        if k >= skip:
            assert not waiting.any()
            assert np.array_equal(h_frames[k - skip], fed) and same(h_rows[k - skip], row), k
            assert np.any(fed[late > 0] != truth_frame[late > 0])          # the delayed frame, not the rendered truth
            assert np.array_equal(fed[late == 0], truth_frame[late == 0])
            assert same(row[:, 0], label[0])                                 # the label is the rule on the truth
    assert_same_state(a, twin)
    for name, want in zip(CTL, applied):
        assert same(a.fetch(name), want), name


# ---- 7. stats --------------------------------------------------------------------------------------------------------------------------------------------
def test_stats_equal_the_restatement_and_reset(make_env, weights):
    n = 5
    a, twin = make(make_env, weights, n, 5), make(make_env, weights, n, 5)
    ref = Reference(twin, 5, beta=0.25, hold=3, seed=9)
    kw = dict(beta=0.25, hold=3, seed=9)
    a.step_dagger(9, PCFG, **kw)
    for _ in range(9):
        ref.tick()
    live = a.dagger_stats(to_host=False)
    assert live.__cuda_array_interface__["shape"] == (n, 6)
    got = a.dagger_stats(reset=True)                           # the read at tick 9 shows the nine ticks, and zeroes behind itself
    assert same(dev_np(a, live), np.zeros((n, 6), F))
    for i, name in enumerate(STATS):
        assert same(got[name], ref.stats.a[:, i]), name
    assert np.all(got["ticks"] == 9) and np.any(got["expert_ticks"] > 0) and np.any(got["expert_ticks"] < 9)
    ref.stats = Stats(n)                                       # k goes on: the gate's blocks do not restart with the stats
    a.step_dagger(11, PCFG, **kw)
    for _ in range(11):
        ref.tick()
    got = a.dagger_stats()
    for i, name in enumerate(STATS):
        assert same(got[name], ref.stats.a[:, i]), name
    assert np.all(got["ticks"] == 11) and np.all(got["max_abs_cte"] > 0)
    assert_same_state(a, twin)
    a.set_expert()
    assert not any(v.any() for v in a.dagger_stats().values())


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_the_counter_and_the_stats_unchanged(make_env, weights):
    from triton_racer_sim_amd import _ffi
    import ctypes
    n = 4
    a, twin = make(make_env, weights, n, 5), make(make_env, weights, n, 5)
    ref = Reference(twin, 5, beta=0.5)
    a.step_dagger(3, PCFG)
    for _ in range(3):
        ref.tick()
    before, steps = a.dagger_stats(), a.counters()[2]
    rows = a.scratch(20, (1, n, 8))

    def raw(pc=None, dc=None, n_steps=1, cap=None):
        pc, dc = pc or a.pilot_config(PCFG), dc or a.dagger_config()
        return a.api.step_dagger(a._h, ctypes.byref(pc), ctypes.byref(dc), n_steps, None if cap is None else ctypes.byref(cap), None)

    for kw, word in ((dict(beta=float("nan")), "beta"), (dict(beta=float("inf")), "beta"), (dict(beta=-0.1), "beta"), (dict(beta=1.5), "beta"),
                     (dict(hold=0), "hold"), (dict(expert_speed=2), "expert_speed"), (dict(expert_speed=-1), "expert_speed")):
        with pytest.raises(RuntimeError, match=r"step_dagger failed \(-1\).*" + word):
            a.step_dagger(1, PCFG, **kw)
    with pytest.raises(RuntimeError, match=r"\(-1\).*n_steps"):
        a.step_dagger(0, PCFG)
    with pytest.raises(RuntimeError, match=r"\(-1\).*model_type"):
        a.step_dagger(1, dict(PCFG, model_type="cnn_2d_full_house"))
    pc = a.pilot_config(PCFG); pc.struct_size += 4
    assert raw(pc=pc) == -1 and b"trs_pilot_config.struct_size" in a.api.last_error()
    dc = a.dagger_config(); dc.struct_size -= 4
    assert raw(dc=dc) == -1 and b"trs_dagger_config.struct_size" in a.api.last_error()
    for cap, word in (({"every": 0, "capacity": 1, "rows": rows}, "every"), ({"skip": -1, "capacity": 1, "rows": rows}, "skip"),
                      ({"capacity": -1, "rows": rows}, "capacity"), ({"capacity": 1, "rows": None}, "d_rows")):
        with pytest.raises(RuntimeError, match=r"\(-1\).*" + word):
            a.step_dagger(1, PCFG, capture=cap)
    cap = a._capture({"capacity": 1, "rows": rows}); cap.struct_size += 8
    assert raw(cap=cap) == -1 and b"trs_expert_capture.struct_size" in a.api.last_error()
    # nothing moved: no step was taken, the stats are the same, and the next accepted call draws the gate of the unchanged k = 3
    assert a.counters()[2] == steps
    after = a.dagger_stats()
    assert all(same(before[k], after[k]) for k in STATS)
    _, _, drives, applied, _, _ = ref.tick()
    assert not np.array_equal(drives, gate(0, ref.gid, 4, 1, 0.5))                  # (the comparison below tells k = 3 from k = 4)
    a.step_dagger(1, PCFG)
    for name, want in zip(CTL, applied):
        assert same(a.fetch(name), want), name
    assert_same_state(a, twin)
    # TRS_ERR_STATE: no expert, no pilot, no camera
    a.set_expert(False)
    with pytest.raises(RuntimeError, match=r"step_dagger failed \(-2\).*no expert set"):
        a.step_dagger(1, PCFG)
    with pytest.raises(RuntimeError, match=r"dagger_stats failed \(-2\).*no expert set"):
        a.dagger_stats()
    bare = make_env("hip", n_envs=n, img_h=H, img_w=W)
    bare.set_expert()
    with pytest.raises(RuntimeError, match=r"\(-2\).*no pilot loaded"):
        bare.step_dagger(1, PCFG)
    blind = make_env("hip", n_envs=n, img_h=H, img_w=W, render=False)
    blind.pilot_load(weights)
    blind.set_expert()
    with pytest.raises(RuntimeError, match=r"\(-2\).*camera"):
        blind.step_dagger(1, PCFG)
    assert bare.counters()[2] == 0 and blind.counters()[2] == 0
    assert ctypes.sizeof(_ffi.TrsDaggerConfig) == a.dagger_config().struct_size


# ---- 9. resident mode ------------------------------------------------------------------------------------------------------------------------------------
def test_in_resident_mode_the_call_succeeds_and_equals_launch_mode(make_env, weights):
    n = 5
    a, r = make(make_env, weights, n, expert=False), make(make_env, weights, n, expert=False)
    r.set_step_mode(True)
    for env in (a, r):
        env.step_synthetic(3, 1)                               # (r: posted to the worker, which the loop then asks to leave)
        env.set_expert()
        env.step_dagger(6, PCFG, beta=0.5, hold=2)
    assert r.step_mode()[0] == "resident"
    assert_same_state(a, r)
    for name in CTL:
        assert same(a.fetch(name), r.fetch(name)), name
    sa, sr = a.dagger_stats(), r.dagger_stats()
    assert all(same(sa[k], sr[k]) for k in STATS) and np.all(sa["ticks"] == 6)
