"""Observation latency on the GPU (include/trsim_spec.h, "observation latency"; trs_set_latency): after every call the observation of env e (frame,
depth frame, x, y, z, speed, cte, index, arrived) is the record the oracle produced L_e ticks earlier — the oracle stepped one tick at a time, its records
kept in a list — or the constructor's zeros, while everything that shows what the simulator did stays the oracle's truth.  One latency for all envs moves
no frame byte; every frame producer (lighting, static and dynamic filter, lens, depth) is delayed alike; off again the handle steps like one that never
set a latency; trs_load_track restarts the history and a reset does not; the refusals leave the handle stepping as its twin; the closed pilot loop
drives on the observation; BatchedGymInterface honours sim_latency like HipGymInterface's delay line; physics-only handles deliver telemetry."""
import numpy as np
import pytest

from conftest import track_points

pytestmark = pytest.mark.gpu

TELE = ("pos_x", "pos_y", "pos_z", "speed", "cte", "seg_idx")
STATE = TELE + ("yaw", "done", "ep_len", "ep_return", "last_return")


def dev_np(handle):
    import torch
    return torch.as_tensor(handle, device="cuda").cpu().numpy()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def truth_record(env, depth=False, frame=None):
    """The truth record R_T of an env (the oracle's, or a twin handle's), with `frame` applied to the raw frame (lighting, a frame filter)."""
    r = {k: env.fetch(k) for k in TELE}
    if env.cfg.render:
        img = env.fetch("img")
        r["img"] = frame(img) if frame else img
        if depth:
            r["depth"] = env.fetch("depth")
    return r


def told(hist, ticks, key):
    """What env e is told after step T = len(hist): hist[T - L_e - 1][key][e], zeros while T - L_e < 1."""
    T = len(hist)
    want = np.zeros_like(hist[-1][key])
    for e, L in enumerate(ticks):
        if T - L >= 1:
            want[e] = hist[T - L - 1][key][e]
    return want


def assert_observation(g, hist, ticks, where, depth=False, image=True):
    got = g.observation(image=image)
    T = len(hist)
    arrived = np.asarray([1 if T - L >= 1 else 0 for L in ticks], np.uint8)
    assert np.array_equal(got[7], arrived), (where, "arrived")
    for k, a in zip(TELE, got[1:7]):
        assert np.array_equal(bits(a), bits(told(hist, ticks, k))), (where, k)
    if image:
        want = told(hist, ticks, "img")
        bad = np.argwhere(np.any(got[0] != want, axis=-1))
        assert bad.size == 0, f"{where}: {len(bad)} pixels of the observation differ, first (env, v, u) {bad[:4].tolist()}"
    if depth:
        assert np.array_equal(bits(dev_np(g.device_observation("depth"))), bits(told(hist, ticks, "depth"))), (where, "depth")


def assert_truth(g, o, where, depth=False, frame=None):
    for k in STATE:
        assert np.array_equal(bits(g.fetch(k)), bits(o.fetch(k))), (where, k)
    if g.cfg.render:
        img = o.fetch("img")
        assert np.array_equal(g.fetch("img"), frame(img) if frame else img), (where, "img")
        if depth:
            assert np.array_equal(bits(g.fetch("depth")), bits(o.fetch("depth"))), (where, "depth")


def assert_history_tells_delays_apart(hist, within=6):
    """The condition of the comparison: for every env no two frames and no two telemetry records within `within` ticks of each other are identical —
    otherwise a wrong delay could deliver the right bytes."""
    same_img = same_tel = pairs = 0
    for a in range(len(hist)):
        for b in range(a + 1, min(a + within, len(hist) - 1) + 1):
            pairs += hist[a]["img"].shape[0]
            same_img += int(np.sum(np.all(hist[a]["img"] == hist[b]["img"], axis=(1, 2, 3))))
            same_tel += int(np.sum(np.all(np.stack([bits(hist[a][k]) == bits(hist[b][k]) for k in TELE]), axis=0)))
    print(f"identical pairs within {within} ticks: frames {same_img}, telemetry {same_tel} of {pairs}")
    assert same_img == 0 and same_tel == 0, (same_img, same_tel, pairs)


class Pair:
    """A HIP handle with a latency and the oracle beside it: every call goes to the HIP handle as it is and to the oracle one tick at a time."""

    def __init__(self, g, o, ticks, depth=False, frame=None):
        self.g, self.o, self.ticks, self.depth, self.frame, self.hist = g, o, list(ticks), depth, frame, []

    def _tick(self, fn):
        fn(self.o)
        self.hist.append(truth_record(self.o, self.depth, self.frame))

    def check(self, where, image=True):
        assert_truth(self.g, self.o, where, self.depth, self.frame)
        assert_observation(self.g, self.hist, self.ticks, where, self.depth and image, image and bool(self.g.cfg.render))

    def synthetic(self, n, per_launch, where=None):
        self.g.step_synthetic(n, per_launch)
        for _ in range(n):
            self._tick(lambda o: o.step_synthetic(1, 1))
        self.check(where or f"step_synthetic({n}, {per_launch}) -> T = {len(self.hist)}")

    def held(self, st, th, n):
        self.g.step(st, th, n_steps=n)
        for _ in range(n):
            self._tick(lambda o: o.step(st, th))
        self.check(f"step(n_steps={n}) -> T = {len(self.hist)}")

    def sequence(self, st, th, per_launch):
        self.g.step_sequence(st, th, steps_per_launch=per_launch)
        for i in range(st.shape[0]):
            self._tick(lambda o: o.step(st[i], th[i]))
        self.check(f"step_sequence({st.shape[0]} rows, {per_launch} per launch) -> T = {len(self.hist)}")


@pytest.mark.parametrize("track,n,h,w,depth", [("generated", 37, 120, 160, False), ("generated", 13, 62, 164, True), ("mountain", 21, 120, 160, False),
                                               ("generated", 9, 240, 320, False)])
def test_observation_equals_the_oracles_history(make_env, track, n, h, w, depth):
    pts = track_points(track)
    g = make_env("hip", n_envs=n, track=pts, img_h=h, img_w=w, depth=depth, auto_reset=True)
    o = make_env("oracle", n_envs=n, track=pts, img_h=h, img_w=w, depth=depth, auto_reset=True)
    ticks = np.arange(n) % 7                                  # every delay 0..6
    g.set_latency(ticks)
    got, mx = g.latency()
    assert mx == 6 and np.array_equal(got, ticks)
    p = Pair(g, o, ticks, depth)
    rng = np.random.default_rng(11)
    for _ in range(12):
        p.synthetic(1, 1)
    p.synthetic(7, 3)                                         # several steps per call: at L = 1 the observation is a frame no buffer held before the ring
    mask = (np.arange(n) % 3 == 0)
    g.reset(mask); o.reset(mask)
    st, th = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(0.6, 1, n).astype(np.float32)
    p.held(st, th, 3)
    p.sequence(rng.uniform(-1, 1, (4, n)).astype(np.float32), rng.uniform(0.6, 1, (4, n)).astype(np.float32), 4)
    assert len(p.hist) == 26
    assert_history_tells_delays_apart(p.hist)


def test_one_latency_for_all_moves_no_frame_byte(make_env):
    n, L = 16, 3
    pts = track_points("generated")
    g = make_env("hip", n_envs=n, track=pts, auto_reset=True)
    o = make_env("oracle", n_envs=n, track=pts, auto_reset=True)
    g.set_latency(L)
    p = Pair(g, o, [L] * n)
    frames = []                                               # trs_get_state's img pointer after step 1, 2, ...
    for T in range(1, 10):
        p.synthetic(1, 1)
        frames.append(g.state_view().img)
        if T - L >= 1:
            assert g.observation_view().img == frames[T - L - 1], T      # the view points into the ring slot of step T - 3
        assert g.observation_view().img != frames[-1]
    p.synthetic(4, 2)
    # every delay 0 with the ring on: the observation is the truth, and the view is the state's frame
    g.set_latency(0, max_ticks=2)
    p = Pair(g, o, [0] * n)
    for _ in range(3):
        p.synthetic(1, 1)
        assert g.observation_view().img == g.state_view().img
        for k, a in zip(TELE, g.observation()[1:7]):
            assert np.array_equal(bits(a), bits(g.fetch(k))), k
        assert np.array_equal(g.observation()[0], g.fetch("img"))


def test_every_frame_producer_is_delayed_alike(make_env):
    from test_lighting_gpu import light_frames, params_for
    n = 8
    pts = track_points("generated")
    ticks = np.arange(n) % 4

    def run(p):
        for _ in range(4):
            p.synthetic(1, 1)
        p.synthetic(5, 2)

    # scene lighting: the history is the lit oracle frame
    g = make_env("hip", n_envs=n, track=pts, auto_reset=True)
    o = make_env("oracle", n_envs=n, track=pts, auto_reset=True)
    lp = params_for(n, 4)
    g.set_lighting(lp)
    g.set_latency(ticks)
    run(Pair(g, o, ticks, frame=lambda img: light_frames(img, lp)))
    # the static and the dynamic-brightness frame filter: the history is the filtered oracle frame
    for cfg in ({"preprocessing_contrast_enhancement_ratio": 1.2, "preprocessing_color_filter_enabled": True},
                {"preprocessing_contrast_enhancement_ratio": 1.2, "preprocessing_dynamic_brightness_enabled": True}):
        g = make_env("hip", n_envs=n, track=pts, auto_reset=True)
        o = make_env("oracle", n_envs=n, track=pts, auto_reset=True)
        g.set_latency(ticks)
        g.set_frame_filter(cfg)
        run(Pair(g, o, ticks, frame=lambda img: o.preprocess_host(img, cfg)))
    # the lens camera (no oracle), and depth with lighting: the history is recorded from a twin handle without latency, stepped singly
    for kw, light in ((dict(camera=dict(fish_eye_x=1.5, fish_eye_y=0.3, offset_x=0.4)), None), (dict(depth=True), params_for(n, 6))):
        g = make_env("hip", n_envs=n, track=pts, auto_reset=True, **kw)
        t = make_env("hip", n_envs=n, track=pts, auto_reset=True, **kw)
        if light is not None:
            g.set_lighting(light); t.set_lighting(light)
        g.set_latency(ticks)
        run(Pair(g, t, ticks, depth="depth" in kw))


def test_off_again_the_handle_steps_like_one_that_never_set_a_latency(make_env):
    n = 10
    pts = track_points("generated")
    g = make_env("hip", n_envs=n, track=pts, depth=True, auto_reset=True)
    t = make_env("hip", n_envs=n, track=pts, depth=True, auto_reset=True)
    ticks = np.arange(n) % 5
    t.step_synthetic(2, 1)
    g.step_synthetic(2, 1)                                     # both frame buffers hold their uniform rows when the ring takes over
    g.set_latency(ticks)
    g.step_synthetic(4, 1); t.step_synthetic(4, 1)
    g.set_latency(None)
    assert g.latency()[1] == 0
    with pytest.raises(RuntimeError, match="no observation latency is set"):
        g.observation()
    g.step_synthetic(5, 2); t.step_synthetic(5, 2)
    assert_truth(g, t, "multi-step launches after off", depth=True)
    for k in range(3):
        g.step_synthetic(1, 1); t.step_synthetic(1, 1)
        assert_truth(g, t, f"single step {k} after off", depth=True)
    # set -> off -> set: the history restarts at the constructor's state
    g.set_latency(ticks)
    img, *tele, arrived = g.observation()
    assert not img.any() and not arrived.any() and all(not a.any() for a in tele)
    assert not dev_np(g.device_observation("depth")).any()
    g.step_synthetic(1, 1); t.step_synthetic(1, 1)
    assert_observation(g, [truth_record(t, depth=True)], ticks, "first step of the new history", depth=True)


@pytest.mark.parametrize("render", [True, False])
def test_a_latency_set_over_a_latency_is_the_setting_alone(make_env, render):
    """One delay for all (the view into the ring) -> different delays in a larger ring (gathered frames) -> one delay in a smaller ring (the view again) -> off:
    every setting replaces the buffers of the one before.  After every step the observation is that of a twin that took the same steps without a latency
    and set only the current setting where it begins; off again, the outputs are those of a twin that never set one.  render=False: telemetry only."""
    n = 5
    kw = dict(n_envs=n, img_h=30, img_w=44, depth=render, render=render, track=track_points("generated"), auto_reset=True)
    g = make_env("hip", **kw)
    done = 0
    for ticks, mx in ((2, 2), ([0, 3, 1, 3, 2], 3), ([1, 1, 1, 1, 1], 1)):
        t = make_env("hip", **kw)
        if done:
            t.step_synthetic(done, 1)
        g.set_latency(ticks, max_ticks=mx); t.set_latency(ticks, max_ticks=mx)
        assert g.latency()[1] == mx and np.array_equal(g.latency()[0], t.latency()[0])
        for k in range(mx + 3):
            g.step_synthetic(1, 1); t.step_synthetic(1, 1); done += 1
            for i, (a, b) in enumerate(zip(g.observation(image=render), t.observation(image=render))):
                assert (a is None and b is None) or np.array_equal(bits(a), bits(b)), (ticks, k, i)
            for name in ("img", "depth") if render else ():
                assert np.array_equal(bits(dev_np(g.device_observation(name))), bits(dev_np(t.device_observation(name)))), (ticks, k, name)
    t = make_env("hip", **kw)
    t.step_synthetic(done, 1)
    g.set_latency(None)
    for k in range(3):
        g.step_synthetic(1, 1); t.step_synthetic(1, 1)
        for i, (a, b) in enumerate(zip(g.fetch_outputs(image=render), t.fetch_outputs(image=render))):
            assert (a is None and b is None) or np.array_equal(bits(a), bits(b)), ("off", k, i)


def test_load_track_restarts_the_history_and_a_reset_does_not(make_env):
    n = 9
    pts = track_points("generated")
    g = make_env("hip", n_envs=n, track=pts, auto_reset=True)
    o = make_env("oracle", n_envs=n, track=pts, auto_reset=True)
    ticks = np.arange(n) % 4
    g.set_latency(ticks)
    p = Pair(g, o, ticks)
    p.synthetic(5, 1)
    g.reset(); o.reset()                                      # every car back to its start: the old episode's packets keep arriving for L_e ticks
    for k in range(4):
        p.synthetic(1, 1, where=f"tick {k + 1} after a reset of all cars")
    g.load_track(pts); o.load_track(pts)
    img, *tele, arrived = g.observation()
    assert not img.any() and not arrived.any() and all(not a.any() for a in tele)
    p = Pair(g, o, ticks)
    for k in range(4):
        p.synthetic(1, 1, where=f"tick {k + 1} after trs_load_track")


def test_refusals_leave_the_handle_stepping_like_its_twin(make_env):
    n = 7
    pts = track_points("generated")
    g = make_env("hip", n_envs=n, track=pts, auto_reset=True)
    t = make_env("hip", n_envs=n, track=pts, auto_reset=True)

    def steps_like_twin(where):
        g.step_synthetic(3, 1); t.step_synthetic(3, 1)
        assert_truth(g, t, where)

    g.set_step_mode(True)
    with pytest.raises(RuntimeError, match="resident mode is selected"):
        g.set_latency(2)
    assert g.step_mode()[0] == "resident" and g.latency()[1] == 0
    steps_like_twin("resident, latency refused")
    g.set_step_mode(False)
    ticks = np.arange(n) % 3
    g.set_latency(ticks)
    with pytest.raises(RuntimeError, match="observation latency is set"):
        g.set_step_mode(True)
    assert g.step_mode()[0] == "launch"
    steps_like_twin("latency, resident refused")
    for bad_ticks, bad_max in (([-1] + [0] * (n - 1), 2), (5, 3), (1, 31), (0, 0), (1, -4)):
        with pytest.raises(RuntimeError, match="set_latency failed \\(-1\\)"):
            g.set_latency(bad_ticks, max_ticks=bad_max)
        got, mx = g.latency()
        assert mx == 2 and np.array_equal(got, ticks)
        steps_like_twin(f"after refused ticks {bad_ticks} / max_ticks {bad_max}")
    with pytest.raises(ValueError):
        g.set_latency(1.5)
    # the observation still follows the history that began at set_latency, 3 steps into the handle's life and 3 + 5 * 3 steps ago
    hist = []
    o = make_env("oracle", n_envs=n, track=pts, auto_reset=True)
    o.step_synthetic(3, 1)
    for _ in range(18):
        o.step_synthetic(1, 1)
        hist.append(truth_record(o))
    assert_observation(g, hist, ticks, "after all refusals")


def test_closed_loop_drives_on_the_observation(make_env):
    import torch
    from test_pilot import make_weights
    from triton_racer_sim_amd.env import device_ptr
    n, h, w = 6, 120, 160
    ws = make_weights(h, w, seed=5)
    ws[-1] = ws[-1] + np.float32([0.0, 0.4])                 # a pilot that drives off
    ticks = np.asarray([0, 1, 2, 3, 0, 1], np.int32)
    a, b, c = (make_env("hip", n_envs=n, img_h=h, img_w=w) for _ in range(3))
    for env in (a, b, c):
        env.pilot_load(ws)
    a.set_latency(ticks); b.set_latency(ticks)
    differs = False
    for T in range(1, 9):
        a.step_pilot(1)
        c.step_pilot(1)
        arrived = torch.as_tensor(b.device_observation("arrived"), device="cuda")
        mode = torch.where(arrived != 0, 2, 0).to(torch.uint8)                    # AI where the observation has arrived, else HUMAN
        torch.cuda.synchronize()
        ai = b.pilot_act_device(frames=b.device_observation("img"), speed=b.device_observation("speed"), mode=mode)
        b.step_device(device_ptr(ai[0]), device_ptr(ai[1]), device_ptr(ai[2]))
        for k in STATE + ("vel",):
            assert np.array_equal(bits(a.fetch(k)), bits(b.fetch(k))), (T, k)
        assert np.array_equal(a.fetch("img"), b.fetch("img")), T
        ctl = [a.fetch(k) for k in ("ctl_steer", "ctl_thr", "ctl_brk")]
        for x, y in zip(ctl, ai):
            assert np.array_equal(bits(x), bits(dev_np(y))), T
        waiting = (T - 1) - ticks < 1                          # the controls of tick T come from the observation after T - 1
        assert all(not x[waiting].any() for x in ctl), T
        assert any(x[~waiting].any() for x in ctl) or T == 1, T
        assert np.array_equal(bits(a.fetch("pos_x"))[ticks == 0], bits(c.fetch("pos_x"))[ticks == 0]), T      # no delay: the loop without latency
        if T == 4:
            differs = any(np.any(a.fetch(k)[ticks > 0] != c.fetch(k)[ticks > 0]) for k in ("pos_x", "pos_z", "speed"))
    assert differs, "the loop under latency equals the loop without: the comparison shows nothing"


def test_batched_gym_interface_honours_sim_latency(make_env):
    from triton_racer_sim_amd.components import BatchedGymInterface, HipGymInterface
    one = HipGymInterface(gym_config={"sim_latency": 120})
    bat = BatchedGymInterface(1, gym_config={"sim_latency": 120}, to_host=True, auto_reset=False)
    try:
        assert one.latency_ticks == 3 and bat.latency_ticks.tolist() == [3]
        rng = np.random.default_rng(5)
        for T in range(1, 9):
            st, th = float(rng.uniform(-1, 1)), float(rng.uniform(0.6, 1))
            want = one.step(st, th, 0.0, False)
            img, x, y, z, speed, cte, idx, done = bat.step(st, th, 0.0, False)
            if T <= 3:
                assert want[0] is None and want[1:] == (0.0,) * 5
                assert not img.any() and (x[0], y[0], z[0], speed[0], cte[0], idx[0]) == (0, 0, 0, 0, 0, 0)
            else:
                assert np.array_equal(img[0], want[0]), T
                assert (float(x[0]), float(y[0]), float(z[0]), float(speed[0]), float(cte[0])) == want[1:], T
            assert done[0] == one.env.fetch("done")[0]
    finally:
        one.onShutdown(); bat.onShutdown()
    # one value per env, device handles on the ports, against the oracle's history
    n, ms = 5, [0, 50, 100, 120, 300]
    ticks = [0, 1, 2, 3, 6]
    bat = BatchedGymInterface(n, gym_config={"sim_latency": ms}, auto_reset=True)
    o = make_env("oracle", n_envs=n, auto_reset=True)
    try:
        assert bat.latency_ticks.tolist() == ticks
        hist = []
        for T in range(1, 10):
            st, th = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(0.6, 1, n).astype(np.float32)
            out = [dev_np(v) for v in bat.step(st, th, None, None)]
            o.step(st, th)
            hist.append(truth_record(o))
            for k, got in zip(("img",) + TELE, out[:7]):
                assert np.array_equal(bits(got), bits(told(hist, ticks, k))), (T, k)
            assert np.array_equal(out[7], o.fetch("done")), T
    finally:
        bat.onShutdown()
    # every latency 0: nothing is set
    bat = BatchedGymInterface(2, gym_config={"sim_latency": 0})
    try:
        assert not bat.delayed and bat.env.latency()[1] == 0
    finally:
        bat.onShutdown()


def test_physics_only_handles_deliver_delayed_telemetry(make_env):
    n = 11
    pts = track_points("generated")
    g = make_env("hip", n_envs=n, track=pts, render=False, auto_reset=True)
    o = make_env("oracle", n_envs=n, track=pts, render=False, auto_reset=True)
    ticks = np.arange(n) % 7
    g.set_latency(ticks)
    assert not g.observation_view().img and not g.observation_view().depth
    with pytest.raises(RuntimeError, match="no camera"):
        g.observation(image=True)
    p = Pair(g, o, ticks)
    for _ in range(5):
        p.synthetic(1, 1)
    p.synthetic(6, 4)
    rng = np.random.default_rng(2)
    p.held(rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(0.6, 1, n).astype(np.float32), 2)
