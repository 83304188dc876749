"""cnn_2d_speed_control in the loop.  The checker for this floating-point kernel is a plain PyTorch
fp32 restatement of the reference's architecture (components/keras_train.py:127-174: conv 5x5/2 x3, conv 3x3 x4,
'valid', ReLU; NHWC flatten; dense 100/50/25 ReLU; linear 2) and of KerasPilot's post-processing
(components/keras_pilot.py:78-95, utils/mapping.py:23-35).  The HIP path uses binary16 (fp16) operands with fp32 accumulation and
stores activations as fp16 (round 3; bfloat16 until round 2 — the same MFMA rate, three fewer mantissa bits), so two references are used:
  * "mirror", layer by layer: fp32 math on fp16-rounded weights, fed the kernel's own previous activation — differs from
    the kernel only by fp32 summation order, which can move a value across an fp16 rounding boundary: per element
    |got - ref| <= 2^-10 |ref| + 2e-4 (one fp16 ulp is up to 2^-10 relative at the bottom of a binade, + an absolute floor)
    and fewer than 2 % of the elements differ at all;
  * "pure": fp32 everywhere (what TensorFlow would compute): tolerance 4e-4 on the two outputs — measured: max |HIP - fp32| 4.4e-5 over
    288 frames x 3 weight sets at both frame sizes (scripts/pilot_precision.py, profiles/r03_pilot_precision.txt; 5.0e-4 with bfloat16).
The cases here run the default plans of 120x160, 240x320, 100x132 and 130x300 and their tuned-off neighbours.  The generic fallback (trs_conv_lt_kernel, the quad-load
kernel: never reached by these plans) and the default plans of 360x480, 480x640 and of frames 96 and 100 wide have their tests in tests/test_pilot_fallback.py.
The outputs here come from 8 K slices of dense1 (120x160) or 123 (240x320), and test_dense_kernel_against_torch_in_both_frame_groupings reads dense1 through a getter
that adds the slabs on the host: the other slice counts, through the tail kernels that add the slabs on the device, are in tests/test_pilot_slices.py."""
import math
import types

import numpy as np
import pytest

from test_pilot_plan_cpu import build_driver, call_of, plan_of

pytestmark = pytest.mark.gpu

SPEC = [(5, 2, 3, 24), (5, 2, 24, 32), (5, 2, 32, 64), (3, 1, 64, 64), (3, 1, 64, 64), (3, 1, 64, 128), (3, 1, 128, 128)]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """What trs_pilot_load plans on this device (csrc/trsim_pilot_plan.hpp through tests/pilot_plan_driver.cpp, a host program): a comparison test asks it
    which kernels its two runs reach.  plan(h, w, n_cap, **tuning) and call(h, w, n_cap, n, **tuning) as in tests/test_pilot_plan_cpu.py.
    The plan is made for this device's CU count, as the library makes it; the values the tests expect of it (64 frames per dense workgroup at 150 frames of
    240x320, 4 frames per chain workgroup at 1027 only, rolling bands at 300 / 150 / 131 frames) are those of the MI355X's 256 CUs: on a part with another
    count they fail, which says that the cases no longer reach the kernels their docstrings name and want choosing anew."""
    import torch
    exe = build_driver(tmp_path_factory.mktemp("pilot_plan"), sanitize=False)
    assert exe, "the plan driver needs g++"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return types.SimpleNamespace(cus=cus, plan=lambda h, w, n_cap, **t: plan_of(exe, h, w, n_cap, cus=cus, **t),
                                 call=lambda h, w, n_cap, n, **t: call_of(exe, h, w, n_cap, n, cus=cus, **t))


def served(plan):
    """the kernel that serves conv1..conv7 in a forward pass"""
    return [l["served_by"] for l in plan["layers"][:7]]


def make_weights(h, w, seed=0):
    """Glorot-uniform kernels (Keras default), small random biases; Keras layouts."""
    rng = np.random.default_rng(seed)
    ws = []
    ih, iw = h, w
    for k, s, cin, cout in SPEC:
        lim = math.sqrt(6.0 / (k * k * cin + k * k * cout))
        ws += [rng.uniform(-lim, lim, (k, k, cin, cout)).astype(np.float32), rng.uniform(-0.05, 0.05, cout).astype(np.float32)]
        ih, iw = (ih - k) // s + 1, (iw - k) // s + 1
    dims = [ih * iw * 128, 100, 50, 25, 2]
    for a, b in zip(dims[:-1], dims[1:]):
        lim = math.sqrt(6.0 / (a + b))
        ws += [rng.uniform(-lim, lim, (a, b)).astype(np.float32), rng.uniform(-0.05, 0.05, b).astype(np.float32)]
    return ws


def torch_layer(i, x_nhwc, ws, mirror=True):
    """Layer i (0..6 conv, 7 dense1) of the reference architecture in fp32 on an NHWC input; with ``mirror`` the weights are
    rounded to fp16 (conv1's carry 256 / 255 and its sums are multiplied by 2^-8, as the kernel folds the pilot's /255) and so is the output."""
    import torch
    import torch.nn.functional as F
    bf = (lambda t: t.half().float()) if mirror else (lambda t: t)
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=np.float32))
    if i == 7:
        z = F.relu(x.reshape(x.shape[0], -1) @ bf(torch.from_numpy(ws[14])) + torch.from_numpy(ws[15]))     # Keras Flatten on NHWC
        return z.numpy()
    k, s, cin, cout = SPEC[i]
    wk = torch.from_numpy(ws[2 * i])
    scale = 1.0
    if i == 0:
        if mirror:
            wk, scale = wk * (256.0 / 255.0), 1.0 / 256.0
        else:
            x = x / 255.0                                               # keras_pilot.py:49-50
    wk = bf(wk).permute(3, 2, 0, 1).contiguous()
    y = F.relu(F.conv2d(x.permute(0, 3, 1, 2), wk, None, stride=s) * scale + torch.from_numpy(ws[2 * i + 1]).view(1, -1, 1, 1))
    return bf(y).permute(0, 2, 3, 1).contiguous().numpy()


def torch_tail(h1, ws):
    import torch
    import torch.nn.functional as F
    z = torch.from_numpy(h1)
    z = F.relu(z @ torch.from_numpy(ws[16]) + torch.from_numpy(ws[17]))
    z = F.relu(z @ torch.from_numpy(ws[18]) + torch.from_numpy(ws[19]))
    return (z @ torch.from_numpy(ws[20]) + torch.from_numpy(ws[21])).numpy()


def torch_pure(frames, ws):
    x = frames
    for i in range(8):
        x = torch_layer(i, x, ws, mirror=False)
    return torch_tail(x, ws)


def pilot_postprocess(out, speed, cfg):
    """KerasPilot.step, ModelType.CNN_2D_SPD_CTL (keras_pilot.py:78-95) with the reference's scalar helpers restated."""
    steer = float(min(max(out[0], -1.0), 1.0))
    pred = float(out[1]) * 20
    thr = cfg.get("spd_ctl_reverse_multiplier", 1.0) * math.atan((pred * cfg.get("spd_ctl_threshold", 1.1) - speed) * 2) / (math.pi / 2)
    if -0.2 < thr < 0.0:
        thr = 0.0
    brk = 0.0
    if cfg.get("spd_ctl_break", False):
        thr = 1.0 if pred - speed > 0.0 else 0.0
        brk = -1.0 * cfg.get("spd_ctl_break_multiplier", 1.0) * math.atan((pred * cfg.get("spd_ctl_threshold", 1.1) - speed) * 1.0) / (math.pi / 2)
        if brk < 0.4:
            brk = 0.0
    return steer, thr, brk


@pytest.mark.parametrize("size", [(120, 160), (240, 320)])
def test_forward_matches_torch_fp32(make_env, size):
    h, w = size
    n = 6
    env = make_env("hip", n_envs=n, img_h=h, img_w=w, auto_reset=True)
    ws = make_weights(h, w, seed=3)
    env.pilot_load(ws)
    env.step_synthetic(12, 1)
    frames = env.fetch("img")
    rng = np.random.default_rng(0)
    frames = np.concatenate([frames[:4], rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)])     # rendered + noise frames
    out = env.pilot_forward_host(frames)
    # layer by layer: the torch layer is fed the kernel's OWN previous activation, so the only difference left is the fp32
    # summation order, which can flip the final fp16 rounding of an element by one ulp (up to 2^-10 relative)
    x, shape = frames, None
    for layer in range(8):
        want = torch_layer(layer, x, ws)
        got = env.pilot_layer(layer, want.shape)
        diff = np.abs(got - want)
        assert (diff <= 2.0 ** -10 * np.abs(want) + 2e-4).all(), f"layer {layer}: worst {float(diff.max())}"
        assert np.mean(diff > 1e-6) < 0.02, f"layer {layer}: {100 * np.mean(diff > 1e-6):.2f}% of the elements differ"
        x = got
    assert np.max(np.abs(out - torch_tail(x, ws))) <= 1e-4          # fp32 tail on identical inputs
    pure = torch_pure(frames, ws)                                     # fp32 everywhere: bounds the total fp16 effect
    print(f"max |HIP - fp32 torch| per output at {h}x{w}: {np.abs(out - pure).max(0)}")
    assert np.max(np.abs(out - pure)) <= 4e-4, float(np.max(np.abs(out - pure)))
    assert np.std(out[:, 0]) > 1e-4                                  # the outputs do depend on the frame


def test_closed_loop_controls_follow_the_reference_tick_order(make_env):
    """trs_step_pilot == [controls = post(model(previous frame), speed); env.step(controls)] done by hand, and the
    first tick uses (0, 0, 0) because no frame exists yet (keras_pilot.py:46-47)."""
    n = 16
    ws = make_weights(120, 160, seed=5)
    cfg = {"spd_ctl_threshold": 1.1, "spd_ctl_reverse_multiplier": 1.0}
    a = make_env("hip", n_envs=n)
    b = make_env("hip", n_envs=n)
    a.pilot_load(ws); b.pilot_load(ws)
    a.step_pilot(6, cfg)
    b.step(0.0, 0.0, 0.0)                                            # tick 1: no frame yet
    for _ in range(5):
        out = b.pilot_forward_host(b.fetch("img"))
        spd = b.fetch("speed")
        ctl = np.array([pilot_postprocess(out[i], float(spd[i]), cfg) for i in range(n)], dtype=np.float32)
        b.step(ctl[:, 0], ctl[:, 1], ctl[:, 2])
    for name in ("pos_x", "pos_z", "yaw", "speed"):
        assert np.max(np.abs(a.fetch(name) - b.fetch(name))) <= 1e-4, name   # float atan on device vs math.atan: ~1e-7 per tick
    assert np.array_equal(a.fetch("seg_idx"), b.fetch("seg_idx"))
    assert np.array_equal(a.fetch("img"), b.fetch("img"))


def test_closed_loop_frames_stay_whole_when_uniform_rows_are_kept(make_env):
    """Round 5: the closed loop's env steps write the uniform rows of a frame buffer (sky, beyond the far plane: 41 % of the bytes) only when the buffer
    does not hold them yet.  Every frame of the loop must still be the oracle's frame for the pose it shows — across a frame-filter change (another palette,
    other uniform rows), steps of other kinds in between (a resident worker, multi-step launches) and a track reload.  RGB + depth.  The comparison
    is a fresh handle that renders WHOLE frames (plain trs_step) of the same step from the same state: that path is what tests/test_gpu_parity.py pins to the oracle."""
    n, h, w = 6, 120, 160
    g = make_env("hip", n_envs=n, img_h=h, img_w=w, depth=True)
    ws = make_weights(h, w, seed=5)
    ws[-1] = ws[-1] + np.float32([0.0, 0.4])
    g.pilot_load(ws)
    flt = {"preprocessing_color_filter_enabled": True, "preprocessing_contrast_enhancement_ratio": 1.3}

    g.step_pilot(7)                                                    # both buffers written whole once, then ground rows only
    g.sync()
    # the loop's latest frame against a fresh handle's whole-frame render of the same pose and controls
    def same_as_whole_frames(where, filt=None):
        ref = make_env("hip", n_envs=n, img_h=h, img_w=w, depth=True)
        if filt:
            ref.set_frame_filter(filt)
        ref.step(0.0, 0.0, 0.0)
        # replay the loop's last step from the state in front of it: the loop leaves (pose after the step, controls it used)
        ref.set_pose(prev["pos_x"], prev["pos_y"], prev["pos_z"], prev["yaw"], prev["vel"])
        ref.step(last_ctl[0], last_ctl[1], last_ctl[2])
        assert np.array_equal(ref.fetch("img"), g.fetch("img")), where
        assert np.array_equal(ref.fetch("depth").view(np.uint32), g.fetch("depth").view(np.uint32)), where

    def one_tick():
        nonlocal prev, last_ctl
        prev = {k: g.fetch(k).copy() for k in ("pos_x", "pos_y", "pos_z", "yaw", "vel")}
        g.step_pilot(1)
        last_ctl = (g.fetch("ctl_steer").copy(), g.fetch("ctl_thr").copy(), g.fetch("ctl_brk").copy())

    prev, last_ctl = None, None
    for k in range(4):
        one_tick()
        same_as_whole_frames(f"plain loop, tick {k}")
    g.set_frame_filter(flt)                                            # another palette: both buffers' uniform rows are stale now
    for k in range(3):
        one_tick()
        same_as_whole_frames(f"filtered loop, tick {k}", flt)
    g.set_frame_filter(enabled=False)
    g.step_synthetic(5, 4)                                             # multi-step launches in between
    g.set_step_mode(True); g.step_synthetic(3, 1); g.set_step_mode(False)   # ... and a resident worker
    for k in range(3):
        one_tick()
        same_as_whole_frames(f"after other step kinds, tick {k}")
    g.load_track("mountain_track")
    g.step_pilot(3)
    for k in range(2):
        one_tick()
        ref = make_env("hip", n_envs=n, img_h=h, img_w=w, depth=True, track="mountain_track")
        ref.step(0.0, 0.0, 0.0)
        ref.set_pose(prev["pos_x"], prev["pos_y"], prev["pos_z"], prev["yaw"], prev["vel"])
        ref.step(*last_ctl)
        assert np.array_equal(ref.fetch("img"), g.fetch("img")), f"after a track reload, tick {k}"


def test_cnn_2d_model_type_closed_loop(make_env):
    """ModelType.CNN_2D (keras_pilot.py:56-64): the same network, outputs are (steering, throttle) capped to [-1, 1],
    breaking 0, smooth steering applied - against the loop done by hand."""
    n = 16
    ws = make_weights(120, 160, seed=6)
    ws[-1] = ws[-1] + np.float32([0.0, 0.6])                         # bias the throttle output so that the cars move
    cfg = {"model_type": "cnn_2d", "smooth_steering_enabled": True, "smooth_steering_threshold": 0.02}
    a = make_env("hip", n_envs=n)
    b = make_env("hip", n_envs=n)
    a.pilot_load(ws); b.pilot_load(ws)
    a.step_pilot(6, cfg)
    b.step(0.0, 0.0, 0.0)                                            # tick 1: no frame yet
    for _ in range(5):
        out = b.pilot_forward_host(b.fetch("img"))
        steer = np.clip(out[:, 0], -1.0, 1.0)
        steer = np.where(steer > 0.02, 1.0, np.where(steer < -0.02, -1.0, steer)).astype(np.float32)
        b.step(steer, np.clip(out[:, 1], -1.0, 1.0), 0.0)
    for name in ("pos_x", "pos_z", "yaw", "speed", "seg_idx", "img", "ctl_steer", "ctl_thr", "ctl_brk"):
        assert np.array_equal(a.fetch(name), b.fetch(name)), name   # no transcendental in this post-processing: bit for bit
    assert a.fetch("speed").max() > 0.1 and np.all(a.fetch("ctl_brk") == 0.0)
    with pytest.raises(RuntimeError, match="model_type"):
        a.step_pilot(1, {"model_type": "cnn_2d_full_house"})         # a valid type, but not what the 22 loaded arrays can serve
    with pytest.raises(ValueError, match="model_type"):
        a.step_pilot(1, {"model_type": "lstm"})


def test_break_mode_and_errors(make_env):
    env = make_env("hip", n_envs=4)
    with pytest.raises(RuntimeError, match="no pilot loaded"):
        env.step_pilot(1)
    with pytest.raises(RuntimeError, match="22 arrays"):
        env.pilot_load(make_weights(120, 160)[:10])
    env.pilot_load(make_weights(120, 160, seed=1))
    env.step_pilot(4, {"spd_ctl_break": True, "smooth_steering_enabled": True, "smooth_steering_threshold": 0.0})
    assert env.fetch("ep_len").max() >= 2
    with pytest.raises(RuntimeError, match="camera"):
        phys = make_env("hip", n_envs=2, render=False)
        phys.pilot_load(make_weights(120, 160))
        phys.step_pilot(1)


def test_keras_pilot_component_contract(tmp_path):
    """HipKerasPilot: KerasPilot's ports / modes / post-processing (keras_pilot.py:17-153) around the GPU network."""
    from triton_racer_sim_amd.components import HipKerasPilot, PILOT_INPUTS, PILOT_OUTPUTS
    ws = make_weights(120, 160, seed=4)
    path = str(tmp_path / "model.npz")
    np.savez(path, *ws)
    cfg = {"spd_ctl_threshold": 1.1, "smooth_steering_enabled": True, "smooth_steering_threshold": 0.02}
    part = HipKerasPilot(cfg, model_path=path, model_type="cnn_2d_speed_control")
    assert part.step_inputs == PILOT_INPUTS and part.step_outputs == PILOT_OUTPUTS and part.getName() == "Keras Pilot"
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
    assert part.step(None, 3.0, 0.0, 0.0, "ai") == (0.0, 0.0, 0.0)                 # no frame yet (keras_pilot.py:46-47)
    assert part.step(frame, 3.0, 0.0, 0.0, "human") == (0.0, 0.0, 0.0)             # not an AI mode (:139)
    raw = part.env.pilot_forward_host(frame[None])[0]
    got = part.step(frame, 3.0, 0.0, 0.0, "ai_steering")
    st, thr, brk = pilot_postprocess(raw, 3.0, cfg)
    st = 1.0 if st > 0.02 else (-1.0 if st < -0.02 else st)                        # smooth steering (:147-153)
    assert all(isinstance(v, float) for v in got)
    assert abs(got[0] - st) < 1e-6 and abs(got[1] - thr) < 1e-5 and got[2] == brk == 0.0
    part.onShutdown()
    brake = HipKerasPilot(dict(cfg, spd_ctl_break=True, smooth_steering_enabled=False), weights=ws, n_cars=3)
    frames = rng.integers(0, 256, (3, 120, 160, 3), dtype=np.uint8)
    speeds = np.array([0.0, 6.0, 25.0])
    s3, t3, b3 = brake.step(frames, speeds, None, None, "ai")
    raws = brake.env.pilot_forward_host(frames)
    for i in range(3):
        want = pilot_postprocess(raws[i], float(speeds[i]), dict(cfg, spd_ctl_break=True))
        assert abs(s3[i] - want[0]) < 1e-6 and abs(t3[i] - want[1]) < 1e-5 and abs(b3[i] - want[2]) < 1e-5
    brake.onShutdown()
    direct = HipKerasPilot(dict(cfg, smooth_steering_enabled=False), weights=ws, model_type="cnn_2d")     # ModelType.CNN_2D (:56-64)
    raw = direct.env.pilot_forward_host(frame[None])[0]
    got = direct.step(frame, 3.0, 0.0, 0.0, "ai")
    assert got == (float(np.clip(np.float64(raw[0]), -1, 1)), float(np.clip(np.float64(raw[1]), -1, 1)), 0.0)
    direct.onShutdown()
    with pytest.raises(ValueError, match="needs the 42 arrays"):
        HipKerasPilot(cfg, weights=ws, model_type="cnn_2d_full_house")     # another architecture's weights
    with pytest.raises(ValueError, match="model types"):
        HipKerasPilot(cfg, weights=ws, model_type="lstm")


def test_pilot_is_deterministic(make_env):
    """No atomics anywhere: the same frames give bit-identical outputs, and two closed loops stay identical step by step."""
    n = 96
    ws = make_weights(120, 160, seed=9)
    a = make_env("hip", n_envs=n, auto_reset=True)
    b = make_env("hip", n_envs=n, auto_reset=True)
    for env in (a, b):
        env.pilot_load(ws)
        env.step_synthetic(5, 1)
    frames = a.fetch("img")
    r1, r2, r3 = a.pilot_forward_host(frames), a.pilot_forward_host(frames), b.pilot_forward_host(frames)
    assert np.array_equal(r1, r2) and np.array_equal(r1, r3)
    for env in (a, b):
        env.step_pilot(25)
    for name in ("pos_x", "pos_z", "yaw", "speed", "cte", "seg_idx", "ep_return", "img"):
        assert np.array_equal(a.fetch(name), b.fetch(name)), name


def test_closed_loop_is_unaffected_by_another_stream(make_env):
    """The pilot loop beside a second handle that keeps its own loop running from a thread (workgroups of other kernels
    share the CUs with the step kernel) gives the states, controls and frames of the same loop run alone.  A race screen:
    an in-place packed multiply in the rasteriser failed it within ~100 steps (scripts/coresidency_probe.py)."""
    import threading
    n, steps = 96, 300
    ws = make_weights(120, 160, seed=9)

    def fresh():
        env = make_env("hip", n_envs=n, auto_reset=True)
        env.pilot_load(ws)
        env.step_synthetic(5, 1)
        return env

    names = ("pos_x", "pos_z", "yaw", "speed", "ctl_steer", "ctl_thr", "img")
    alone = fresh()
    want = []
    for _ in range(steps // 4):
        alone.step_pilot(4)
        want.append([alone.fetch(f) for f in names])
    victim, other = fresh(), fresh()
    stop = threading.Event()

    def busy():
        while not stop.is_set():
            other.step_pilot(8)
            other.sync()

    t = threading.Thread(target=busy)
    t.start()
    try:
        for k in range(steps // 4):
            victim.step_pilot(4)
            for f, w in zip(names, want[k]):
                assert np.array_equal(victim.fetch(f), w), (f, 4 * (k + 1))
    finally:
        stop.set()
        t.join()


@pytest.mark.parametrize("size,wsplit", [((120, 160), None), ((240, 320), None), ((240, 320), 1), ((100, 132), None), ((130, 300), None)])
def test_fused_head_equals_the_two_layers(make_env, planner, size, wsplit):
    """conv1 -> conv2 fused (conv1's activation stays in LDS; trs_conv12_band_kernel) against the two separate kernels (trs_pilot_tuning.no_fuse).
    The band form (120x160 at its whole width; 240x320, 130x300 and 100x132 — whose frame row of 396 bytes is no multiple of 16 — cut in two parts of conv2
    columns of equal width, the last one overlapping its neighbour; the plan is asserted) keeps the conv1 tile
    split by column parity and takes conv2's k dimension in that order (even columns, then odd): the same products in another
    summation order, so an output can land on the neighbouring fp16 value — at most one ulp (2^-10 relative), on a small fraction
    of the elements.  240x320 with fuse_wsplit_max = 1 (a band may not be cut in width, and a whole-width band does not fit LDS): the
    library falls back to the two layers by itself (round 4 removed the direct form of the fused head) — bit-identical by construction,
    and both activations are also checked against the PyTorch mirror."""
    h, w = size
    n = 21
    ws = make_weights(h, w, seed=3)
    env = make_env("hip", n_envs=n, img_h=h, img_w=w, auto_reset=True)
    tune = {} if wsplit is None else {"fuse_wsplit_max": wsplit}
    fused_plan, plain_plan = planner.plan(h, w, n, **tune), planner.plan(h, w, n, no_fuse=1, **tune)
    assert served(plain_plan)[:2] == ["u8", "span<1>"]
    if wsplit == 1:
        assert fused_plan["head"]["on"] == 0 and served(fused_plan)[:2] == ["u8", "span<1>"]      # the documented fallback: both runs are the two layers
    else:
        parts = {(120, 160): 1, (240, 320): 2, (100, 132): 2, (130, 300): 2}[size]
        assert fused_plan["head"]["wsplit"] == parts and served(fused_plan)[:2] == ["band<whole>" if parts == 1 else "band<split>"] * 2
    if tune:
        env.pilot_tuning(**tune)
    env.pilot_load(ws)
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    oh1, ow1 = (h - 5) // 2 + 1, (w - 5) // 2 + 1
    oh2, ow2 = (oh1 - 5) // 2 + 1, (ow1 - 5) // 2 + 1
    fused_out = env.pilot_forward_host(frames)
    fused_l1 = env.pilot_layer(1, (n, oh2, ow2, 32))
    again = env.pilot_forward_host(frames)
    assert np.array_equal(fused_out, again) and np.array_equal(fused_l1, env.pilot_layer(1, (n, oh2, ow2, 32)))
    env.pilot_tuning(no_fuse=1, **tune)
    env.pilot_load(ws)                                                # the choice is read when the weights are loaded
    plain_out = env.pilot_forward_host(frames)
    plain_l1 = env.pilot_layer(1, (n, oh2, ow2, 32))
    mirror_l1 = torch_layer(1, torch_layer(0, frames, ws), ws)         # conv2 of the PyTorch mirror on its own conv1 (fp16-rounded weights and activations)
    dm = np.abs(plain_l1 - mirror_l1)
    assert (dm <= 2.0 ** -9 * np.abs(mirror_l1) + 4e-4).all(), float(dm.max())   # two layers of summation-order roundings
    if wsplit == 1:
        assert np.array_equal(fused_l1, plain_l1)
        assert np.array_equal(fused_out, plain_out)
    else:
        diff = np.abs(fused_l1 - plain_l1)
        assert (diff <= 2.0 ** -10 * np.abs(plain_l1) + 2e-4).all(), float(diff.max())
        assert np.mean(diff > 0) < 0.04, float(np.mean(diff > 0))
        assert np.max(np.abs(fused_out - plain_out)) <= 2e-3


def test_fused_head_conv1_beyond_the_fp16_range(make_env):
    """The fused head's conv1 epilogue skips the saturation step when |bias| + sum |w| < 65504 for every channel (checked when the weights are
    loaded: its inputs are pixels / 256 <= 1).  With conv1's kernel scaled by 3e5 that bound fails: the saturating epilogue runs, conv1's
    activation sits at 65504 where the sums overflow — and the fused head still agrees with the two separate layers (which always saturate);
    everything stays finite."""
    h, w, n = 120, 160, 5
    ws = make_weights(h, w, seed=29)
    ws[0] = ws[0] * np.float32(3e5)
    ws[2] = ws[2] * np.float32(1e-5)                                     # conv2 brings the signal back into range
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    oh1, ow1 = (h - 5) // 2 + 1, (w - 5) // 2 + 1
    oh2, ow2 = (oh1 - 5) // 2 + 1, (ow1 - 5) // 2 + 1
    res = {}
    for no_fuse in (0, 1):
        env = make_env("hip", n_envs=n, img_h=h, img_w=w, auto_reset=True)
        env.pilot_tuning(no_fuse=no_fuse)
        env.pilot_load(ws)
        out = env.pilot_forward_host(frames)
        res[no_fuse] = (out, env.pilot_layer(1, (n, oh2, ow2, 32)), env.pilot_layer(0, (n, oh1, ow1, 24)))
    assert np.isfinite(res[0][0]).all() and np.isfinite(res[0][1]).all()
    assert res[1][2].max() == 65504.0                                    # conv1 saturates with these weights
    diff = np.abs(res[0][1] - res[1][1])
    assert (diff <= 2.0 ** -9 * np.abs(res[1][1]) + 1e-2).all(), float(diff.max())
    assert np.abs(res[1][1]).max() > 0.1


@pytest.mark.parametrize("size,n", [((120, 160), 300), ((240, 320), 150), ((130, 300), 131)])
def test_fused_head_rolling_bands_are_bit_identical_to_one_band_per_item(make_env, planner, size, n):
    """Round 3: with a (frame, part) stream per CU or more, a workgroup of the band-form head walks a frame's bands top to bottom and keeps
    the three conv1 rows two neighbouring bands share in a ring (trs_pilot_tuning.fuse_roll, the default) instead of computing them
    twice.  Same values into the same MFMAs: conv2's activation and the model's outputs must equal the one-band-per-item order bit for
    bit — whole streams per workgroup and a ragged last round (n not a multiple of the CU count), the width-split form (equal parts since round 4: the last one overlaps its neighbour)."""
    h, w = size
    ws = make_weights(h, w, seed=5)
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    oh2, ow2 = ((h - 5) // 2 + 1 - 5) // 2 + 1, ((w - 5) // 2 + 1 - 5) // 2 + 1
    for roll in (1, 0):                                                # the batch is large enough for the default to roll, and the tuning field turns it off
        call = planner.call(h, w, n, n, fuse_roll=roll)
        assert (call["head_runs"], call["roll"]) == (1, roll), call
    res = {}
    for roll in (1, 0):
        env = make_env("hip", n_envs=n, img_h=h, img_w=w, auto_reset=True)
        env.pilot_tuning(fuse_roll=roll)
        env.pilot_load(ws)
        out = env.pilot_forward_host(frames)
        res[roll] = (out, env.pilot_layer(1, (n, oh2, ow2, 32)))
        del env
    assert np.array_equal(res[1][1], res[0][1])
    assert np.array_equal(res[1][0], res[0][0])


@pytest.mark.parametrize("size,n", [((120, 160), 77), ((240, 320), 40), ((240, 320), 77), ((100, 132), 5), ((120, 160), 1), ((240, 320), 150)])
def test_dense_kernel_against_torch_in_both_frame_groupings(make_env, planner, size, n):
    """dense1 on trs_pilot_dense_kernel against fp32 PyTorch on the kernel's own conv7 activation (the chunked 1x1-convolution kernel it
    was compared with until round 3 is gone), in both of its forms: 64 frames per workgroup where K is long enough that every workgroup keeps two
    LDS chunks or more (240x320 on 256 CUs: 129 frames or more — of these cases only 150) and 32 frames per workgroup (trs_pilot_tuning.dense = 2, and
    the default everywhere else) — the same fp16 products, K and frames split differently: fp32 summation order only.  The plan is asserted: at
    240x320 with 150 frames the two runs are trs_pilot_dense_kernel<2> and <1>; in every other case both runs are <1>, so the comparison between
    the runs says nothing there and the check is the one against PyTorch.  n is not a multiple of 32 / 64 (ragged last frame group) and spans
    several groups; 240x320 needs several LDS chunks per slice and a ragged last one."""
    h, w = size
    ws = make_weights(h, w, seed=5)
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    outs, h1s, l6 = {}, {}, {}
    oh, ow = h, w
    for k, s_, _, _ in SPEC:
        oh, ow = (oh - k) // s_ + 1, (ow - k) // s_ + 1
    nf = {mode: planner.call(h, w, n, n, dense=int(mode))["nf"] for mode in ("1", "2")}
    assert nf == {"1": 2 if (size, n) == ((240, 320), 150) else 1, "2": 1}
    for mode in ("1", "2"):                                           # 2: always 32 frames per workgroup (1 takes 64 where K is long: 240x320 with n >= 129)
        env = make_env("hip", n_envs=n, img_h=h, img_w=w, auto_reset=True)
        env.pilot_tuning(dense=int(mode))
        env.pilot_load(ws)
        for rep in range(2):
            outs[mode] = env.pilot_forward_host(frames)
        h1s[mode] = env.pilot_layer(7, (n, 100))
        l6[mode] = env.pilot_layer(6, (n, oh, ow, 128))
    want = torch_layer(7, l6["1"], ws)                                # fp32 dense1 on the kernel's own conv7 activation
    assert np.max(np.abs(h1s["1"] - want)) <= 1e-3 * max(1.0, float(np.abs(want).max()))
    assert np.max(np.abs(h1s["2"] - want)) <= 1e-3 * max(1.0, float(np.abs(want).max()))
    assert np.max(np.abs(outs["2"] - outs["1"])) <= 1e-4
    assert np.array_equal(l6["2"], l6["1"])
    assert n == 1 or np.std(outs["1"][:, 0]) > 1e-5


@pytest.mark.parametrize("size,n", [((120, 160), 37), ((120, 160), 1027), ((100, 132), 9), ((240, 320), 6), ((120, 160), 1)])
@pytest.mark.parametrize("layers", ["4", "3"])
def test_conv_chain_is_bit_identical_to_the_single_layers(make_env, planner, size, n, layers):
    """conv4..conv7 (or conv5..conv7) in one launch with the activations in LDS (trs_conv_chain_kernel) against one launch per
    layer (trs_pilot_tuning.chain_layers = 0): the same MFMA order on the same fp16 values, so every activation — the interior ones are
    recomputed by the debug getter — and the outputs agree bit for bit.  37 frames: 2 frames per workgroup, odd tail; 1027: 4 per
    workgroup with a ragged last one (3 frames: the second conv4 pass has one frame); 100x132 and one frame: 2 per workgroup; 240x320 does not fit
    LDS: no chain, both runs go layer by layer (the plan is asserted)."""
    h, w = size
    ws = make_weights(h, w, seed=9)
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    shapes, (ih, iw) = [], (h, w)
    for k, s_, _, cout in SPEC:
        ih, iw = (ih - k) // s_ + 1, (iw - k) // s_ + 1
        shapes.append((n, ih, iw, cout))
    on, off = planner.plan(h, w, n, chain_layers=int(layers)), planner.plan(h, w, n, chain_layers=0)
    assert off["chain"]["first"] == -1 and "chain" not in served(off)
    if size == (240, 320):
        assert on["chain"]["first"] == -1 and served(on) == served(off)
    else:
        assert (on["chain"]["nl"], on["chain"]["F"]) == (int(layers), 4 if n == 1027 else 2)
        assert served(on)[3:] == ["frame"] * (4 - int(layers)) + ["chain"] * int(layers) and served(off)[3:] == ["frame"] * 4
    res = {}
    for mode in ("0", layers):
        env = make_env("hip", n_envs=n, img_h=h, img_w=w, auto_reset=True)
        env.pilot_tuning(chain_layers=int(mode))
        env.pilot_load(ws)
        out = env.pilot_forward_host(frames)
        out = env.pilot_forward_host(frames)
        res[mode] = [out] + [env.pilot_layer(i, shapes[i]) for i in (6, 5, 4, 3, 2)]
    for a, b in zip(res["0"], res[layers]):
        assert np.array_equal(a, b)
    assert n == 1 or np.std(res[layers][0][:, 0]) > 1e-5


@pytest.mark.parametrize("size,n", [((120, 160), 37), ((120, 160), 1027), ((100, 132), 9), ((240, 320), 11)])
def test_conv3_with_frames_in_lds_is_bit_identical_to_the_span_kernel(make_env, planner, size, n):
    """conv3 on trs_conv_frame5_kernel (input frames in LDS, even / odd column planes, weights from L2) against the span kernel
    (trs_pilot_tuning.frame5 = 0): the same k order on the same fp16 values — conv3's activation and the outputs agree bit for bit.  240x320: the input frame (281 KB)
    is cut into 5 bands of 6 output rows (the last has 3)."""
    h, w = size
    ws = make_weights(h, w, seed=13)
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    (ih, iw) = (h, w)
    for k, s_, _, cout in SPEC[:3]:
        ih, iw = (ih - k) // s_ + 1, (iw - k) // s_ + 1
    on, off = planner.plan(h, w, n, frame5=2), planner.plan(h, w, n, frame5=0)
    assert served(on)[2] == "frame5" and served(off)[2] == "span<2>"
    assert on["layers"][2]["frame5_bands"] == (5 if size == (240, 320) else 1)
    res = {}
    for mode in ("0", "2"):                                          # 2: also when the frame has to be cut into row bands
        env = make_env("hip", n_envs=n, img_h=h, img_w=w, auto_reset=True)
        env.pilot_tuning(frame5=int(mode))
        env.pilot_load(ws)
        out = env.pilot_forward_host(frames)
        res["1" if mode == "2" else mode] = (out, env.pilot_layer(2, (n, ih, iw, 64)))
    # both kernels start their accumulators at the bias and take the k dimension in the same order: bit for bit
    assert np.array_equal(res["0"][1], res["1"][1])
    assert np.array_equal(res["0"][0], res["1"][0])
    assert np.abs(res["1"][1]).max() > 0


def _range_weights(h, w, seed, conv2_peak):
    """Glorot weights rescaled so that conv2's activations peak at ``conv2_peak`` (fp32 reference on noise + flat frames) and the following two
    layers scale the signal back down by the same factor — the network's outputs stay O(1) while one activation tensor sits at the top of
    (or beyond) binary16's range."""
    ws = make_weights(h, w, seed=seed)
    rng = np.random.default_rng(seed)
    frames = np.concatenate([rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8), np.full((1, h, w, 3), 255, np.uint8)])
    a1 = torch_layer(0, frames, ws, mirror=False)
    a2 = torch_layer(1, a1, ws, mirror=False)
    s = float(conv2_peak) / float(a2.max())
    r = math.sqrt(s)
    ws[2] = ws[2] * np.float32(s); ws[3] = ws[3] * np.float32(s)       # conv2: kernel and bias
    ws[4] = ws[4] / np.float32(r); ws[6] = ws[6] / np.float32(r)       # conv3, conv4: kernels only (their inputs are s / r and 1 x too large)
    return ws, frames


def test_fp16_range_top_of_the_range_and_saturation_count(make_env):
    """the reference runs the network in fp32 (components/keras_pilot.py:49-59); this library stores activations as fp16 and
    saturates at 65504.  (a) Activations up to ~3e4 (conv2) — inside the range: no saturation is counted (trs_pilot_range_check, TRS_F_STATS[3])
    and the outputs agree with fp32 PyTorch to 2e-3 of the output scale (fp16's 2^-11 relative rounding per stored activation; measured value
    printed).  (b) The same network pushed to a conv2 peak of ~2.6e5 — beyond the range: the check reports saturated elements in conv2 and
    nothing downstream of the clamp is an infinity or a NaN."""
    h, w = 120, 160
    env = make_env("hip", n_envs=4, img_h=h, img_w=w)
    ws, frames = _range_weights(h, w, seed=23, conv2_peak=3.0e4)
    env.pilot_load(ws)
    out = env.pilot_forward_host(frames)
    a2 = env.pilot_layer(1, (4,) + tuple(torch_layer(1, torch_layer(0, frames, ws), ws).shape[1:]))
    assert 1.0e4 <= a2.max() < 65504.0, float(a2.max())
    sat = env.pilot_range_check()
    assert sat.sum() == 0, sat
    assert int(env.fetch("stats")[3]) == 0
    pure = torch_pure(frames, ws)
    scale = max(1.0, float(np.abs(pure).max()))
    rel = float(np.max(np.abs(out - pure))) / scale
    print(f"conv2 peak {a2.max():.0f}: max |HIP - fp32| / scale = {rel:.2e} (outputs {out[0]}, fp32 {pure[0]})")
    assert rel <= 2e-3, rel
    # (b) beyond the range
    ws_hi, _ = _range_weights(h, w, seed=23, conv2_peak=2.6e5)
    env.pilot_load(ws_hi)
    out_hi = env.pilot_forward_host(frames)
    sat_hi = env.pilot_range_check()
    print(f"conv2 peak 2.6e5: saturated elements per layer {sat_hi[:7]}, outputs {out_hi[0]}")
    assert sat_hi[1] > 0 and sat_hi[7] == sat_hi[:7].sum()
    assert int(env.fetch("stats")[3]) == int(sat_hi[7])
    assert np.isfinite(out_hi).all()
    a2_hi = env.pilot_layer(1, a2.shape)
    assert a2_hi.max() == 65504.0 and np.isfinite(a2_hi).all()


def _all_layers_large_weights(h, w, seed, peak):
    """Glorot weights rescaled LAYER BY LAYER (fp32 reference on noise + a white frame) so that EVERY convolution's activation tensor peaks at ``peak``:
    each kernel and bias are multiplied by peak / (the layer's fp32 maximum given the rescaled layers in front of it); dense1's kernel is divided by the
    last factor chain so that the network's outputs stay O(1)."""
    ws = make_weights(h, w, seed=seed)
    rng = np.random.default_rng(seed)
    frames = np.concatenate([rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8), np.full((1, h, w, 3), 255, np.uint8)])
    x = frames
    for i in range(7):
        a = torch_layer(i, x, ws, mirror=False)
        s = np.float32(float(peak) / float(a.max()))
        ws[2 * i] = ws[2 * i] * s; ws[2 * i + 1] = ws[2 * i + 1] * s
        x = torch_layer(i, x, ws, mirror=False)
    ws[14] = ws[14] * np.float32(1.0 / float(peak))                       # dense1 sees conv7 at `peak`
    return ws, frames


@pytest.mark.gpu
def test_fp16_activations_at_1e3_to_1e4_through_all_seven_convolutions(make_env):
    """the reference computes in fp32 (components/keras_pilot.py:49-59); here every stored activation is binary16.  With every convolution's
    activations peaking at 2e4 (typical values 1e3-1e4: four orders of magnitude above Glorot-random networks, whose |outputs| <~ 0.05) nothing saturates, and the
    error against fp32 PyTorch stays at binary16's rounding: per layer, fed the kernel's own previous activation, <= one ulp (2^-10 relative) + an absolute term
    for sums that cancel; end to end, against fp32 everywhere, the relative error of the outputs is printed and bounded by 3e-3 of the output scale
    (seven stored activations at 2^-11 relative each, amplified by cancellation in dense1's 4,608-term sums)."""
    h, w = 120, 160
    env = make_env("hip", n_envs=4, img_h=h, img_w=w)
    ws, frames = _all_layers_large_weights(h, w, seed=31, peak=2.0e4)
    env.pilot_load(ws)
    out = env.pilot_forward_host(frames)
    assert env.pilot_range_check().sum() == 0
    x = frames
    for layer in range(7):
        want = torch_layer(layer, x, ws)                                   # mirror arithmetic on the kernel's own input
        got = env.pilot_layer(layer, want.shape)
        assert 5.0e3 <= got.max() < 65504.0, (layer, float(got.max()))
        assert np.median(got[got > 0]) >= 2.0e2, (layer, float(np.median(got[got > 0])))
        diff = np.abs(got - want)
        assert (diff <= 2.0 ** -10 * np.abs(want) + 2e-4 * float(want.max())).all(), (layer, float(diff.max()))
        x = got
    pure = torch_pure(frames, ws)
    scale = max(1.0, float(np.abs(pure).max()))
    rel = float(np.max(np.abs(out - pure))) / scale
    print(f"all seven convolutions at a peak of 2e4: max |HIP - fp32 PyTorch| / output scale = {rel:.2e} (outputs {out[0]}, fp32 {pure[0]})")
    assert rel <= 3e-3, rel
