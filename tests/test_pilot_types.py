"""The other two model types the reference's KerasPilot serves (components/keras_pilot.py:67-76,97-118):
``cnn_2d_speed_as_feature`` = Keras_2D_CNN.get_model(num_feature_vectors=1) (components/keras_train.py:127-174,390-392) and
``cnn_2d_full_house`` = Keras_2D_FULL_HOUSE.get_model (keras_train.py:184-245).  The checker is a plain PyTorch fp32 restatement
of those architectures with seeded random weights (no model file ships; TensorFlow is absent): conv stack as in
tests/test_pilot.py, the small dense branches and both heads in fp32.  Tolerances as for cnn_2d_speed_control: the two outputs
within 1e-3 of fp32-everywhere (the fp16 effect of the conv stack; 5e-2 in the bfloat16 rounds), and within 5e-4 of a reference whose conv stack is the
kernel's own conv7 activation (everything behind it is fp32 on both sides).
The forward passes here are 6 frames in 8 K slices: one frame group, whole groups of 8 in trs_pilot_tail_ex_kernel.  Its remainder loop, dense4 with several frame
groups and 64 frames per workgroup, and a batch change on one handle are in tests/test_pilot_slices.py, which uses make_named_weights and torch_heads from here
(hence their cnn_2d_speed_control branch and torch_heads' ``flat``)."""
import math

import numpy as np
import pytest

from test_pilot import SPEC, make_weights, pilot_postprocess, torch_layer

pytestmark = pytest.mark.gpu


def dense_init(rng, a, b):
    lim = math.sqrt(6.0 / (a + b))
    return rng.uniform(-lim, lim, (a, b)).astype(np.float32), rng.uniform(-0.05, 0.05, b).astype(np.float32)


def make_named_weights(h, w, kind, seed=0):
    """{layer name: (kernel, bias)} in Keras layouts for the two architectures."""
    rng = np.random.default_rng(seed)
    base = make_weights(h, w, seed=seed + 100)
    named = {f"conv{i + 1}": (base[2 * i], base[2 * i + 1]) for i in range(7)}
    ih, iw = h, w
    for k, s, _, _ in SPEC:
        ih, iw = (ih - k) // s + 1, (iw - k) // s + 1
    F = ih * iw * 128
    if kind == "cnn_2d_speed_control":                                # no extra input: tests/test_pilot_slices.py runs all three types through one reference
        named["dense1"] = dense_init(rng, F, 100)
        named["dense2"], named["dense3"], named["output_layer"] = dense_init(rng, 100, 50), dense_init(rng, 50, 25), dense_init(rng, 25, 2)
    elif kind == "cnn_2d_speed_as_feature":
        f = (4, 8, 16)
        named["feature1"], named["feature2"], named["feature3"] = dense_init(rng, 1, f[0]), dense_init(rng, f[0], f[1]), dense_init(rng, f[1], f[2])
        named["dense1"] = dense_init(rng, F + f[2], 100)
        named["dense2"], named["dense3"], named["output_layer"] = dense_init(rng, 100, 50), dense_init(rng, 50, 25), dense_init(rng, 25, 2)
    else:
        f = (16, 32, 64)
        named["feature1"], named["feature2"], named["feature3"] = dense_init(rng, 1, f[0]), dense_init(rng, f[0], f[1]), dense_init(rng, f[1], f[2])
        named["current_spd_1"], named["current_spd_2"], named["current_spd_3"] = dense_init(rng, 1, f[0]), dense_init(rng, f[0], f[1]), dense_init(rng, f[1], f[2])
        named["dense1"] = dense_init(rng, F + 64, 100)
        named["dense2"], named["dense3"], named["output_speed"] = dense_init(rng, 100, 50), dense_init(rng, 50, 25), dense_init(rng, 25, 1)
        named["dense4"] = dense_init(rng, F + 128, 100)
        named["dense5"], named["dense6"], named["out_steering"] = dense_init(rng, 100, 50), dense_init(rng, 50, 25), dense_init(rng, 25, 1)
    # give the extra rows of dense1 / dense4 weight: the branches must matter for the test to see them
    for nm in ("dense1", "dense4"):
        if nm in named:
            k, b = named[nm]
            k[F:] *= 20.0
    return named, F


def torch_heads(x_flat, speed, segment, named, kind, h16_dense=False, flat=None):
    """Everything behind the flatten, fp32 (with ``h16_dense`` the flatten rows of dense1 / dense4 and x are rounded to fp16, as the
    matrix-core path does).  ``flat``: {"dense1": float32[n, 100] (, "dense4": ...)}, the products of the flatten with the flatten rows worked out by the
    caller (tests/test_pilot_slices.py: in binary64, slice by slice, with a slice left out), used in place of x @ k[:F]; ``x_flat`` is not read then."""
    import torch
    import torch.nn.functional as Fn
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    lin = lambda z, nm, act=True: (Fn.relu(z @ t(named[nm][0]) + t(named[nm][1])) if act else z @ t(named[nm][0]) + t(named[nm][1]))
    x = None if flat is not None else t(x_flat)

    def big(z_extra, nm):
        k, b = t(named[nm][0]), t(named[nm][1])
        F = k.shape[0] - (0 if z_extra is None else z_extra.shape[1])
        if flat is not None:
            prod = t(flat[nm])
        else:
            kx = k[:F].half().float() if h16_dense else k[:F]
            xx = x.half().float() if h16_dense else x
            prod = xx @ kx
        return Fn.relu(prod + b if z_extra is None else prod + z_extra @ k[F:] + b)

    if kind == "cnn_2d_speed_control":
        return lin(lin(lin(big(None, "dense1"), "dense2"), "dense3"), "output_layer", act=False).numpy()
    spd = t(speed).reshape(-1, 1) / 20.0
    if kind == "cnn_2d_speed_as_feature":
        y = lin(lin(lin(spd, "feature1"), "feature2"), "feature3")
        z = big(y, "dense1")
        return lin(lin(lin(z, "dense2"), "dense3"), "output_layer", act=False).numpy()
    y = lin(lin(lin(t(segment).reshape(-1, 1), "feature1"), "feature2"), "feature3")
    s = lin(lin(lin(spd, "current_spd_1"), "current_spd_2"), "current_spd_3")
    out_speed = lin(lin(lin(big(y, "dense1"), "dense2"), "dense3"), "output_speed", act=False)
    out_steer = lin(lin(lin(big(torch.cat([y, s], 1), "dense4"), "dense5"), "dense6"), "out_steering", act=False)
    return torch.cat([out_steer, out_speed], 1).numpy()


def conv_stack_pure(frames, named):
    ws = [a for i in range(7) for a in named[f"conv{i + 1}"]]
    x = frames
    for i in range(7):
        x = torch_layer(i, x, ws, mirror=False)
    return x.reshape(x.shape[0], -1)


@pytest.mark.parametrize("kind", ["cnn_2d_speed_as_feature", "cnn_2d_full_house"])
def test_forward_matches_torch_fp32(make_env, kind):
    h, w, n = 120, 160, 6
    env = make_env("hip", n_envs=n, img_h=h, img_w=w, auto_reset=True)
    named, F = make_named_weights(h, w, kind, seed=3)
    env.pilot_load(named)
    env.step_synthetic(12, 1)
    rng = np.random.default_rng(1)
    frames = np.concatenate([env.fetch("img")[:4], rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)])
    speed = rng.uniform(0, 20, n).astype(np.float32)
    segment = rng.uniform(0, 10, n).astype(np.float32)
    out = env.pilot_forward_host(frames, speed=speed, segment=segment if kind == "cnn_2d_full_house" else None)
    pure = torch_heads(conv_stack_pure(frames, named), speed, segment, named, kind)
    assert np.max(np.abs(out - pure)) <= 1e-3, float(np.max(np.abs(out - pure)))
    oh, ow = h, w
    for k, s_, _, _ in SPEC:
        oh, ow = (oh - k) // s_ + 1, (ow - k) // s_ + 1
    shape7 = (n, oh, ow, 128)
    x7 = env.pilot_layer(6, shape7).reshape(n, -1)                    # the kernel's own conv7 activation (fp16 values as fp32)
    assert x7.shape[1] == F
    mirror = torch_heads(x7, speed, segment, named, kind, h16_dense=True)
    assert np.max(np.abs(out - mirror)) <= 5e-4, float(np.max(np.abs(out - mirror)))
    # the extra inputs are really read: other speeds / segments, other outputs
    out2 = env.pilot_forward_host(frames, speed=speed[::-1].copy(), segment=(segment[::-1].copy() if kind == "cnn_2d_full_house" else None))
    assert np.max(np.abs(out2 - out)) > 1e-3
    again = env.pilot_forward_host(frames, speed=speed, segment=segment if kind == "cnn_2d_full_house" else None)
    assert np.array_equal(again, out)                                 # fixed summation orders: bit-identical reruns


@pytest.mark.parametrize("kind", ["cnn_2d_speed_as_feature", "cnn_2d_full_house"])
def test_closed_loop_equals_the_loop_done_by_hand(make_env, kind):
    """trs_step_pilot with the env's own speed / tracker index == [forward(previous frame, speed, segment); KerasPilot's
    post-processing; env.step] by hand (keras_pilot.py:67-76 / 97-118)."""
    n = 16
    named, _ = make_named_weights(120, 160, kind, seed=8)
    out_name = "output_layer" if kind == "cnn_2d_speed_as_feature" else "output_speed"
    k, b = named[out_name]
    named[out_name] = (k, b + np.float32(0.5))                        # bias towards driving
    cfg = {"model_type": kind, "spd_ctl_threshold": 1.1, "spd_ctl_reverse_multiplier": 1.0}
    a, bb = make_env("hip", n_envs=n), make_env("hip", n_envs=n)
    a.pilot_load(named); bb.pilot_load(named)
    a.step_pilot(6, cfg)
    bb.step(0.0, 0.0, 0.0)
    for _ in range(5):
        spd = bb.fetch("speed")
        seg = bb.segment(bb.fetch("seg_idx")).astype(np.float32)      # 'loc/segment' = idx / n_points * 10 (track_data_process.py:106-107)
        out = bb.pilot_forward_host(bb.fetch("img"), speed=spd, segment=seg if kind == "cnn_2d_full_house" else None)
        if kind == "cnn_2d_speed_as_feature":
            ctl = np.stack([np.clip(out[:, 0], -1, 1), np.clip(out[:, 1], -1, 1), np.zeros(n, np.float32)], 1).astype(np.float32)
        else:
            ctl = np.array([pilot_postprocess(out[i], float(spd[i]), cfg) for i in range(n)], dtype=np.float32)
        bb.step(ctl[:, 0], ctl[:, 1], ctl[:, 2])
    for name in ("pos_x", "pos_z", "yaw", "speed"):
        assert np.max(np.abs(a.fetch(name) - bb.fetch(name))) <= 1e-4, name
    assert np.array_equal(a.fetch("seg_idx"), bb.fetch("seg_idx")) and np.array_equal(a.fetch("img"), bb.fetch("img"))
    assert a.fetch("speed").max() > 0.05
    with pytest.raises(RuntimeError, match="model_type"):
        a.step_pilot(1, {"model_type": "cnn_2d_speed_control"})       # the loaded weights are another architecture's


STEP_RULE_CONFIGS = {"default": {}, "break": {"spd_ctl_break": True}, "smooth": {"smooth_steering_enabled": True, "smooth_steering_threshold": 0.02},
                     "break+smooth": {"spd_ctl_break": True, "smooth_steering_enabled": True, "smooth_steering_threshold": 0.02}}


@pytest.mark.parametrize("kind", ["cnn_2d_speed_control", "cnn_2d", "cnn_2d_speed_as_feature", "cnn_2d_full_house"])
def test_keras_pilot_step_rule_for_every_model_type(make_env, kind):
    """KerasPilot.step behind the network (keras_pilot.py:56-118,139-153; mapping.py:23-35) through trs_pilot_act, for every model type, config and mode.
    The output layers get zero kernels and a chosen bias, so the raw outputs ARE the bias (asserted bit for bit) and everything the rule sees is known here:
    predicted speed 0.3 x 20 = 6.0, target 6.6 at threshold 1.1.  5 cars of 100x132 frames: four per workgroup, the second workgroup has three idle waves.
    Speeds 0 / 6.5 / 6.7 / 12 / 25 give full throttle, a small positive one, the (-0.2, 0) dead zone, reverse, and a brake above the 0.4 cut; every one
    lies >= 1e-3 from every cut-off (checked below), so the 1e-5 on the atan values (tests/test_pilot.py's tolerance for the same quantities) decides no branch."""
    from triton_racer_sim_amd.env import SLOT_JPEG_IN, SLOT_MODE, SLOT_PILOT_IN
    h, w, n = 100, 132, 5
    f32 = np.float32
    capped = kind in ("cnn_2d", "cnn_2d_speed_as_feature")
    speeds = np.array([0.0, 6.5, 6.7, 12.0, 25.0], f32)
    modes = np.array([2, 0, 1, 2, 7], np.uint8)                        # ai, human, ai_steering, ai, no mode at all
    speed_bias, threshold = f32(0.3), f32(1.1)
    half_pi = math.pi / 2

    # where the speeds lie relative to the rule's cut-offs, in binary64
    target = float(speed_bias) * 20 * float(threshold) - speeds.astype(np.float64)
    thr64, brk64 = np.arctan(target * 2) / half_pi, -np.arctan(target) / half_pi
    assert min(np.abs(thr64 + 0.2).min(), np.abs(thr64).min(), np.abs(brk64 - 0.4).min(), np.abs(float(speed_bias) * 20 - speeds).min()) >= 1e-3
    assert thr64[0] > 0.9 and 0 < thr64[1] < 0.2 and -0.2 < thr64[2] < 0 and thr64[3] < -0.9 and brk64[4] > 0.4 and (brk64[:3] < 0.4).all()

    def want(out0, i, cfg, mode):
        """(steering, throttle, breaking, throttle and breaking are atan values) of car i in float32"""
        if mode not in (1, 2):
            return f32(0), f32(0), f32(0), False
        steer = min(max(f32(out0), f32(-1)), f32(1))
        if capped:
            thr, brk, soft = min(max(speed_bias, f32(-1)), f32(1)), f32(0), False
        else:
            pred = speed_bias * f32(20)
            delta = f32(pred * threshold) - speeds[i]
            thr, brk, soft = f32(math.atan(float(delta * f32(2))) / half_pi), f32(0), True
            if -0.2 < thr < 0.0:
                thr = f32(0)
            if cfg.get("spd_ctl_break"):
                thr = f32(1) if pred - speeds[i] > 0 else f32(0)
                brk = f32(-math.atan(float(delta)) / half_pi)
                if brk < 0.4:
                    brk = f32(0)
        if cfg.get("smooth_steering_enabled"):
            t = f32(cfg["smooth_steering_threshold"])
            steer = f32(1) if steer > t else (f32(-1) if steer < -t else steer)
        return steer, thr, brk, soft

    env = make_env("hip", n_envs=n, img_h=h, img_w=w)
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    segment = rng.uniform(0, 10, n).astype(f32)
    full = kind == "cnn_2d_full_house"
    d_frames, d_mode = env.scratch(SLOT_JPEG_IN, (n, h, w, 3), np.uint8), env.scratch(SLOT_MODE, (n,), np.uint8)
    d_speed, d_segment = (env.scratch(s, (n,), f32) for s in SLOT_PILOT_IN)
    env.upload(d_frames, frames); env.upload(d_mode, modes); env.upload(d_speed, speeds); env.upload(d_segment, segment)
    bits = lambda a: np.asarray(a, f32).view(np.uint32)
    for steer_bias in (f32(0.5), f32(-0.01), f32(-1.7)):
        assert min(abs(abs(float(steer_bias)) - c) for c in (1.0, 0.02)) >= 1e-3
        if kind in ("cnn_2d_speed_control", "cnn_2d"):
            named = make_weights(h, w, seed=6)
            named[20], named[21] = np.zeros_like(named[20]), np.array([steer_bias, speed_bias], f32)
        else:
            named, _ = make_named_weights(h, w, kind, seed=6)
            if full:
                named["out_steering"] = (np.zeros((25, 1), f32), np.array([steer_bias], f32))
                named["output_speed"] = (np.zeros((25, 1), f32), np.array([speed_bias], f32))
            else:
                named["output_layer"] = (np.zeros((25, 2), f32), np.array([steer_bias, speed_bias], f32))
        env.pilot_load(named)
        raw = env.pilot_forward_host(frames, speed=None if kind in ("cnn_2d_speed_control", "cnn_2d") else speeds, segment=segment if full else None)
        assert np.array_equal(bits(raw), bits(np.tile(np.array([steer_bias, speed_bias], f32), (n, 1))))
        for name, cfg in STEP_RULE_CONFIGS.items():
            for masked in (True, False):
                ai = env.pilot_act_device(frames=d_frames, speed=d_speed, mode=d_mode if masked else None, cfg=dict(cfg, model_type=kind),
                                          segment=d_segment if full else None)
                steer, thr, brk = (env.to_host(a) for a in ai)
                for i in range(n):
                    case = (kind, float(steer_bias), name, masked, i)
                    w_steer, w_thr, w_brk, soft = want(steer_bias, i, cfg, int(modes[i]) if masked else 2)
                    print(case, "got", steer[i], thr[i], brk[i], "want", w_steer, w_thr, w_brk)
                    assert bits(steer[i]) == bits(w_steer), case
                    if masked and modes[i] not in (1, 2):
                        assert not bits([steer[i], thr[i], brk[i]]).any(), case                      # exactly (0, 0, 0)
                    elif capped:
                        assert bits(thr[i]) == bits(speed_bias) and bits(brk[i]) == 0, case
                    else:
                        exact_thr = cfg.get("spd_ctl_break") or w_thr == 0
                        assert (bits(thr[i]) == bits(w_thr)) if exact_thr else abs(float(thr[i]) - float(w_thr)) <= 1e-5, case
                        assert (bits(brk[i]) == 0) if w_brk == 0 else abs(float(brk[i]) - float(w_brk)) <= 1e-5, case
                        if cfg.get("spd_ctl_break"):
                            assert thr[i] in (0.0, 1.0), case
