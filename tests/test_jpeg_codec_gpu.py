"""trs_jpeg_roundtrip and trs_set_camera_codec on the GPU against the restatement of include/trsim_spec.h ("camera codec (JPEG round trip)") in
tests/test_jpeg_codec_cpu.py — which is pinned to decode(encode()) and to Pillow's save and open there — byte for byte: every edge rule (one MCU, a dummy
block row and column, replicated rows with an odd chroma height, half an MCU row at the bottom, 240 x 320), every content at three qualities, the device
composition trs_decode_jpeg(trs_encode_jpeg()) behind both step modes, one frame and more frames than workgroups, the closed pilot loop against its manual
composition with and without a latency, the refusals, and the gym interfaces' img_jpeg_quality.
The frames are the test's own device copies; the results lie between two sentinel guard frames, and the source is compared with what was uploaded."""
import ctypes

import numpy as np
import pytest

from conftest import track_points
from test_jpeg_codec_cpu import roundtrip
from test_jpeg_gpu import SENTINEL, make, plain_env
from test_latency_gpu import STATE, bits, dev_np

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (24, 40), (50, 100), (120, 160), (240, 320)]
KINDS = ["rich", "noise", "checker", "flat0", "flat255", "ramp"]
WGS_PER_CU = 4                                  # include/trsim.h: min(n_images, 4 x CU count) workgroups
_WANT = {}


def want(kind, h, w, q, seed=0):
    """(frame, codec(frame, q)) of the restatement, computed once per session"""
    key = (kind, h, w, q, seed)
    if key not in _WANT:
        img = make(kind, h, w, seed)
        _WANT[key] = (img, roundtrip(img, q))
    return _WANT[key]


def device_roundtrip(torch, env, frames, quality):
    """trs_jpeg_roundtrip from a device copy of `frames` into sentinel-filled frames between two sentinel guard frames -> uint8[n][H][W][3]"""
    n = len(frames)
    host = np.ascontiguousarray(frames)
    src = torch.as_tensor(host).cuda()
    dst = torch.full((n + 2, env.H, env.W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()                        # the env works on its own stream
    env.device_jpeg_roundtrip(src, quality, d_dst=dst[1:], n_images=n)
    env.sync()
    out = dst.cpu().numpy()
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all(), "a guard frame was written"
    assert np.array_equal(src.cpu().numpy(), host), "the source was written"
    return out[1:-1]


def assert_frame(got, ref, where):
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"{where}: {len(bad)} bytes differ, the first at (row, column, channel) {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {ref[tuple(bad[0])]}")


@pytest.mark.parametrize("h,w", SIZES)
def test_bytes(make_env, h, w):
    torch = pytest.importorskip("torch")
    env = plain_env(make_env, h, w)
    for q in (75, 100, 10):
        refs = [want(kind, h, w, q) for kind in KINDS]
        got = device_roundtrip(torch, env, np.stack([r[0] for r in refs]), q)
        for i, kind in enumerate(KINDS):
            assert_frame(got[i], refs[i][1], f"{h}x{w} quality {q} {kind}")
    # the comparison has something to show: the hard frames come back changed, and differently at each quality
    assert not np.array_equal(want("checker", h, w, 75)[1], want("checker", h, w, 75)[0])
    assert not np.array_equal(want("noise", h, w, 75)[1], want("noise", h, w, 10)[1])


@pytest.mark.parametrize("resident", [False, True])
def test_composition_on_the_device(make_env, resident):
    """rendered frames after a few steps: trs_jpeg_roundtrip(latest frames) == trs_decode_jpeg(trs_encode_jpeg(latest frames)), nothing through the host"""
    torch = pytest.importorskip("torch")
    n = 5
    env = make_env("hip", n_envs=n, auto_reset=True, track=track_points())
    if resident:
        env.set_step_mode(True, idle_us=300)
    env.step_synthetic(4, 1)
    rendered = env.fetch("img")
    cap = env.jpeg_header_bytes() + 2 + env.H * env.W * 3
    slots = torch.zeros((n * cap,), dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    off = torch.arange(n, dtype=torch.int64, device="cuda") * cap
    two = torch.full((n, env.H, env.W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    one = torch.full((n + 2, env.H, env.W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    env.device_encode_jpeg(slots, ln, quality=75, cap=cap)
    env.device_decode_jpeg(slots, off, ln, two, status)
    env.device_jpeg_roundtrip(None, 75, d_dst=one[1:])
    own = env.device_jpeg_roundtrip(None, 75)                        # ... and into the handle's own buffer
    env.sync()
    assert (status.cpu().numpy() == 0).all()
    got, ref = one.cpu().numpy(), two.cpu().numpy()
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all()
    for i in range(n):
        assert_frame(got[1 + i], ref[i], f"env {i} resident={resident}")
        assert_frame(got[1 + i], roundtrip(rendered[i], 75), f"env {i} against the restatement")
    assert np.array_equal(dev_np(own), ref)
    assert not np.array_equal(ref, rendered)                         # rendered frames are where a 4:2:0 quality-75 file differs
    assert np.array_equal(env.fetch("img"), rendered)                # no call changed a frame of the env
    assert np.array_equal(env.jpeg_roundtrip(None, 75), ref) and np.array_equal(env.jpeg_roundtrip(rendered, 75), ref)   # the host entry point, both sources
    env.step_synthetic(1, 1)                                         # and the handle steps on
    assert not np.array_equal(env.fetch("img"), rendered)


def test_one_frame_and_more_frames_than_workgroups(make_env):
    torch = pytest.importorskip("torch")
    h, w = 24, 40
    env = plain_env(make_env, h, w)
    kinds = [("rich", 0), ("noise", 0), ("ramp", 0), ("flat255", 0), ("noise", 1), ("checker", 0), ("rich", 1)]
    seven = [want(k, h, w, 75, s) for k, s in kinds]
    assert_frame(device_roundtrip(torch, env, seven[0][0][None], 75)[0], seven[0][1], "one frame")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = WGS_PER_CU * cus
    n = 2 * grid + 3                                                 # every workgroup loops, some of them three times
    order = np.arange(n) % len(seven)
    assert n > grid and len(set(order[i] for i in range(0, n, grid))) > 1      # a workgroup's frames differ from each other
    got = device_roundtrip(torch, env, np.stack([seven[j][0] for j in order]), 75)
    for j, (kind, ref) in enumerate(zip(kinds, seven)):
        assert (got[order == j] == ref[1]).all(), f"frames of kind {kind}"


def trained_env(make_env, n):
    from test_pilot_trained import H, W, trained_weights
    env = make_env("hip", n_envs=n, img_h=H, img_w=W, auto_reset=True)
    env.pilot_load(trained_weights())
    return env


def assert_same_state(a, b, where, skip=()):
    for k in STATE + ("vel",):
        if k not in skip:
            assert np.array_equal(bits(a.fetch(k)), bits(b.fetch(k))), (where, k)
    assert np.array_equal(a.fetch("img"), b.fetch("img")), (where, "img")


CTL = ("ctl_steer", "ctl_thr", "ctl_brk")


def test_closed_loop_equals_the_manual_composition(make_env):
    """trs_step_pilot with a codec set against device_jpeg_roundtrip -> pilot_act_device -> step_device on a twin: controls, state and frames bit for bit;
    a third handle without a codec drives differently, and the truth frames of all three stay the rasteriser's"""
    torch = pytest.importorskip("torch")
    from triton_racer_sim_amd.env import device_ptr
    n = 16
    a, b, c = (trained_env(make_env, n) for _ in range(3))
    a.set_camera_codec(75)
    assert a.camera_codec() == 75 and b.camera_codec() == 0
    differs = False
    for T in range(1, 7):
        a.step_pilot(1)
        c.step_pilot(1)
        if T == 1:                                                   # no frame yet: (0, 0, 0) (keras_pilot.py:46-47)
            b.step(0.0, 0.0, 0.0)
            assert all(not a.fetch(k).any() for k in CTL)
        else:
            seen = b.device_jpeg_roundtrip(None, 75)
            ai = b.pilot_act_device(frames=seen)
            b.step_device(device_ptr(ai[0]), device_ptr(ai[1]), device_ptr(ai[2]))
            b.sync()                                                 # (dev_np reads on another stream)
            for k, y in zip(CTL, ai):
                assert np.array_equal(bits(a.fetch(k)), bits(dev_np(y))), (T, k)
            differs = differs or any(np.any(a.fetch(k) != c.fetch(k)) for k in CTL)
        assert_same_state(a, b, f"tick {T}")
    assert differs, "the pilot's controls with the codec equal those without: the comparison shows nothing"
    # (the twin never set a codec: the frames compared above are the rasteriser's, so the truth stayed the truth); the codec buffer holds the restatement's frame
    own = a.device_jpeg_roundtrip(None, 75)
    a.sync()
    assert_frame(dev_np(own)[3], roundtrip(a.fetch("img")[3], 75), "the handle's codec buffer, env 3")


def test_closed_loop_under_a_latency_reads_the_delayed_frame(make_env):
    torch = pytest.importorskip("torch")
    from triton_racer_sim_amd.env import device_ptr
    n, L = 16, 2
    a, b = (trained_env(make_env, n) for _ in range(2))
    for env in (a, b):
        env.set_latency(L)
    a.set_camera_codec(75)
    for T in range(1, 7):
        a.step_pilot(1)
        arrived = torch.as_tensor(b.device_observation("arrived"), device="cuda")
        mode = torch.where(arrived != 0, 2, 0).to(torch.uint8)                    # AI where the observation has arrived, else HUMAN
        torch.cuda.synchronize()
        seen = b.device_jpeg_roundtrip(b.device_observation("img"), 75)
        ai = b.pilot_act_device(frames=seen, speed=b.device_observation("speed"), mode=mode)
        b.step_device(device_ptr(ai[0]), device_ptr(ai[1]), device_ptr(ai[2]))
        b.sync()                                                     # (dev_np reads on another stream)
        for k, y in zip(CTL, ai):
            assert np.array_equal(bits(a.fetch(k)), bits(dev_np(y))), (T, k)
        assert_same_state(a, b, f"tick {T}")
        waiting = (T - 1) - L < 1
        assert all(bool(a.fetch(k).any()) != waiting for k in CTL[:2]), T
        assert np.array_equal(a.observation()[0], b.observation()[0]), T          # the observation stays the truth of L ticks ago, not the codec's frame


def test_codec_off_again_drives_like_a_handle_that_never_set_it(make_env):
    pytest.importorskip("torch")
    n = 16
    a, c = (trained_env(make_env, n) for _ in range(2))
    a.set_camera_codec(75)
    a.step_pilot(4)
    c.step_pilot(4)
    assert any(np.any(a.fetch(k) != c.fetch(k)) for k in CTL)
    a.set_camera_codec(0)
    assert a.camera_codec() == 0
    for env in (a, c):                                               # the same state again: every env on its start pose, and a frame of it
        env.reset()
        env.step(0.0, 0.0, 0.0)
    for T in range(1, 4):
        a.step_pilot(1)
        c.step_pilot(1)
        for k in CTL:
            assert np.array_equal(bits(a.fetch(k)), bits(c.fetch(k))), (T, k)
        assert_same_state(a, c, f"tick {T} after the codec was turned off", skip=("last_return",))
    assert any(a.fetch(k).any() for k in CTL)


def test_refusals_leave_the_handle_stepping_like_its_twin(make_env):
    torch = pytest.importorskip("torch")
    n = 4
    pts = track_points()
    g, t = (make_env("hip", n_envs=n, auto_reset=True, track=pts) for _ in range(2))
    api, h = g.api, g._h

    def steps_like_twin(where):
        g.step_synthetic(2, 1); t.step_synthetic(2, 1)
        assert_same_state(g, t, where)

    steps_like_twin("before")
    buf = torch.full((2 * n + 1, g.H, g.W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    fb = g.H * g.W * 3
    src, dst = buf.data_ptr(), buf.data_ptr() + n * fb
    out = ctypes.c_void_p()
    rt = lambda s, count, q, d: api.jpeg_roundtrip(h, s, count, q, d, ctypes.byref(out))
    for q in (0, 101, -5):
        assert rt(src, n, q, dst) == -1, q                           # TRS_ERR_ARG
        assert rt(None, n, q, None) == -1, q
    assert rt(src, 0, 75, dst) == -1 and rt(None, n - 1, 75, dst) == -1 and rt(src, n + 1, 75, None) == -1
    assert rt(src, n, 75, src) == -1 and b"overlaps" in api.last_error()           # in place
    assert rt(src, n, 75, src + fb) == -1 and rt(src + fb, n, 75, src) == -1       # shifted by one frame, either way
    assert rt(src + 2, n, 75, dst) == -1 and rt(src, n, 75, dst + 2) == -1         # not dword-aligned
    hd = np.full((n, g.H, g.W, 3), SENTINEL, np.uint8)
    assert api.jpeg_roundtrip_host(h, None, n, 0, hd.ctypes.data) == -1 and api.jpeg_roundtrip_host(h, None, n, 75, None) == -1
    g.sync()
    assert (buf.cpu().numpy() == SENTINEL).all() and (hd == SENTINEL).all()        # a refused call wrote nothing
    steps_like_twin("after refused round trips")
    for q in (-1, 101):
        assert api.set_camera_codec(h, q) == -1 and g.camera_codec() == 0
    blind = plain_env(make_env, 24, 40)                              # no camera: no latest frame, and nothing a codec could be set on
    assert blind.api.jpeg_roundtrip(blind._h, None, 1, 75, None, ctypes.byref(out)) == -2      # TRS_ERR_STATE
    assert blind.api.set_camera_codec(blind._h, 75) == -2 and blind.camera_codec() == 0
    wide = plain_env(make_env, 16, 1216)                             # beyond the plan's width limit (include/trsim.h: img_w > 1200 at 160 KiB)
    wbuf = torch.full((2, 16, 1216, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    assert wide.api.jpeg_roundtrip(wide._h, wbuf.data_ptr(), 1, 75, wbuf.data_ptr() + 16 * 1216 * 3, ctypes.byref(out)) == -5     # TRS_ERR_LIMIT
    assert b"img_w <= 1200" in wide.api.last_error()
    wide.sync()
    assert (wbuf.cpu().numpy() == SENTINEL).all()
    # a codec and a fused frame filter exclude each other, in either order; the refused call changes nothing
    cfg = {"preprocessing_color_filter_enabled": True, "preprocessing_contrast_enhancement_ratio": 1.2}
    g.set_frame_filter(cfg); t.set_frame_filter(cfg)
    assert api.set_camera_codec(h, 75) == -2 and b"frame filter" in api.last_error() and g.camera_codec() == 0
    steps_like_twin("filter set, codec refused")
    g.set_frame_filter(enabled=False); t.set_frame_filter(enabled=False)
    steps_like_twin("filter off")
    raw = g.fetch("img")
    g.set_camera_codec(75)
    pc = g.pre_config(cfg)
    assert api.set_frame_filter(h, ctypes.byref(pc)) == -2 and b"camera codec" in api.last_error() and g.camera_codec() == 75
    assert api.set_camera_codec(h, 101) == -1 and g.camera_codec() == 75
    g.set_frame_filter(enabled=False)                                # removing a filter that is not there is no refusal
    steps_like_twin("codec set, filter refused")                     # (a codec changes nothing a step without a pilot shows)
    assert not np.array_equal(g.fetch("img"), raw)
    assert rt(src, n, 75, dst) == 0, api.last_error()                # and the round trip works after all of it
    g.sync()
    assert np.array_equal(buf[n:2 * n].cpu().numpy(), roundtrip(np.full((g.H, g.W, 3), SENTINEL, np.uint8), 75)[None].repeat(n, 0))
    assert (buf[2 * n].cpu().numpy() == SENTINEL).all()


def test_gym_interfaces_honour_img_jpeg_quality(make_env):
    pytest.importorskip("torch")
    from triton_racer_sim_amd.components import BatchedGymInterface, HipGymInterface
    n = 3
    coded = BatchedGymInterface(n, gym_config={"img_jpeg_quality": 75}, to_host=True)
    plain = BatchedGymInterface(n, to_host=True)
    dev = BatchedGymInterface(n, gym_config={"img_jpeg_quality": "75"})
    late = BatchedGymInterface(n, gym_config={"img_jpeg_quality": 75, "sim_latency": 100}, to_host=True)
    one = HipGymInterface(gym_config={"img_jpeg_quality": 75})
    o = make_env("oracle", n_envs=n, auto_reset=True)
    try:
        assert coded.jpeg_quality == 75 and plain.jpeg_quality == 0 and late.latency_ticks.tolist() == [2] * n
        rng = np.random.default_rng(3)
        truth = []
        for T in range(1, 6):
            st, th = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(0.6, 1, n).astype(np.float32)
            o.step(st, th)
            truth.append(o.fetch("img"))
            got, ref = coded.step(st, th, None, None), plain.step(st, th, None, None)
            assert np.array_equal(ref[0], truth[-1]), T              # without the key: unchanged
            for i in range(n):
                assert_frame(got[0][i], roundtrip(truth[-1][i], 75), f"tick {T} env {i}")
            for x, y in zip(got[1:], ref[1:]):
                assert np.array_equal(bits(x), bits(y)), T
            assert np.array_equal(coded.env.fetch("img"), truth[-1]), T          # the env's own frame stays the truth
            assert np.array_equal(dev_np(dev.step(st, th, None, None)[0]), got[0]), T
            img = late.step(st, th, None, None)[0]                   # sim_latency of 2 ticks: the codec's frame of the delayed one (zeros before it arrives)
            told = truth[T - 3] if T >= 3 else np.zeros_like(truth[-1])
            for i in range(n):
                assert_frame(img[i], roundtrip(told[i], 75), f"tick {T} env {i}, 2 ticks late")
            single = one.step(float(st[0]), float(th[0]), 0.0, False)
            assert_frame(single[0], got[0][0], f"HipGymInterface tick {T}")
        with pytest.raises(ValueError):
            BatchedGymInterface(1, gym_config={"img_jpeg_quality": 101})
    finally:
        for part in (coded, plain, dev, late, one):
            part.onShutdown()

