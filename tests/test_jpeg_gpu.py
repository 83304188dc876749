"""trs_encode_jpeg on the GPU against the numpy restatement of include/trsim_spec.h ("tub image (JPEG)") in tests/test_jpeg_cpu.py — which is pinned to
Pillow's files there — byte for byte: every edge rule (sizes with dummy blocks, replicated chroma rows, no padding at all), every entropy-coder path
(stuffed 0xFF, ZRL, every AC size, 1..7 pad bits, DC + EOB only), rendered frames behind every step path, more frames than workgroups, files that
overflow their slot, the refusals, and the Python recorder fed with the files."""
import json
import os

import numpy as np
import pytest

from conftest import track_points
from test_jpeg_cpu import HEADER_BYTES, encode, frame

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SIZES = [(24, 40), (50, 100), (60, 80), (120, 160), (240, 320)]
_REFS = {}


def rich_noise(h, w, seed=0):
    """noise whose 8 x 8 blocks cycle through amplitudes 1, 3, 10, 40, 127, binary +-127, black/white columns and a faint checkerboard: at quality 100
    it has stuffed bytes, ZRL codes and every AC size 1..10 in one frame (asserted where it is used)"""
    rng = np.random.default_rng(7000 * h + w + seed)
    amp = np.array([1, 3, 10, 40, 127, 127, 0, 0])
    yy, xx = np.mgrid[0:h, 0:w]
    k = (((yy // 8) * 5 + xx // 8) % 8)[..., None]
    s = rng.uniform(-1, 1, (h, w, 3))
    s = np.where(k == 5, np.sign(s), s)
    v = 128 + amp[k[..., 0]][..., None] * s
    v = np.where(k == 6, ((xx & 1) * 255)[..., None], v)
    v = np.where(k == 7, (128 + 2 * ((xx + yy) & 1))[..., None], v)
    return np.clip(v, 0, 255).astype(np.uint8)


def make(kind, h, w, seed=0):
    if kind == "rich":
        return rich_noise(h, w, seed)
    if kind == "pad":                                   # a ramp whose first block is noise: the seed moves the scan's bit count
        g = frame("ramp", h, w)
        g[:8, :8] = frame("noise", 8, 8, seed=seed)
        return g
    return frame(kind, h, w, seed)


def ref(kind, h, w, q, seed=0):
    """(frame, file, statistics) of the restatement, computed once per session"""
    key = (kind, h, w, q, seed)
    if key not in _REFS:
        img = make(kind, h, w, seed)
        _REFS[key] = (img,) + encode(img, q, with_stats=True)
    return _REFS[key]


def pillow_or_none(img, q):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return None
    from test_jpeg_cpu import pillow_bytes
    return pillow_bytes(img, q)


def device_encode(torch, env, frames, quality, cap, n_images=None):
    """trs_encode_jpeg from a device copy of `frames` (None: the latest frames) into sentinel-filled slots -> (uint8[n][cap], int32[n])"""
    n = env.n if frames is None else len(frames)
    n = n if n_images is None else n_images
    src = None if frames is None else torch.as_tensor(np.ascontiguousarray(frames)).cuda()
    dst = torch.full((n, cap), SENTINEL, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()                        # the env works on its own stream
    env.device_encode_jpeg(dst, ln, frames=src, n_images=n, quality=quality, cap=cap)
    env.sync()
    return dst.cpu().numpy(), ln.cpu().numpy()


def assert_slot(slot, length, want, where):
    """the slot holds the file `want`, its length is reported, and every byte behind the file is still the sentinel"""
    assert length == len(want), f"{where}: length {length}, the restatement's file has {len(want)} bytes"
    got = slot[:len(want)].tobytes()
    if got != want:
        d = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{where}: first difference at byte {d} of {len(want)} (header {HEADER_BYTES}): got {got[d:d + 8].hex()} want {want[d:d + 8].hex()}")
    assert (slot[len(want):] == SENTINEL).all(), f"{where}: bytes behind the file's end were written"


def plain_env(make_env, h, w):
    return make_env("hip", n_envs=1, track=None, render=False, img_h=h, img_w=w)


@pytest.mark.parametrize("h,w", SIZES)
def test_sizes_and_content(make_env, h, w):
    torch = pytest.importorskip("torch")
    env = plain_env(make_env, h, w)
    assert env.jpeg_header_bytes() == HEADER_BYTES
    # what the inputs are claimed to hold, from the restatement
    st = ref("rich", h, w, 100)[2]
    assert st["stuffed"] >= 1 and st["zrl"] >= 1 and st["ac_sizes"] == list(range(1, 11)), st
    assert ref("checker", h, w, 100)[2]["max_category"] >= 10
    assert ref("flat0", h, w, 75)[2]["only_dc_and_eob"] and ref("flat255", h, w, 75)[2]["only_dc_and_eob"]
    pads, seed = {}, 0
    while len(pads) < 7 and seed < 400:
        p = ref("pad", h, w, 75, seed)[2]["pad_bits"]
        if p:
            pads.setdefault(p, seed)
        seed += 1
    assert sorted(pads) == [1, 2, 3, 4, 5, 6, 7]
    groups = {100: [("rich", 0), ("checker", 0), ("noise", 0)],
              75: [("rich", 0), ("noise", 0), ("flat0", 0), ("flat255", 0), ("ramp", 0)] + [("pad", pads[p]) for p in sorted(pads)],
              10: [("noise", 0), ("ramp", 0)]}
    for q, items in groups.items():
        refs = [ref(kind, h, w, q, s) for kind, s in items]
        cap = max(len(r[1]) for r in refs) + 64
        slots, ln = device_encode(torch, env, np.stack([r[0] for r in refs]), q, cap)
        for i, (kind, s) in enumerate(items):
            assert_slot(slots[i], ln[i], refs[i][1], f"{h}x{w} quality {q} {kind} {s}")
    img, want, _ = ref("rich", h, w, 100)
    pil = pillow_or_none(img, 100)
    assert pil is None or pil == want


# (an observation latency and resident mode exclude each other, trs_set_latency: that case runs by launches only)
RENDER_CASES = [(c, r) for c in ("plain", "filter", "lighting", "mountain") for r in (False, True)] + [("latency", False)]


@pytest.mark.parametrize("case,resident", RENDER_CASES)
def test_rendered_frames(make_env, case, resident):
    """d_src NULL behind the step paths: the files are the restatement's (and Pillow's) for the frames trs_copy_to_host shows"""
    torch = pytest.importorskip("torch")
    n = 5
    env = make_env("hip", n_envs=n, auto_reset=True, track=track_points("mountain" if case == "mountain" else "generated"))
    if case == "filter":
        env.set_frame_filter({"preprocessing_color_filter_enabled": True, "preprocessing_contrast_enhancement_ratio": 1.3})
    if case == "lighting":
        from triton_racer_sim_amd.env import lighting_params
        env.set_lighting(lighting_params(n, seed=3))
    if case == "latency":
        env.set_latency([0, 1, 2, 3, 1])
    if resident:
        env.set_step_mode(True, idle_us=300)
    seen = set()
    for steps in (4, 1):                                             # the 5th step is the third into its frame buffer: its uniform rows were skipped twice
        env.step_synthetic(steps, 1)
        frames = env.fetch("img")
        want = [encode(f, 75) for f in frames]
        cap = env.jpeg_default_cap()
        assert max(len(x) for x in want) <= cap
        slots, ln = device_encode(torch, env, None, 75, cap)
        for i in range(n):
            assert_slot(slots[i], ln[i], want[i], f"{case} resident={resident} env {i}")
            pil = pillow_or_none(frames[i], 75)
            assert pil is None or pil == want[i]
        files = env.encode_jpeg()                                    # the host call: packed files, the same bytes
        assert len(files) == n and [files[i] for i in range(n)] == want
        assert files.offsets[-1] == sum(len(x) for x in want) == files.blob.size
        seen.update(want)
        assert np.array_equal(env.fetch("img"), frames)              # encoding changed no frame
    assert len(seen) > n


def test_one_frame_and_more_frames_than_workgroups(make_env):
    """n_images = 1, and one more than twice the workgroups the library launches (min(n_images, 4 x CU count), include/trsim.h): every workgroup loops"""
    torch = pytest.importorskip("torch")
    h, w = 24, 40
    env = plain_env(make_env, h, w)
    kinds = [("rich", 0), ("noise", 0), ("ramp", 0), ("flat255", 0), ("noise", 1), ("checker", 0), ("rich", 1)]
    refs = [ref(k, h, w, 75, s) for k, s in kinds]
    cap = max(len(r[1]) for r in refs) + 17                          # (an odd slot size: slots are not dword-aligned)
    slots, ln = device_encode(torch, env, refs[0][0][None], 75, cap)
    assert_slot(slots[0], ln[0], refs[0][1], "one frame")
    n = 2 * 4 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    order = np.arange(n) % len(refs)
    slots, ln = device_encode(torch, env, np.stack([r[0] for r in refs])[order], 75, cap)
    want_len = np.array([len(r[1]) for r in refs])[order]
    assert np.array_equal(ln, want_len)
    for j, r in enumerate(refs):                                     # all slots that hold frame j at once
        rows = slots[order == j]
        assert (rows[:, :len(r[1])] == np.frombuffer(r[1], np.uint8)).all(), f"frame kind {kinds[j]}"
        assert (rows[:, len(r[1]):] == SENTINEL).all()


def test_overflow_and_packed_files(make_env):
    torch = pytest.importorskip("torch")
    h, w, q = 50, 100, 75
    env = plain_env(make_env, h, w)
    smooth, noise = ref("ramp", h, w, q), ref("noise", h, w, q)
    assert len(smooth[1]) + 64 < len(noise[1])
    cap = (len(smooth[1]) + len(noise[1])) // 2
    n = 7
    frames = np.stack([(smooth, noise)[i & 1][0] for i in range(n)])
    slots, ln = device_encode(torch, env, frames, q, cap)
    for i in range(n):
        if i & 1:
            assert ln[i] == -len(noise[1]), "an overflowed slot reports the negated true length"
        else:
            assert_slot(slots[i], ln[i], smooth[1], f"fitting slot {i} beside overflowed neighbours")
    # the same batch through trs_encode_jpeg_host: packed files, offsets, lengths
    src = torch.as_tensor(frames).cuda()
    torch.cuda.current_stream().synchronize()
    total = len(smooth[1]) * ((n + 1) // 2)
    guard = 32
    blob = np.full(total + guard, SENTINEL, np.uint8)
    off, hl = np.full(n + 1, -1, np.int64), np.zeros(n, np.int32)
    call = lambda blob_cap: env.api.encode_jpeg_host(env._h, src.data_ptr(), n, q, cap, blob.ctypes.data, blob_cap, off.ctypes.data, hl.ctypes.data)
    assert call(total) == 0, env.api.last_error()
    assert np.array_equal(hl, ln)
    assert off[0] == 0 and off[-1] == total
    for i in range(n):
        if i & 1:
            assert off[i + 1] == off[i]
        else:
            assert blob[off[i]:off[i + 1]].tobytes() == smooth[1]
    assert (blob[total:] == SENTINEL).all()
    blob[:] = SENTINEL
    assert call(total - 1) == -5                                     # TRS_ERR_LIMIT
    assert b"blob_cap" in env.api.last_error()
    assert (blob[total - 1:] == SENTINEL).all() and off[-1] == total and np.array_equal(hl, ln)
    # Python: the overflowed frames come from Pillow on the host where it imports, else the call names the frame
    try:
        import PIL  # noqa: F401
        files = env.encode_jpeg(frames, quality=q, cap=cap)
        assert [files[i] for i in range(n)] == [(smooth, noise)[i & 1][1] for i in range(n)]
        assert (files.lengths[1::2] < 0).all()
    except ImportError:
        with pytest.raises(RuntimeError, match="env 1"):
            env.encode_jpeg(frames, quality=q, cap=cap)


def test_refusals_leave_the_handle_stepping(make_env):
    torch = pytest.importorskip("torch")
    n = 4
    g, o = (make_env(kind, n_envs=n, auto_reset=True, track=track_points()) for kind in ("hip", "oracle"))
    for env in (g, o):
        env.step_synthetic(2, 1)
    cap = g.jpeg_default_cap()
    dst = torch.full((n, cap), SENTINEL, dtype=torch.uint8, device="cuda")
    ln = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()
    api, h = g.api, g._h
    enc = lambda src, n_images, quality, c: api.encode_jpeg(h, src, n_images, quality, dst.data_ptr(), c, ln.data_ptr())
    assert enc(None, n, 0, cap) == -1 and enc(None, n, 101, cap) == -1                  # TRS_ERR_ARG
    assert enc(None, n, 75, HEADER_BYTES + 1) == -1
    assert enc(None, 0, 75, cap) == -1 and enc(None, -3, 75, cap) == -1
    assert enc(None, n - 1, 75, cap) == -1                                               # the latest frames are n_envs frames
    assert api.jpeg_header_bytes(h, 0) == -1 and api.jpeg_header_bytes(h, 75) == HEADER_BYTES
    off = np.zeros(n + 1, np.int64)
    blob = np.zeros(16, np.uint8)
    assert api.encode_jpeg_host(h, None, n, 75, HEADER_BYTES + 1, blob.ctypes.data, blob.nbytes, off.ctypes.data, None) == -1
    blind = make_env("hip", n_envs=n, track=track_points(), render=False)
    blind.step_synthetic(1, 1)
    assert blind.api.encode_jpeg(blind._h, None, n, 75, dst.data_ptr(), cap, ln.data_ptr()) == -2    # TRS_ERR_STATE: no camera
    assert b"camera" in blind.api.last_error()
    g.sync()
    assert (dst.cpu().numpy() == SENTINEL).all() and (ln.cpu().numpy() == 12345).all()  # a refused call wrote nothing
    assert enc(None, n, 75, HEADER_BYTES + 2) == 0                                       # the smallest slot: every file overflows, nothing beyond the slots
    g.sync()
    want = [encode(f, 75) for f in o.fetch("img")]
    assert ln.cpu().numpy().tolist() == [-len(x) for x in want]
    assert (dst.cpu().numpy().reshape(-1)[n * (HEADER_BYTES + 2):] == SENTINEL).all()
    for env in (g, o):
        env.step_synthetic(3, 1)
        env.step(np.linspace(-1, 1, n, dtype=np.float32), 0.6, 0.0)
    for name in ("img", "seg_idx", "done", "ep_len"):
        assert np.array_equal(g.fetch(name), o.fetch(name)), name
    for name in ("pos_x", "pos_z", "speed", "cte"):
        assert np.max(np.abs(g.fetch(name) - o.fetch(name))) <= 1e-5, name


def test_tubs_fed_with_device_encoded_files(make_env, tmp_path):
    """BatchedDataStorage fed by HipJpegEncoder writes the tubs the array-fed recorder writes: the same JSON byte for byte, the same img_k.jpg"""
    pytest.importorskip("torch")
    from triton_racer_sim_amd.components import HipJpegEncoder
    from triton_racer_sim_amd.recorder import BatchedDataStorage, load_records
    try:
        import PIL  # noqa: F401
        have_pillow = True
    except ImportError:
        have_pillow = False
    n, ticks = 6, 4
    env = make_env("hip", n_envs=n, auto_reset=True, track=track_points())
    enc = HipJpegEncoder(env)
    assert enc.step_inputs == ["cam/img"] and enc.step_outputs == ["cam/img_jpg"]
    fed = BatchedDataStorage(n, storage_root=str(tmp_path / "jpg"), image_port="cam/img_jpg")
    assert fed.step_inputs[0] == "cam/img_jpg"
    plain = BatchedDataStorage(n, storage_root=str(tmp_path / "arr")) if have_pillow else None
    frames = []
    for t in range(ticks):
        env.step_synthetic(1, 1)
        img, x, y, z, speed, cte, seg, _ = env.fetch_outputs()
        frames.append(img)
        (jpg,) = enc.step(env.device_array("img"))
        rest = (np.full(n, 0.3, np.float32), np.linspace(-1, 1, n).astype(np.float32), None, speed, seg / 100.0, x, y, z, cte, False, True)
        fed.step(jpg, *rest)
        if plain is not None:
            plain.step(img, *rest)
    fed.onShutdown()
    if plain is not None:
        plain.onShutdown()
    for i in range(n):
        tub = tmp_path / "jpg" / f"records_{i + 1}"
        for k in range(ticks):
            data = (tub / f"img_{k}.jpg").read_bytes()
            assert data == encode(frames[k][i], 75), (i, k)
            record = (tub / f"record_{k}.json").read_bytes()
            assert json.loads(record)["cam/img"] == f"img_{k}.jpg"
            if plain is not None:
                other = tmp_path / "arr" / f"records_{i + 1}"
                assert record == (other / f"record_{k}.json").read_bytes(), (i, k)
                assert data == (other / f"img_{k}.jpg").read_bytes(), (i, k)
        assert sorted(os.listdir(tub)) == sorted(f"{kind}_{k}.{ext}" for k in range(ticks) for kind, ext in (("img", "jpg"), ("record", "json")))
    if have_pillow:
        imgs, _, labels = load_records([str(tmp_path / "jpg" / f"records_{i + 1}") for i in range(n)])
        assert imgs.shape == (n * (ticks - 1), env.H, env.W, 3) and labels.shape == (n * (ticks - 1), 2)      # (the loaders start at record 1)
