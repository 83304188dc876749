"""trs_decode_jpeg on the GPU against the restatement of include/trsim_spec.h ("tub image (JPEG), decoding") in tests/test_jpeg_decode_cpu.py — which is
pinned to Pillow's decoder there — byte for byte: five sizes with every entropy path (stuffed 0xFF, ZRL, every AC size, DC + EOB only blocks, 1..7 pad
bits) and optimised tables, the encoder's slots decoded in place behind both step modes, files at odd offsets with more files than waves, frames that
start one byte past a dword boundary (the byte stores), every kind of bad file between good ones, the refusals, and the Python layer up to a tub read back.
Every device buffer of files ends in 4 KiB of sentinel bytes the test owns, and the frames lie between two sentinel frames."""
import numpy as np
import pytest

from conftest import track_points
from test_jpeg_cpu import encode
from test_jpeg_decode_cpu import CORRUPT, DECODED, SIZE_DIFFERS, SKIPPED, UNSUPPORTED, decode, golden_decode, status_cases
from test_jpeg_gpu import SENTINEL, SIZES, plain_env, ref

pytestmark = pytest.mark.gpu

TAIL = 4096
WAVES_PER_WG, WGS_PER_CU = 4, 2                 # include/trsim.h: min(ceil(n / 4), 2 x CU count) workgroups of 4 waves
_DECODED = {}


def want(data, h, w):
    """(frame, status, statistics) of the restatement, computed once per file and session"""
    key = (bytes(data), h, w)
    if key not in _DECODED:
        _DECODED[key] = decode(data, h, w)
    return _DECODED[key]


def pack(files, odd=False):
    """the files in one uint8 buffer (odd: each at an odd offset, with sentinel bytes between them) + TAIL sentinel bytes -> (blob, int64 offsets, int32 lengths)"""
    off, pos = [], 0
    for f in files:
        if odd:
            pos += 1 if pos % 2 == 0 else 2
        off.append(pos)
        pos += len(f)
    blob = np.full(pos + TAIL, SENTINEL, np.uint8)
    for o, f in zip(off, files):
        blob[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return blob, np.asarray(off, np.int64), np.asarray([len(f) for f in files], np.int32)


def device_decode(torch, env, blob, off, ln, expect_rc=0, misalign=0):
    """trs_decode_jpeg from device copies into sentinel-filled frames between two sentinel guard frames -> (uint8[n][H][W][3], int32 status[n]).
    misalign: the guard frames start that many bytes past a dword boundary (and so does every frame, where a frame's bytes are a multiple of 4)"""
    n = len(off)
    d_blob, d_off, d_len = (torch.as_tensor(a).cuda() for a in (blob, off, ln))
    flat = torch.full(((n + 2) * env.H * env.W * 3 + 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    lead = (misalign - flat.data_ptr()) % 4
    dst = flat[lead:lead + flat.numel() - 4].view(n + 2, env.H, env.W, 3)
    assert misalign == 0 or dst[1:].data_ptr() % 4 == misalign
    status = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()                        # the env works on its own stream
    env.device_decode_jpeg(d_blob, d_off, d_len, dst[1:], status[1:], n_images=n)
    env.sync()
    out, st = dst.cpu().numpy(), status.cpu().numpy()
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all(), "a guard frame was written"
    edge = flat.cpu().numpy()
    assert (edge[:lead] == SENTINEL).all() and (edge[lead + dst.numel():] == SENTINEL).all()
    assert st[0] == -7 and st[-1] == -7
    assert np.array_equal(d_blob.cpu().numpy(), blob)
    return out[1:-1], st[1:-1]


def assert_frames(frames, status, files, h, w, where):
    """decoded files carry the restatement's frame; frames of statuses 1..3 are untouched; the statuses are the restatement's (1 for an empty file)"""
    for i, data in enumerate(files):
        frame, st, _ = want(data, h, w) if len(data) else (None, SKIPPED, {})
        assert status[i] == st, f"{where}: file {i} has status {status[i]}, the restatement gives {st}"
        if st == DECODED:
            if not np.array_equal(frames[i], frame):
                bad = np.argwhere(frames[i] != frame)
                raise AssertionError(f"{where}: file {i}: {len(bad)} bytes differ, the first at (row, column, channel) {bad[0].tolist()}: "
                                     f"got {frames[i][tuple(bad[0])]}, want {frame[tuple(bad[0])]}")
        elif st != CORRUPT:
            assert (frames[i] == SENTINEL).all(), f"{where}: the frame of file {i} (status {st}) was written"


@pytest.mark.parametrize("h,w", SIZES)
def test_sizes_and_content(make_env, h, w):
    torch = pytest.importorskip("torch")
    env = plain_env(make_env, h, w)
    opt = golden_decode()[f"optfile_{h}x{w}"].tobytes()
    if (h, w) == (240, 320):                                         # three files of this size in the module: the restatement decodes serially
        items = [("rich", 100, 0), ("flat0", 75, 0)]
    else:
        pads, seed = {}, 0
        while len(pads) < 7 and seed < 400:
            p = ref("pad", h, w, 75, seed)[2]["pad_bits"]
            if p:
                pads.setdefault(p, seed)
            seed += 1
        items = ([("rich", 100, 0), ("checker", 100, 0), ("noise", 100, 0)] +
                 [("rich", 75, 0), ("noise", 75, 0), ("flat0", 75, 0), ("flat255", 75, 0), ("ramp", 75, 0)] + [("pad", 75, pads[p]) for p in sorted(pads)] +
                 [("noise", 10, 0), ("ramp", 10, 0)])
    files = [ref(kind, h, w, q, s)[1] for kind, q, s in items] + [opt]
    # what the inputs are claimed to hold, from the restatement, before anything is compared
    stats = [want(f, h, w)[2] for f in files]
    assert all(want(f, h, w)[1] == DECODED for f in files)
    rich = stats[0]
    assert rich["stuffed"] >= 1 and rich["zrl"] >= 1 and rich["ac_sizes"] == list(range(1, 11)), rich
    n_blocks = 6 * -(-h // 16) * -(-w // 16)
    assert stats[[i[0] for i in items].index("flat0")]["dc_eob_blocks"] == n_blocks
    if (h, w) != (240, 320):
        assert {s["pad_bits"] for s in stats} >= {1, 2, 3, 4, 5, 6, 7}
    from test_jpeg_decode_cpu import parse
    assert parse(opt)["ac"][0] != parse(files[0])["ac"][0], "the optimised file carries the standard's tables"
    frames, status = device_decode(torch, env, *pack(files))
    assert_frames(frames, status, files, h, w, f"{h}x{w}")
    assert (status == DECODED).all()


@pytest.mark.parametrize("resident", [False, True])
def test_device_round_trip(make_env, resident):
    """step, trs_encode_jpeg into slots, trs_decode_jpeg from those slots, nothing through the host: the frames are decode(encode(frame)), and Pillow's"""
    torch = pytest.importorskip("torch")
    n = 5
    env = make_env("hip", n_envs=n, auto_reset=True, track=track_points())
    if resident:
        env.set_step_mode(True, idle_us=300)
    env.step_synthetic(4, 1)
    rendered = env.fetch("img")
    files = [encode(f, 75) for f in rendered]
    sizes = sorted(len(f) for f in files)
    assert sizes[0] < sizes[-1]
    cap = sizes[-1] - 1                                              # the largest file does not fit its slot
    over = [len(f) > cap for f in files]
    slots = torch.full((n * cap + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    off = torch.arange(n, dtype=torch.int64, device="cuda") * cap
    dst = torch.full((n + 2, env.H, env.W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()
    env.device_encode_jpeg(slots, ln, quality=75, cap=cap)
    env.device_decode_jpeg(slots, off, ln, dst[1:], status)
    env.sync()
    out, st, lengths = dst.cpu().numpy(), status.cpu().numpy(), ln.cpu().numpy()
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all()
    assert (slots.cpu().numpy()[n * cap:] == SENTINEL).all()
    assert 1 <= sum(over) < n
    for i in range(n):
        if over[i]:
            assert lengths[i] == -len(files[i]) and st[i] == SKIPPED
            assert (out[1 + i] == SENTINEL).all(), "the frame of the overflowed slot was written"
            continue
        frame, s, _ = want(files[i], env.H, env.W)
        assert s == DECODED and st[i] == DECODED and lengths[i] == len(files[i])
        assert np.array_equal(out[1 + i], frame), f"env {i} resident={resident}"
        try:
            from test_jpeg_decode_cpu import pillow_decode
            assert np.array_equal(out[1 + i], pillow_decode(files[i]))
        except ImportError:
            pass
    assert np.array_equal(env.fetch("img"), rendered)                # neither call changed a frame of the env
    env.step_synthetic(1, 1)                                         # and the handle steps on
    assert not np.array_equal(env.fetch("img"), rendered)


def test_odd_offsets_and_more_files_than_waves(make_env):
    """files at odd byte offsets with odd lengths; n = 1, two files into frames one byte past a dword boundary (stored by bytes: the same frames as the
    aligned call's dword stores), and one more than twice the waves the library launches: every wave loops"""
    torch = pytest.importorskip("torch")
    h, w = 24, 40
    env = plain_env(make_env, h, w)
    kinds = [("rich", 0), ("noise", 0), ("ramp", 0), ("flat255", 0), ("noise", 1), ("checker", 0), ("rich", 1)]
    seven = [ref(k, h, w, 75, s)[1] for k, s in kinds]
    seven = [f if len(f) % 2 else f + b"\x00" for f in seven]        # (a byte behind EOI: the decoder stops at the last MCU)
    frames, status = device_decode(torch, env, *pack(seven[:1], odd=True))
    assert_frames(frames, status, seven[:1], h, w, "one file")
    aligned, status = device_decode(torch, env, *pack(seven[:2]))
    shifted, status1 = device_decode(torch, env, *pack(seven[:2]), misalign=1)
    assert (status == DECODED).all() and (status1 == DECODED).all() and np.array_equal(shifted, aligned)
    assert_frames(shifted, status1, seven[:2], h, w, "frames one byte past a dword boundary")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * WAVES_PER_WG * WGS_PER_CU * cus + 1
    order = np.arange(n) % len(seven)
    blob, off, ln = pack([seven[j] for j in order], odd=True)
    assert (off % 2 == 1).all() and (ln % 2 == 1).all()
    frames, status = device_decode(torch, env, blob, off, ln)
    assert (status == DECODED).all()
    for j, f in enumerate(seven):                                    # all frames that came from file j at once
        assert (frames[order == j] == want(f, h, w)[0]).all(), f"file kind {kinds[j]}"


def test_bad_files_among_good_ones(make_env):
    torch = pytest.importorskip("torch")
    h, w = 24, 40
    env = plain_env(make_env, h, w)
    good, cases = status_cases(h, w)
    other = ref("rich", h, w, 75)[1]
    files = [good]
    for k, (_, data, _) in enumerate(cases):
        files += [data, other if k % 2 else good]
    files += [b"", good]                                             # an empty file: skipped
    expect = [DECODED] + sum(([st, DECODED] for _, _, st in cases), []) + [SKIPPED, DECODED]
    assert sorted(set(expect)) == [DECODED, SKIPPED, UNSUPPORTED, SIZE_DIFFERS, CORRUPT]
    for odd in (False, True):
        blob, off, ln = pack(files, odd=odd)
        frames, status = device_decode(torch, env, blob, off, ln)
        assert status.tolist() == expect, [c[0] for c in cases]
        assert_frames(frames, status, files, h, w, f"bad files among good ones (odd offsets: {odd})")
    ln2 = ln.copy()
    ln2[0] = -len(good)                                              # the encoder's overflow report
    frames, status = device_decode(torch, env, blob, off, ln2)
    assert status[0] == SKIPPED and (frames[0] == SENTINEL).all() and status[1:].tolist() == expect[1:]


def test_refusals_leave_the_handle_stepping(make_env):
    torch = pytest.importorskip("torch")
    n = 4
    g, o = (make_env(kind, n_envs=n, auto_reset=True, track=track_points()) for kind in ("hip", "oracle"))
    for env in (g, o):
        env.step_synthetic(2, 1)
    data = encode(g.fetch("img")[0], 75)
    blob, off, ln = pack([data] * n)
    d_blob, d_off, d_len = (torch.as_tensor(a).cuda() for a in (blob, off, ln))
    dst = torch.full((n, g.H, g.W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()
    api, h = g.api, g._h
    ptr = [d_blob.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), dst.data_ptr(), status.data_ptr()]
    dec = lambda p, count: api.decode_jpeg(h, p[0], p[1], p[2], count, p[3], p[4])
    assert dec(ptr, 0) == -1 and dec(ptr, -3) == -1                  # TRS_ERR_ARG
    for k in range(5):
        assert dec(ptr[:k] + [None] + ptr[k + 1:], n) == -1, k
    hd, hs = np.full((n, g.H, g.W, 3), SENTINEL, np.uint8), np.full(n, -7, np.int32)
    assert api.decode_jpeg_host(h, blob.ctypes.data, off.ctypes.data, 0, hd.ctypes.data, hs.ctypes.data) == -1
    assert api.decode_jpeg_host(h, None, off.ctypes.data, n, hd.ctypes.data, hs.ctypes.data) == -1
    assert api.decode_jpeg_host(h, blob.ctypes.data, off.ctypes.data, n, None, hs.ctypes.data) == -1
    wide = plain_env(make_env, 16, 1024)                             # wider than a workgroup's LDS holds (include/trsim.h: img_w > 544 at 160 KiB)
    wdst = torch.full((1, 16, 1024, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    assert wide.api.decode_jpeg(wide._h, ptr[0], ptr[1], ptr[2], 1, wdst.data_ptr(), ptr[4]) == -5       # TRS_ERR_LIMIT
    assert b"img_w" in wide.api.last_error()
    g.sync()
    wide.sync()
    assert (dst.cpu().numpy() == SENTINEL).all() and (status.cpu().numpy() == -7).all() and (wdst.cpu().numpy() == SENTINEL).all()   # a refused call wrote nothing
    assert (hd == SENTINEL).all() and (hs == -7).all()
    assert dec(ptr, n) == 0, api.last_error()
    g.sync()
    assert (status.cpu().numpy() == DECODED).all() and (dst.cpu().numpy() == want(data, g.H, g.W)[0]).all()
    for env in (g, o):
        env.step_synthetic(3, 1)
        env.step(np.linspace(-1, 1, n, dtype=np.float32), 0.6, 0.0)
    for name in ("img", "seg_idx", "done", "ep_len"):
        assert np.array_equal(g.fetch(name), o.fetch(name)), name
    for name in ("pos_x", "pos_z", "speed", "cte"):
        assert np.max(np.abs(g.fetch(name) - o.fetch(name))) <= 1e-5, name


def test_python_layer_and_a_tub_read_back(make_env, tmp_path):
    pytest.importorskip("torch")
    from triton_racer_sim_amd.components import HipJpegDecoder, HipJpegEncoder
    from triton_racer_sim_amd.recorder import BatchedDataStorage, load_records
    try:
        import PIL  # noqa: F401
        have_pillow = True
    except ImportError:
        have_pillow = False
    n, ticks = 6, 4
    env = make_env("hip", n_envs=n, auto_reset=True, track=track_points())
    enc, dec = HipJpegEncoder(env), HipJpegDecoder(env)
    assert dec.step_inputs == ["cam/img_jpg"] and dec.step_outputs == ["cam/img"]
    fed = BatchedDataStorage(n, storage_root=str(tmp_path / "jpg"), image_port="cam/img_jpg")
    written = []
    for t in range(ticks):
        env.step_synthetic(1, 1)
        img, x, y, z, speed, cte, seg, _ = env.fetch_outputs()
        (jpg,) = enc.step(env.device_array("img"))
        written.append([jpg[i] for i in range(n)])
        fed.step(jpg, np.full(n, 0.3, np.float32), np.linspace(-1, 1, n).astype(np.float32), None, speed, seg / 100.0, x, y, z, cte, False, True)
        if t == ticks - 1:                                           # bytes and JpegFrames, the call and the component
            want_frames = np.stack([want(f, env.H, env.W)[0] for f in written[-1]])
            for files in (jpg, written[-1]):
                frames, status = env.decode_jpeg(files)
                assert (status == DECODED).all() and frames.dtype == np.uint8 and np.array_equal(frames, want_frames)
            assert np.array_equal(dec.step(jpg)[0], want_frames) and dec.step(None) == (None,)
    fed.onShutdown()
    tubs = [str(tmp_path / "jpg" / f"records_{i + 1}") for i in range(n)]
    imgs, feats, labels = load_records(tubs, env=env, batch=7)       # (7: the 18 images take three calls, the last one partial)
    assert imgs.shape == (n * (ticks - 1), env.H, env.W, 3) and imgs.dtype == np.float32
    if have_pillow:
        ref_imgs, ref_feats, ref_labels = load_records(tubs)
        assert np.array_equal(imgs, ref_imgs) and np.array_equal(feats, ref_feats) and np.array_equal(labels, ref_labels)
    else:
        frames = np.stack([want(written[k][i], env.H, env.W)[0] for i in range(n) for k in range(1, ticks)])     # (the loaders start at record 1)
        assert np.array_equal(imgs, frames.astype(np.float32) / np.float32(255))
    # what the device leaves to the host: Pillow decodes it where it imports, else the call names the file; another size always raises
    small = plain_env(make_env, 24, 40)
    good, cases = status_cases(24, 40)
    progressive = dict((c[0], c[1]) for c in cases)["progressive"]
    if have_pillow:
        from test_jpeg_decode_cpu import pillow_decode
        frames, status = small.decode_jpeg([good, progressive])
        assert status.tolist() == [DECODED, UNSUPPORTED] and np.array_equal(frames[1], pillow_decode(progressive)) and np.array_equal(frames[0], want(good, 24, 40)[0])
    else:
        with pytest.raises(RuntimeError, match="index 1"):
            small.decode_jpeg([good, progressive])
    with pytest.raises(RuntimeError, match="index 2"):
        small.decode_jpeg([good, good, dict((c[0], c[1]) for c in cases)["other size"]])
    with pytest.raises(RuntimeError, match="index 0"):
        small.decode_jpeg([good[:700], good])
