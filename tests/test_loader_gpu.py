"""The training minibatches on the GPU (trs_sample_batch; include/trsim_spec.h, "training minibatches") against the numpy restatement of
tests/test_loader_cpu.py, bit for bit: every layout and type, every loader and label, frames whose starts are only 4-byte aligned, windows that start
mid-epoch and end with the split, a batch with more work items than the grid has workgroups; canaries around every output; the refusals; and the Python
layer end to end (collect -> dataset -> batches -> pilot_loss).  Device buffers are filled directly: only trs_sample_batch is under test up to there."""
import ctypes

import numpy as np
import pytest

from test_loader_cpu import DTYPES, F, LABELS, LAYOUTS, LOADERS, N_FEATURES, features_labels, images_of, n_train_of, order

pytestmark = pytest.mark.gpu

CANARY = 0xA5
COMBOS = [("nhwc", "float32"), ("nhwc", "float16"), ("nhwc", "uint8"), ("nchw", "float32"), ("nchw", "float16")]
RULES = [(lo, la) for lo in LOADERS for la in LABELS]
NP_DTYPES = {"float32": np.float32, "float16": np.float16, "uint8": np.uint8}
SEED = 0xC0FFEE


def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


class Canaried:
    """`payload` bytes of device memory between two guards of `guard` bytes, everything filled with the canary byte; the payload starts 256-byte aligned."""

    def __init__(self, payload, guard):
        torch, dev = torch_dev()
        self.guard = (int(guard) + 255) // 256 * 256
        self.payload = int(payload)
        self.t = torch.full((2 * self.guard + self.payload,), CANARY, dtype=torch.uint8, device=dev)
        self.ptr = self.t.data_ptr() + self.guard
        assert self.ptr % 256 == 0
        torch.cuda.current_stream(dev).synchronize()                 # the fill is torch's; the gather runs on the env's stream, which does not wait for it

    def host(self):
        a = self.t.cpu().numpy()
        return a[:self.guard], a[self.guard:self.guard + self.payload], a[self.guard + self.payload:]

    def untouched(self):
        return bool((self.t == CANARY).all().item())


def make_set(n, H, W, seed=1):
    """n records: the first frame a byte ramp, the rest random; rows with negative speeds, 0 and 13.7."""
    rng = np.random.default_rng(seed + 1000 * n + H * W)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    frames[0] = (np.arange(H * W * 3) % 256).astype(np.uint8).reshape(H, W, 3)
    rows = rng.uniform(-1, 1, (n, 8)).astype(F)
    rows[:, 4] = rng.uniform(-5, 25, n).astype(F)
    rows[:min(n, 3), 4] = np.array([0.0, 13.7, -2.3], F)[:min(n, 3)]
    rows[:, 6] = (rng.integers(0, 1185, n) / 1185 * 10).astype(F)
    return frames, rows


def loader_config(api, n, nt, loader, label, layout, dtype, seed=SEED):
    from triton_racer_sim_amd import _ffi
    c = _ffi.TrsLoaderConfig()
    api.default_loader_config(ctypes.byref(c))
    c.loader, c.label, c.layout, c.dtype = LOADERS[loader], LABELS[label], LAYOUTS[layout], DTYPES[dtype]
    c.n_records, c.n_train, c.seed = n, nt, seed
    return c


class Outputs:
    """Canaried output buffers for `slots` batch slots of H x W frames."""

    def __init__(self, slots, H, W, dtype, n_feat):
        self.frame_out = H * W * 3 * np.dtype(NP_DTYPES[dtype]).itemsize
        self.n_feat = n_feat
        self.images = Canaried(slots * self.frame_out, self.frame_out)
        self.features = Canaried(slots * max(n_feat, 1) * 4, 256)
        self.labels = Canaried(slots * 2 * 4, 256)
        self.index = Canaried(slots * 4, 256)

    def all(self):
        return self.images, self.features, self.labels, self.index

    def untouched(self):
        return all(b.untouched() for b in self.all())


def check_batch(env, d_frames, d_rows, frames, rows, n, nt, split, epoch, first, batch, layout, dtype, loader, label, extra=2):
    H, W = env.H, env.W
    cfg = loader_config(env.api, n, nt, loader, label, layout, dtype)
    nf = N_FEATURES[loader]
    out = Outputs(batch + extra, H, W, dtype, nf)
    rc = env.api.sample_batch(env._h, ctypes.byref(cfg), d_frames.data_ptr(), d_rows.data_ptr(), split, epoch, first, batch,
                              out.images.ptr, out.features.ptr, out.labels.ptr, out.index.ptr)
    assert rc == 0, env.api.last_error()
    env.sync()
    what = (H, W, n, nt, split, epoch, first, batch, layout, dtype, loader, label)
    idx = order(SEED, n, nt, split, epoch, first, batch)
    want_img = images_of(frames[idx], layout, dtype)
    want_feat, want_lab = features_labels(rows[idx], loader, label)
    for buf, want in ((out.images, want_img), (out.features, want_feat), (out.labels, want_lab), (out.index, idx.astype(np.int32))):
        pre, got, post = buf.host()
        want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert np.array_equal(got[:want.size], want), what                            # bit for bit
        assert np.all(got[want.size:] == CANARY), what                                # slots beyond `batch`
        assert np.all(pre == CANARY) and np.all(post == CANARY), what                 # a frame (images) / 256 bytes either side
    return idx


def windows(n_s, batch):
    """`first` values for a batch: one that ends exactly at the split's end, one that starts mid-epoch, the start."""
    return sorted({n_s - batch, (n_s - batch) // 2, 0})


@pytest.fixture()
def upload():
    torch, dev = torch_dev()

    def _up(frames, rows):
        d = torch.as_tensor(frames).to(dev), torch.as_tensor(rows).to(dev)
        torch.cuda.current_stream(dev).synchronize()                 # as for the canaries: the env's stream does not wait for torch's
        return d
    return _up


# ---- bit-exact against the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(3, 4), (5, 12), (33, 8), (2, 2048), (120, 160)])
def test_batches_equal_the_restatement(make_env, upload, H, W):
    """3 x 4: 36-byte frames, so record r starts at a multiple of 4 and no more; 33 x 8 and 5 x 12: a partial last wave; 2 x 2048: exactly one NCHW item and
    three NHWC items per slot; 120 x 160: 15 and 5 items per slot, the last one partial."""
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    case = 0
    for n in (1, 5, 37, 300):
        frames, rows = make_set(n, H, W)
        d_frames, d_rows = upload(frames, rows)
        nt = n_train_of(0.8, n)
        for split in (0, 1):
            n_s = nt if split == 0 else n - nt
            for batch in (1, 7, 64):
                if batch > n_s:
                    continue
                for first in windows(n_s, batch):
                    # every layout x type at every window, the loaders and labels rotating through them ...
                    for layout, dtype in COMBOS:
                        loader, label = RULES[case % len(RULES)]
                        case += 1
                        check_batch(env, d_frames, d_rows, frames, rows, n, nt, split, 1 + case % 3, first, batch, layout, dtype, loader, label)
    # ... and every loader x label with every layout x type at one window
    n, nt = 37, n_train_of(0.8, 37)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    for loader, label in RULES:
        for layout, dtype in COMBOS:
            check_batch(env, d_frames, d_rows, frames, rows, n, nt, 0, 2, nt - 7, 7, layout, dtype, loader, label)
    assert case >= 5 * 14


@pytest.mark.parametrize("layout,dtype", [("nhwc", "float32"), ("nchw", "float16")])
def test_more_items_than_workgroups(make_env, upload, layout, dtype):
    """300 slots of 120 x 160 frames are 4500 NHWC work items, more than the 16 x CU count = 4096 workgroups of the grid: workgroups stride over items.  (The
    same batch as NCHW has 1500 items, one per workgroup: the largest grid the other layout's kernel gets in this suite.)"""
    env = make_env("hip", n_envs=1, track=None)
    frames, rows = make_set(300, 120, 160)
    d_frames, d_rows = upload(frames, rows)
    check_batch(env, d_frames, d_rows, frames, rows, 300, 300, 0, 1, 0, 300, layout, dtype, "full_house", "applied", extra=1)


def test_a_physics_only_set_has_rows_alone(make_env, upload):
    env = make_env("hip", n_envs=1, track=None, render=False)
    n, nt = 37, 29
    _, rows = make_set(n, 2, 4)
    torch, dev = torch_dev()
    d_rows = torch.as_tensor(rows).to(dev)
    cfg = loader_config(env.api, n, nt, "full_house", "applied", "nchw", "float32")
    out = Outputs(9, 2, 4, "float32", 2)
    assert env.api.sample_batch(env._h, ctypes.byref(cfg), None, d_rows.data_ptr(), 0, 4, 22, 7, None, out.features.ptr, out.labels.ptr, out.index.ptr) == 0
    env.sync()
    idx = order(SEED, n, nt, 0, 4, 22, 7)
    feat, lab = features_labels(rows[idx], "full_house", "applied")
    assert out.images.untouched()
    for buf, want in ((out.features, feat), (out.labels, lab), (out.index, idx.astype(np.int32))):
        pre, got, post = buf.host()
        want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert np.array_equal(got[:want.size], want) and np.all(got[want.size:] == CANARY) and np.all(pre == CANARY) and np.all(post == CANARY)


# ---- an epoch ----------------------------------------------------------------------------------------------------------------------------------------------
def test_an_epoch_covers_its_split_once(make_env, upload, hip_api):
    H, W, n = 2, 4, 300
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    nt = n_train_of(0.8, n)
    seen = {}
    for split, n_s in ((0, nt), (1, n - nt)):
        for epoch in (0, 1):
            got = []
            for first in range(0, n_s - n_s % 7, 7):                 # drop_remainder at batch 7
                got.extend(check_batch(env, d_frames, d_rows, frames, rows, n, nt, split, epoch, first, 7, "nhwc", "uint8", "default", "expert"))
            got.extend(check_batch(env, d_frames, d_rows, frames, rows, n, nt, split, epoch, n_s - n_s % 7, n_s % 7, "nhwc", "uint8", "default", "expert"))
            assert len(set(got)) == len(got) == n_s                  # never a record twice
            lib = np.empty(n_s, np.int32)                            # d_index (compared with the restatement above) equals trs_loader_order
            cfg = loader_config(hip_api, n, nt, "default", "expert", "nhwc", "uint8")
            assert hip_api.loader_order(ctypes.byref(cfg), split, epoch, 0, n_s, lib.ctypes.data) == 0
            assert np.array_equal(lib, got)
            seen[split, epoch] = got
    assert set(seen[0, 0]) == set(seen[0, 1]) and set(seen[1, 0]) == set(seen[1, 1])            # inside their split
    assert set(seen[0, 0]).isdisjoint(seen[1, 0]) and len(seen[0, 0]) + len(seen[1, 0]) == n
    assert seen[0, 0] != seen[0, 1] and seen[1, 0] != seen[1, 1]                                 # epochs 0 and 1 differ


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(make_env, upload):
    from triton_racer_sim_amd import _ffi
    H, W, n, nt = 4, 8, 10, 8
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    blind = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W, render=False)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    out = Outputs(8, H, W, "float32", 2)

    def call(handle=None, cfg=None, frames="ok", rows="ok", split=0, epoch=0, first=0, batch=4, images="ok", features="ok", labels="ok", index="ok", **fields):
        c = cfg if cfg is not None else loader_config(env.api, n, nt, "full_house", "expert", "nchw", "float32")
        for k, v in fields.items():
            setattr(c, k, v)
        pick = lambda how, ptr, off: None if how is None else ptr + (off if how == "off" else 0)
        rc = env.api.sample_batch((handle or env)._h, None if cfg is False else ctypes.byref(c), pick(frames, d_frames.data_ptr(), 2), pick(rows, d_rows.data_ptr(), 2),
                                  split, epoch, first, batch, pick(images, out.images.ptr, 4), pick(features, out.features.ptr, 2),
                                  pick(labels, out.labels.ptr, 2), pick(index, out.index.ptr, 2))
        env.sync()
        return rc

    refused = [
        dict(struct_size=36), dict(struct_size=48), dict(cfg=False),
        dict(loader=4), dict(loader=-1), dict(label=2), dict(layout=2), dict(dtype=3), dict(dtype=-1),
        dict(layout=1, dtype=2),                                     # NCHW with uint8
        dict(n_records=-1), dict(n_train=11), dict(n_train=-1),
        dict(split=2), dict(split=-1), dict(epoch=-1), dict(first=-1), dict(batch=-1),
        dict(first=5, batch=4), dict(first=8, batch=1), dict(split=1, first=0, batch=3), dict(first=2 ** 31 - 1, batch=2 ** 31 - 1),   # beyond the split
        dict(rows=None), dict(labels=None), dict(features=None), dict(frames=None), dict(images=None),                                 # a missing required pointer
        dict(images="off"), dict(features="off"), dict(labels="off"), dict(index="off"), dict(frames="off"), dict(rows="off"),         # alignment
        dict(handle=blind),                                          # frames on a handle without a camera
    ]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert env.api.last_error(), kw
        assert out.untouched(), kw
    # the same call with nothing wrong is accepted, and so are the optional pointers' absences
    assert call(batch=0) == 0 and out.untouched()
    assert call(first=4, batch=4, index=None) == 0 and not out.untouched()
    assert call(loader=0, features=None) == 0
    assert call(handle=blind, frames=None, images=None) == 0


def test_a_resident_worker_leaves_first(make_env, upload):
    """Resident mode is treated as trs_normalize treats it: the worker leaves the GPU, the gather runs on the stream, trs_sync waits for it."""
    H, W, n, nt = 8, 8, 16, 12
    env = make_env("hip", n_envs=4, img_h=H, img_w=W, auto_reset=True)
    env.set_step_mode(True)
    env.step_synthetic(3, 1)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    check_batch(env, d_frames, d_rows, frames, rows, n, nt, 0, 0, 2, 7, "nchw", "float32", "speed_ctl", "expert")
    env.step_synthetic(2, 1)
    env.sync()
    assert env.counters()[2] == 5


# ---- end to end: collect -> dataset -> batches -> pilot_loss ---------------------------------------------------------------------------------------------------
def collected(env, ticks=45):
    env.set_expert(sigma=1.5)
    frames, rows = env.collect(ticks, every=5, skip=20)
    return frames, rows


def epoch_of(ds, batch_size, epoch, split, layout, dtype, stream=None):
    imgs, feats, labels = [], [], []
    for im, fe, la in ds.batches(batch_size, epoch, split=split, layout=layout, dtype=dtype, stream=stream):
        if stream is not None:
            stream.synchronize()
        imgs.append(im.cpu().numpy()); feats.append(fe.cpu().numpy()); labels.append(la.cpu().numpy())
    return np.concatenate(imgs), np.concatenate(feats), np.concatenate(labels)


@pytest.mark.parametrize("loader,label,layout,dtype", [("speed_ctl", "expert", "nchw", "float32"), ("full_house", "applied", "nhwc", "float32"),
                                                       ("speed_feature", "expert", "nchw", "float16"), ("default", "applied", "nhwc", "uint8")])
def test_dataset_batches_equal_records_for(make_env, loader, label, layout, dtype):
    from triton_racer_sim_amd import recorder
    torch, dev = torch_dev()
    env = make_env("hip", n_envs=8, img_h=8, img_w=8, auto_reset=True)
    frames, rows = collected(env)
    h_frames, h_rows = env.to_host(frames), env.to_host(rows)
    assert h_rows.shape == (40, 8)
    ds = env.dataset(frames, rows, loader=loader, label=label, seed=5)
    env.collect(10, every=1, skip=0)                                 # the handles are gone: the dataset holds its own copy
    assert len(ds) == 40 and (ds.n_train, ds.n_val) == (32, 8)
    want_img, want_feat, want_lab = recorder.records_for(loader, h_frames, h_rows, label=label)
    for split, bs, stream in (("train", 5, None), ("val", 3, torch.cuda.Stream(dev)), ("train", 32, None)):
        for epoch in (0, 1):
            idx = ds.order(split, epoch)
            assert np.array_equal(idx, order(5, 40, 32, 0 if split == "train" else 1, epoch))
            idx = idx[:len(idx) // bs * bs]                          # drop_remainder
            img, feat, lab = epoch_of(ds, bs, epoch, split, layout, dtype, stream)
            w = want_img[idx] if dtype != "uint8" else h_frames[idx]
            w = w.astype(NP_DTYPES[dtype])
            w = w.transpose(0, 3, 1, 2) if layout == "nchw" else w
            assert img.dtype == NP_DTYPES[dtype] and np.array_equal(img.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (split, bs, epoch)
            assert np.array_equal(feat.view(np.uint32), want_feat[idx].view(np.uint32)) and feat.shape == (len(idx), N_FEATURES[loader])
            assert np.array_equal(lab.view(np.uint32), want_lab[idx].view(np.uint32))


def test_dataset_with_the_camera_codec_and_append(make_env):
    from triton_racer_sim_amd import recorder
    env = make_env("hip", n_envs=8, img_h=16, img_w=16, auto_reset=True)
    frames, rows = collected(env)
    h_frames, h_rows = env.to_host(frames), env.to_host(rows)
    ds = env.dataset(frames, rows, loader="speed_ctl", seed=9, jpeg_quality=75)
    coded = env.jpeg_roundtrip(h_frames, quality=75)
    assert not np.array_equal(coded, h_frames)
    want = recorder.records_for("speed_ctl", coded, h_rows)
    idx = ds.order("train", 3)
    img, _, lab = epoch_of(ds, 8, 3, "train", "nhwc", "float32")
    assert np.array_equal(img, want[0][idx]) and np.array_equal(lab, want[2][idx])
    # a second collection: n = 40 + 24, the split re-derived from it
    frames2, rows2 = env.collect(15, every=5, skip=0)
    h2_frames, h2_rows = env.to_host(frames2), env.to_host(rows2)
    ds.append(frames2, rows2)
    n = 40 + h2_rows.shape[0]
    assert len(ds) == n == 64 and ds.n_train == n_train_of(0.8, n) == 51 and ds.n_val == 13
    train, val = ds.order("train", 0), ds.order("val", 0)
    assert set(train).isdisjoint(val) and sorted(np.concatenate([train, val])) == list(range(n))
    assert np.array_equal(train, order(9, n, 51, 0, 0)) and np.array_equal(val, order(9, n, 51, 1, 0))
    all_frames, all_rows = np.concatenate([coded, h2_frames]), np.concatenate([h_rows, h2_rows])
    want = recorder.records_for("speed_ctl", all_frames, all_rows)
    img, _, lab = epoch_of(ds, 13, 0, "val", "nhwc", "float32")
    assert np.array_equal(img, want[0][val]) and np.array_equal(lab, want[2][val])
    with pytest.raises(ValueError):
        ds.append(None, rows2)
    for quality in (0, 101):                                         # 0 is not "no codec": refused, and nothing is copied
        with pytest.raises(ValueError):
            ds.append(frames2, rows2, jpeg_quality=quality)
    assert len(ds) == n


@pytest.mark.parametrize("with_stream", [False, True])
def test_a_batch_stays_valid_until_the_next_but_one_is_requested(make_env, with_stream):
    """What `batches` promises: batch t - 1 may be held, unread, across the request for batch t.  That request also launches the gather of batch t + 1,
    so the test waits for the env's stream as well before it reads the held batch for the first time: a gather into the held batch's buffers would show."""
    torch, dev = torch_dev()
    env = make_env("hip", n_envs=8, img_h=8, img_w=8, auto_reset=True)
    frames, rows = collected(env)
    h_frames, h_rows = env.to_host(frames), env.to_host(rows)
    ds = env.dataset(frames, rows, loader="speed_feature", split=1.0, seed=3)
    stream = torch.cuda.Stream(dev) if with_stream else None
    bs, epoch = 5, 2
    idx = ds.order("train", epoch)
    assert len(idx) == 40
    held, served = None, 0
    for t, batch in enumerate(ds.batches(bs, epoch, layout="nhwc", dtype="uint8", stream=stream)):
        if stream is not None:
            stream.synchronize()
        env.sync()                                                   # gather(t + 1) has run as well
        for u, b in ((t - 1, held), (t, batch)):
            if b is None:
                continue
            w = idx[u * bs:(u + 1) * bs]
            want_feat, want_lab = features_labels(h_rows[w], "speed_feature", "expert")
            assert np.array_equal(b[0].cpu().numpy(), h_frames[w]), (t, u)
            assert np.array_equal(b[1].cpu().numpy().view(np.uint32), want_feat.view(np.uint32)), (t, u)
            assert np.array_equal(b[2].cpu().numpy().view(np.uint32), want_lab.view(np.uint32)), (t, u)
        if held is not None:
            assert held[0].data_ptr() != batch[0].data_ptr()
        held, served = batch, served + 1
    assert served == 8


def test_pilot_loss_is_the_mse_of_the_loaded_pilot(make_env):
    """The device path (uint8 gather -> trs_pilot_forward_ex -> mean of squares in binary64 on the device) against the host path (pilot_forward_host on the
    fetched frames in the same batches of 4, the mean in numpy binary64).  The pilot's outputs are the same binary32 values on both paths, so the two
    means differ by the order in which m = 2 x 12 binary64 squares are summed alone.  Tolerance: 1e-12 relative, above the m x 2^-53 = 2.7e-15 that two
    orders of summation of m terms can differ by.  Measured on the first run (one MI355X): the host's forwards and backwards sums differ by 0 (spread
    0.000e+00 relative), and pilot_loss equals the host's mean to the bit (0.0012383324049446466 both); the test prints both figures."""
    from test_pilot_trained import trained_weights
    env = make_env("hip", n_envs=8, auto_reset=True)
    env.pilot_load(trained_weights())
    frames, rows = collected(env, ticks=60)                          # 8 captured ticks x 8 envs
    h_frames, h_rows = env.to_host(frames), env.to_host(rows)
    ds = env.dataset(frames, rows, loader="speed_ctl", seed=2)
    assert (len(ds), ds.n_train, ds.n_val) == (64, 51, 13)
    got = ds.pilot_loss("val", batch_size=4)
    idx = ds.order("val", 0)[:12]
    out = np.concatenate([env.pilot_forward_host(h_frames[idx[a:a + 4]]) for a in range(0, 12, 4)])
    _, lab = features_labels(h_rows[idx], "speed_ctl", "expert")
    sq = (out.astype(np.float64) - lab.astype(np.float64)).reshape(-1) ** 2
    want = float(np.mean(sq))
    fwd, bwd = float(np.add.reduce(sq)) / sq.size, float(np.add.reduce(sq[::-1])) / sq.size
    print(f"pilot_loss {got!r}, host {want!r}, relative difference {abs(got - want) / want:.3e}; forwards / backwards spread {abs(fwd - bwd) / want:.3e}")
    assert want > 0 and abs(got - want) <= 1e-12 * want
    with pytest.raises(ValueError):
        ds.pilot_loss("val", batch_size=14)
