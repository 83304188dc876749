"""The augmented training minibatches on the GPU (trs_sample_batch_aug; include/trsim_spec.h, "training minibatches, augmentation") against the numpy
restatement of tests/test_augment_cpu.py applied to the plain batch's inputs, bit for bit: every layout and type, the loaders and labels, frames of one
quad per row whose starts are only 4-byte aligned, rows whose middle quad maps onto itself, a batch with more work items than the grid has workgroups;
mirror probabilities 0, 0.5 and 1; the jitter off, moderate and at its extremes; a guard band of known bytes around every output; the off path against
trs_sample_batch; the refusals; and the Python layer.  Device buffers are filled directly: only trs_sample_batch_aug is under test up to there.
A batch of one record cannot hold a mirrored and an unmirrored record: at batch 1 two windows are compared, one of each kind."""
import ctypes

import numpy as np
import pytest

from test_augment_cpu import BELOW_ONE, REFUSALS, augment_config, augmentation, augmented_frames, augmented_labels
from test_loader_cpu import F, N_FEATURES, features_labels, images_of, n_train_of, order
from test_loader_gpu import CANARY, COMBOS, SEED, Outputs, loader_config, torch_dev, upload  # noqa: F401  (upload is a fixture)

pytestmark = pytest.mark.gpu

AUG_SEED = 0xA06
RULES = [(lo, la) for lo in ("speed_ctl", "default", "speed_feature") for la in ("expert", "applied")]
MODERATE = dict(gain=0.25, bias=32.0)
EXTREME = dict(gain=BELOW_ONE, bias=255.0)
AUGS = [dict(mirror=0.5), dict(mirror=0.5, per_channel=True, **MODERATE), dict(mirror=0.5, **MODERATE), dict(mirror=1.0, per_channel=True, **EXTREME),
        dict(mirror=0.0, **EXTREME), dict(mirror=1.0), dict(mirror=0.0, per_channel=True, **MODERATE)]


def make_set(n, H, W, seed=2):
    """n records of random bytes, none of which equals its own mirror image; rows with negative speeds and steering labels of both signs and zero."""
    rng = np.random.default_rng(seed + 1000 * n + H * W)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    assert all(not np.array_equal(f, f[:, ::-1]) for f in frames)
    rows = rng.uniform(-1, 1, (n, 8)).astype(F)
    rows[:, 4] = rng.uniform(-5, 25, n).astype(F)
    rows[:min(n, 2), 0] = np.array([0.0, -0.0], F)[:min(n, 2)]
    rows[:, 6] = (rng.integers(0, 1185, n) / 1185 * 10).astype(F)
    return frames, rows


def both_clamps_occur(frames, params):
    """R1's t = x * gain + bias + 0.5 (each operation rounded) reaches t <= 0 and t >= 255 among these records."""
    t = frames.astype(F) * params[:, None, None, 0:3]
    t = (t + params[:, None, None, 4:7]).astype(F)
    t = (t + F(0.5)).astype(F)
    return bool((t <= 0).any() and (t >= 255).any())


def window(n, nt, split, epoch, batch, aug, want):
    """A `first` whose window of `batch` positions holds mirrored records (`want` = "both": and unmirrored ones; True / False: only such), by the restatement."""
    n_s = nt if split == 0 else n - nt
    flags, _ = augmentation(AUG_SEED, epoch, order(SEED, n, nt, split, epoch), aug.get("mirror", 0.0))
    for first in range(n_s - batch, -1, -1):
        w = flags[first:first + batch]
        if (w.any() and not w.all()) if want == "both" else bool(w.all()) == want and bool(w.any()) == want:
            return first
    raise AssertionError(("no such window", n, nt, split, epoch, batch, aug, want))


def check_batch(env, d_frames, d_rows, frames, rows, n, nt, split, epoch, first, batch, layout, dtype, loader, label, aug, extra=2):
    H, W = env.H, env.W
    cfg, a = loader_config(env.api, n, nt, loader, label, layout, dtype), augment_config(env.api, seed=AUG_SEED, **aug)
    out = Outputs(batch + extra, H, W, dtype, N_FEATURES[loader])
    with_frames = frames is not None
    rc = env.api.sample_batch_aug(env._h, ctypes.byref(cfg), ctypes.byref(a), d_frames.data_ptr() if with_frames else None, d_rows.data_ptr(), split, epoch, first,
                                  batch, out.images.ptr if with_frames else None, out.features.ptr, out.labels.ptr, out.index.ptr)
    assert rc == 0, env.api.last_error()
    env.sync()
    what = (H, W, n, nt, split, epoch, first, batch, layout, dtype, loader, label, aug)
    idx = order(SEED, n, nt, split, epoch, first, batch)
    flags, params = augmentation(AUG_SEED, epoch, idx, **aug)
    want_feat, want_lab = features_labels(rows[idx], loader, label)
    want_lab = augmented_labels(want_lab, flags)
    wanted = [(out.features, want_feat), (out.labels, want_lab), (out.index, idx.astype(np.int32))]
    if with_frames:
        wanted.append((out.images, images_of(augmented_frames(frames[idx], flags, params), layout, dtype)))
    else:
        assert out.images.untouched(), what
    for buf, want in wanted:
        pre, got, post = buf.host()
        want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert np.array_equal(got[:want.size], want), what                            # bit for bit
        assert np.all(got[want.size:] == CANARY), what                                # slots beyond `batch`
        assert np.all(pre == CANARY) and np.all(post == CANARY), what                 # the guard band: a frame (images) / 256 bytes either side
    return idx, flags, params


# ---- bit-exact against the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(3, 4), (2, 8), (5, 12), (120, 160)])
def test_batches_equal_the_restatement(make_env, upload, H, W):
    """3 x 4: one quad per row and 36-byte frames, so record r starts at a multiple of 4 and no more; 2 x 8: two quads that swap; 5 x 12: odd height, the
    middle quad of a row maps onto itself; 120 x 160: five work items per slot, the last one partial, rows that straddle waves and items."""
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    n, nt = 64, n_train_of(0.8, 64)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    case = 0
    for aug in AUGS:
        for layout, dtype in COMBOS:
            loader, label = RULES[case % len(RULES)]
            split, epoch = (0, 1 + case % 3) if case % 4 else (1, 2)
            case += 1
            first = window(n, nt, split, epoch, 7, aug, "both") if aug["mirror"] == 0.5 else (nt if split == 0 else n - nt) - 7
            idx, flags, params = check_batch(env, d_frames, d_rows, frames, rows, n, nt, split, epoch, first, 7, layout, dtype, loader, label, aug)
            assert {0.0: not flags.any(), 0.5: flags.any() and not flags.all(), 1.0: flags.all()}[aug["mirror"]]
            if aug.get("gain") == BELOW_ONE:
                assert both_clamps_occur(frames[idx], params), (H, W, aug)
    # batch 1: a mirrored record and an unmirrored one, in every layout and type
    aug = dict(mirror=0.5, per_channel=True, **MODERATE)
    for layout, dtype in COMBOS:
        seen = set()
        for want in (True, False):
            _, flags, _ = check_batch(env, d_frames, d_rows, frames, rows, n, nt, 0, 1, window(n, nt, 0, 1, 1, aug, want), 1, layout, dtype, "speed_ctl", "applied", aug)
            seen.add(bool(flags[0]))
        assert seen == {True, False}
    # every loader x label at one window
    for loader, label in RULES:
        check_batch(env, d_frames, d_rows, frames, rows, n, nt, 0, 2, window(n, nt, 0, 2, 7, aug, "both"), 7, "nchw", "float32", loader, label, aug)


@pytest.mark.parametrize("layout,dtype", COMBOS)
def test_more_items_than_workgroups(make_env, upload, layout, dtype):
    """A 2 x 8 frame is one work item, so a batch of more slots than the grid's cu_count * 16 workgroups makes workgroups stride over items."""
    torch, dev = torch_dev()
    batch = torch.cuda.get_device_properties(dev).multi_processor_count * 16 + 5
    env = make_env("hip", n_envs=1, track=None, img_h=2, img_w=8)
    n = batch + 3
    frames, rows = make_set(n, 2, 8)
    d_frames, d_rows = upload(frames, rows)
    aug = dict(mirror=0.5, per_channel=True, **MODERATE)
    _, flags, _ = check_batch(env, d_frames, d_rows, frames, rows, n, n, 0, 1, 2, batch, layout, dtype, "speed_feature", "expert", aug, extra=1)
    assert flags.any() and not flags.all()


def test_full_house_takes_the_jitter_and_refuses_the_mirror(make_env, upload):
    H, W, n, nt = 5, 12, 37, 29
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    for label in ("expert", "applied"):
        check_batch(env, d_frames, d_rows, frames, rows, n, nt, 0, 3, 4, 7, "nchw", "float32", "full_house", label, dict(per_channel=True, **MODERATE))
    cfg, a = loader_config(env.api, n, nt, "full_house", "expert", "nchw", "float32"), augment_config(env.api, mirror=0.5, **MODERATE)
    out = Outputs(8, H, W, "float32", 2)
    assert env.api.sample_batch_aug(env._h, ctypes.byref(cfg), ctypes.byref(a), d_frames.data_ptr(), d_rows.data_ptr(), 0, 3, 4, 7, out.images.ptr, out.features.ptr,
                                    out.labels.ptr, out.index.ptr) == -1
    assert b"FULL_HOUSE" in env.api.last_error()
    env.sync()
    assert out.untouched()


def test_a_physics_only_set_flips_labels_alone(make_env):
    env = make_env("hip", n_envs=1, track=None, render=False)
    n, nt = 37, 29
    _, rows = make_set(n, 2, 4)
    torch, dev = torch_dev()
    d_rows = torch.as_tensor(rows).to(dev)
    torch.cuda.current_stream(dev).synchronize()
    aug = dict(mirror=0.5, per_channel=True, **MODERATE)
    for label in ("expert", "applied"):
        _, flags, _ = check_batch(env, None, d_rows, None, rows, n, nt, 0, 4, window(n, nt, 0, 4, 7, aug, "both"), 7, "nchw", "float32", "speed_feature", label, aug)
        assert flags.any() and not flags.all()


# ---- the off path ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", COMBOS)
def test_off_is_trs_sample_batch(make_env, upload, layout, dtype):
    """aug NULL and the off config (whatever its seed and per_channel) give the bytes of trs_sample_batch in images, features, labels and index."""
    H, W, n, nt = 5, 12, 37, 29
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    cfg = loader_config(env.api, n, nt, "full_house", "applied", layout, dtype)
    got = []
    for a in ("plain", None, augment_config(env.api), augment_config(env.api, per_channel=True, seed=77)):
        out = Outputs(9, H, W, dtype, 2)
        tail = (d_frames.data_ptr(), d_rows.data_ptr(), 0, 2, 11, 7, out.images.ptr, out.features.ptr, out.labels.ptr, out.index.ptr)
        if a == "plain":
            rc = env.api.sample_batch(env._h, ctypes.byref(cfg), *tail)
        else:
            rc = env.api.sample_batch_aug(env._h, ctypes.byref(cfg), None if a is None else ctypes.byref(a), *tail)
        assert rc == 0, env.api.last_error()
        env.sync()
        got.append([b.t.cpu().numpy() for b in out.all()])
    assert not np.all(got[0][0] == CANARY)
    for other in got[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(got[0], other))              # guards included


# ---- determinism -------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_repeats_and_epochs_differ(make_env, upload):
    H, W, n = 5, 12, 37
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    aug = dict(mirror=0.5, per_channel=True, **MODERATE)
    cfg, a = loader_config(env.api, n, n, "default", "expert", "nhwc", "uint8"), augment_config(env.api, seed=AUG_SEED, **aug)
    runs = {}
    for key, epoch, first in (("a", 0, 0), ("b", 0, 0), ("c", 1, 0)):
        out = Outputs(n, H, W, "uint8", 0)
        assert env.api.sample_batch_aug(env._h, ctypes.byref(cfg), ctypes.byref(a), d_frames.data_ptr(), d_rows.data_ptr(), 0, epoch, first, n, out.images.ptr,
                                        None, out.labels.ptr, out.index.ptr) == 0, env.api.last_error()
        env.sync()
        runs[key] = [b.host()[1].copy() for b in (out.images, out.labels, out.index)]
    assert all(np.array_equal(x, y) for x, y in zip(runs["a"], runs["b"]))
    # the whole set is one batch in both epochs: every record is in both, at other positions; one that the restatement draws differently differs
    by_record = {}
    for key in ("a", "c"):
        img, _, index = runs[key]
        index = index.view(np.int32)
        by_record[key] = {int(r): img.reshape(n, -1)[k] for k, r in enumerate(index)}
    f0, p0 = augmentation(AUG_SEED, 0, np.arange(n), **aug)
    f1, p1 = augmentation(AUG_SEED, 1, np.arange(n), **aug)
    changed = [r for r in range(n) if f0[r] != f1[r]]
    assert changed and sorted(by_record["a"]) == sorted(by_record["c"]) == list(range(n))
    assert all(not np.array_equal(by_record["a"][r], by_record["c"][r]) for r in changed)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(make_env, upload):
    H, W, n, nt = 4, 8, 10, 8
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    frames, rows = make_set(n, H, W)
    d_frames, d_rows = upload(frames, rows)
    out = Outputs(8, H, W, "float32", 1)

    def call(a, first=0, batch=4, rows_ptr=True, images_off=0, **fields):
        c = loader_config(env.api, n, nt, "speed_feature", "expert", "nchw", "float32")
        for k, v in fields.items():
            setattr(c, k, v)
        rc = env.api.sample_batch_aug(env._h, ctypes.byref(c), ctypes.byref(a), d_frames.data_ptr(), d_rows.data_ptr() if rows_ptr else None, 0, 0, first, batch,
                                      out.images.ptr + images_off, out.features.ptr, out.labels.ptr, out.index.ptr)
        env.sync()
        return rc

    for field, value, word in REFUSALS:
        a = augment_config(env.api, 0.5, 0.25, 32.0)
        setattr(a, field, value)
        assert call(a) == -1 and word in env.api.last_error().decode(), (field, value)
        assert out.untouched(), (field, value)
    a = augment_config(env.api, 0.5, 0.25, 32.0)
    for kw in (dict(first=5), dict(batch=-1), dict(rows_ptr=False), dict(images_off=4), dict(loader=4), dict(n_train=11), dict(struct_size=36), dict(layout=1, dtype=2)):
        assert call(a, **kw) == -1, kw                                                # trs_sample_batch's refusals, unchanged
        assert out.untouched(), kw
    assert call(a, batch=0) == 0 and out.untouched()
    assert call(a) == 0 and not out.untouched()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------------------------
def epoch_of(ds, batch_size, epoch, split, layout, dtype, augment):
    got = [[t.cpu().numpy() for t in batch] for batch in ds.batches(batch_size, epoch, split=split, layout=layout, dtype=dtype, augment=augment)]
    return [np.concatenate(part) for part in zip(*got)]


@pytest.mark.parametrize("layout,dtype", [("nchw", "float32"), ("nhwc", "uint8")])
def test_dataset_batches_with_an_augment(make_env, layout, dtype):
    from triton_racer_sim_amd import Augment, DeviceDataset
    H, W, n = 8, 8, 40
    env = make_env("hip", n_envs=1, track=None, img_h=H, img_w=W)
    frames, rows = make_set(n, H, W)
    ds = DeviceDataset(env, loader="speed_feature", label="applied", seed=5).append(frames, rows)
    assert (len(ds), ds.n_train) == (40, 32)
    epoch, bs = 3, 5
    idx = ds.order("train", epoch)[:30]
    plain_img, plain_feat, plain_lab = epoch_of(ds, bs, epoch, "train", layout, dtype, None)           # augment=None: today's output
    want_feat, want_lab = features_labels(rows[idx], "speed_feature", "applied")
    assert np.array_equal(plain_img, images_of(frames[idx], layout, dtype)) and np.array_equal(plain_lab.view(np.uint32), want_lab.view(np.uint32))
    # the mirror alone: ds.augmentation says which records of the plain batch come out flipped
    mirror_only = Augment(mirror=0.5, seed=11)
    index, mirror, params = ds.augmentation(mirror_only, "train", epoch, 0, 30)
    assert np.array_equal(index, idx) and mirror.any() and not mirror.all() and np.all(params[:, 0:3] == 1) and np.all(params[:, 4:7] == 0)
    img, feat, lab = epoch_of(ds, bs, epoch, "train", layout, dtype, mirror_only)
    w_axis = 3 if layout == "nchw" else 2
    for k in range(30):
        assert np.array_equal(img[k], np.flip(plain_img[k], w_axis - 1) if mirror[k] else plain_img[k]), k
        assert lab[k, 0].view(np.uint32) == plain_lab[k, 0].view(np.uint32) ^ (np.uint32(0x80000000) if mirror[k] else np.uint32(0)) and lab[k, 1] == plain_lab[k, 1]
    assert np.array_equal(feat, plain_feat)
    # mirror and jitter: the C call's answer, i.e. the restatement's
    full = Augment(mirror=0.5, gain=0.2, bias=20, per_channel=True, seed=12)
    index, mirror, params = ds.augmentation(full, "train", epoch)
    flags, want_params = augmentation(12, epoch, ds.order("train", epoch), 0.5, 0.2, 20.0, True)
    assert len(index) == 32 and np.array_equal(mirror, flags) and np.array_equal(params.view(np.uint32), want_params.view(np.uint32))
    img, feat, lab = epoch_of(ds, bs, epoch, "train", layout, dtype, full)
    assert np.array_equal(img.view(np.uint8), images_of(augmented_frames(frames[idx], flags[:30], want_params[:30]), layout, dtype).view(np.uint8))
    assert np.array_equal(lab.view(np.uint32), augmented_labels(want_lab, flags[:30]).view(np.uint32)) and np.array_equal(feat, want_feat)
    with pytest.raises(TypeError):
        next(ds.batches(bs, epoch, augment=dict(mirror=0.5)))
    house = DeviceDataset(env, loader="full_house", seed=5).append(frames, rows)
    with pytest.raises(RuntimeError, match="FULL_HOUSE"):
        next(house.batches(bs, epoch, augment=mirror_only))
    assert len(list(house.batches(bs, epoch, augment=Augment(gain=0.2, bias=20)))) == 6
