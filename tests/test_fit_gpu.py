"""The trainer as the product strings it together (DeviceDataset.fit_tail / fit in triton-racer-sim_amd/dataset.py, the session calls of env.py underneath)
against the same fit driven by hand on a twin handle.  The kernels it calls are pinned elsewhere (the gathers in tests/test_loader_gpu.py and
tests/test_augment_gpu.py, the step in tests/test_train_gpu.py and tests/test_train_conv_gpu.py); here the loop is: which epoch and which records a step gets,
what validation is measured on, which weights are kept, when the run stops, and what a fit that raises leaves behind.

hand_fit takes HOST arrays and uses no DeviceDataset, no batches() and no pilot_loss: the epoch's order from the numpy restatement (test_loader_cpu.order), each
batch built on the host (and augmented by the restatement of test_augment_cpu), uploaded into two scratch slots and stepped; the validation loss from
pilot_forward_host on the frames as collected, in binary64.  Training is deterministic, so the two handles agree exactly: every weight comparison is bit for bit.
A loss of the fit and the twin's are binary64 means of the same non-negative binary32-derived terms added in different orders: a sum of n such terms errs by at
most (n - 1) 2^-53 of itself in any order, the division rounds once more, so the two differ by at most n 2^-52 of the value — n = the batches of the epoch for the
training loss, 2 x batches x val_batch for the validation loss.  No other tolerance appears.

The set: 200 records of slice_frames whose labels are a function of the frame's mean colours plus noise (NOISE), so that the validation loss falls for a few
epochs and rises once the noise is being fitted (LR; both chosen on the device from a short list as the first pair that meets the conditions can_tell asserts,
profiles/r35_fit_loop.txt).  split 0.8: 160 training records, six batches of 24 per epoch (16 dropped; past one lap of batches()'s three buffer sets), 40 validation
records: two batches of 16 or one of 24."""
import functools
import math
import time

import numpy as np
import pytest

from test_augment_cpu import augmentation, augmented_frames, augmented_labels
from test_loader_cpu import features_labels, images_of, n_train_of, order
from test_pilot_slices import slice_frames
from test_train_gpu import bits, tail_weights
from triton_racer_sim_amd import _ffi

f32, EPS = np.float32, 2.0 ** -52
SMALLEST, CHAIN = (93, 100), (96, 128)          # conv7 is one pixel and no chain is planned; the chain runs and the interior is materialised
RECORDS, SPLIT, SEED, CARS = 200, 0.8, 7, 24
LR, NOISE = 5e-3, 0.6                          # the first of noise (0.3, 0.6, 1.0, 0.15) x lr (2e-3, 3e-3, 5e-3, 1e-2), noise outermost, that meets the conditions
AUGMENT = (("mirror", 0.5), ("gain", 0.2), ("bias", 20.0), ("per_channel", True), ("seed", 12))
ALL_CONVS = ("conv4", "conv5", "conv6", "conv7")
STATE = ("pos_x", "pos_y", "pos_z", "yaw", "vel", "speed", "cte", "seg_idx", "done", "ep_return", "ep_len")
CTL = ("ctl_steer", "ctl_thr", "ctl_brk")


# ---- the rule of the run ---------------------------------------------------------------------------------------------------------------------
def expected_run(val_losses, epochs, patience):
    """(epochs_run, best_epoch) of a fit whose validation losses would be val_losses[0 .. epochs - 1]: a strictly smaller loss is the new best and resets the
    count, anything else counts; `patience` counts in a row end the run (None: never)."""
    best, best_val, since = None, math.inf, 0
    for epoch in range(epochs):
        if val_losses[epoch] < best_val:
            best, best_val, since = epoch, val_losses[epoch], 0
        else:
            since += 1
            if patience is not None and since >= patience:
                return epoch + 1, best
    return epochs, best


def test_a_tie_after_the_minimum_keeps_the_first_and_counts():
    assert expected_run([0.5, 0.3, 0.3, 0.2, 0.4], 5, 2) == (5, 3)          # the tie counts once, the next epoch improves
    assert expected_run([0.5, 0.3, 0.3, 0.3, 0.1], 5, 2) == (4, 1)          # two ties in a row stop the run on the first minimum
    assert expected_run([0.5, 0.3, 0.3, 0.3, 0.1], 5, None) == (5, 4)


def test_a_minimum_in_the_first_epoch():
    assert expected_run([0.1, 0.2, 0.3, 0.4], 4, 2) == (3, 0)
    assert expected_run([0.1, 0.2, 0.05, 0.4], 4, 2) == (4, 2)
    assert expected_run([0.1], 1, 1) == (1, 0)


def test_patience_one_stops_at_the_first_epoch_that_is_not_better():
    assert expected_run([0.5, 0.4, 0.45, 0.1, 0.0], 5, 1) == (3, 1)
    assert expected_run([0.5, 0.4, 0.3, 0.2, 0.1], 5, 1) == (5, 4)
    assert expected_run([0.5, 0.5, 0.1], 3, 1) == (2, 0)


def test_patience_larger_than_epochs_never_stops():
    assert expected_run([0.5, 0.6, 0.7, 0.8], 4, 5) == (4, 0)
    assert expected_run([0.5, 0.6, 0.7, 0.8], 4, 4) == (4, 0)               # three epochs did not improve: one short of four
    assert expected_run([0.5, 0.6, 0.7, 0.8], 4, 3) == (4, 0)               # the third falls on the last epoch: the run is over either way
    assert expected_run([0.5, 0.6, 0.7, 0.8, 0.9], 5, 3) == (4, 0)


def test_an_all_rising_list_and_none():
    rising = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    assert expected_run(rising, 6, 2) == (3, 0) and expected_run(rising, 6, 1) == (2, 0)
    assert expected_run(rising, 6, None) == (6, 0)
    assert expected_run([0.3, 0.2, 0.25, 0.1, 0.4, 0.5], 6, None) == (6, 3)
    assert expected_run(rising, 3, None) == (3, 0)                           # only the first `epochs` values are looked at


# ---- the set, the pilot, the twin ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noisy_set(h, w, noise=NOISE, n=RECORDS, seed=5):
    """(frames uint8[n, h, w, 3], rows float32[n, 8]), read-only: steering follows the frame's brightness, speed its red against its blue, both under noise"""
    frames = slice_frames(h, w, n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    colour = frames.reshape(n, -1, 3).mean(1) / 255.0
    grey = colour.mean(1)
    rows = rng.uniform(-1.0, 1.0, (n, 8)).astype(f32)
    rows[:, 0] = np.clip(8.0 * (grey - grey.mean()) + noise * rng.standard_normal(n), -1.0, 1.0)
    rows[:, 4] = 20.0 * (0.5 + 5.0 * (colour[:, 0] - colour[:, 2]) + noise * rng.standard_normal(n))
    frames.setflags(write=False); rows.setflags(write=False)
    return frames, rows


@functools.lru_cache(maxsize=None)
def loaded_weights(h, w):
    named, _ = tail_weights(h, w, seed=3)
    return tuple(np.ascontiguousarray(a, f32) for nm in _ffi.PILOT_LAYERS[22] for a in named[nm])


def writable(frames, rows):
    """Copies for DeviceDataset.append: torch does not take a read-only array"""
    return (None if frames is None else np.array(frames)), np.array(rows)


def fresh(make_env, h, w, weights, n_envs=CARS, **kw):
    env = make_env("hip", n_envs=n_envs, img_h=h, img_w=w, **kw)
    env.pilot_load(list(weights))
    return env


def hand_fit(env, frames, rows, epochs, batch, val_batch=None, augment=None, seed=SEED, split=SPLIT, convs=None, **adam):
    """The fit on host arrays through the session calls alone.  Returns ([(train_loss, val_loss)] per epoch, [the 22 arrays after the epoch] per epoch)."""
    n = len(rows)
    n_train = n_train_of(split, n)
    n_val = n - n_train
    _, labels = features_labels(rows, "speed_ctl", "expert")
    val_batch = max(min(env.n, n_val), 1) if val_batch is None else val_batch
    val = order(seed, n, n_train, 1, 0)[:n_val // val_batch * val_batch]
    history, weights = [], []
    env.pilot_train_begin(convs=convs, **adam)
    try:
        for epoch in range(epochs):
            records = order(seed, n, n_train, 0, epoch)
            losses = []
            for t in range(n_train // batch):
                rec = records[t * batch:(t + 1) * batch]
                x, y = images_of(frames[rec], "nhwc", "uint8"), labels[rec]
                if augment is not None:
                    flags, params = augmentation(augment.seed, epoch, rec, augment.mirror, augment.gain, augment.bias, augment.per_channel)
                    x, y = augmented_frames(x, flags, params), augmented_labels(y, flags)
                d_x, d_y = env.scratch(20, x.shape, np.uint8), env.scratch(21, (batch, 2), np.float32)
                env.upload(d_x, x); env.upload(d_y, y)
                losses.append(env.pilot_train_step(d_x, d_y, batch))
            out = np.concatenate([env.pilot_forward_host(frames[val[a:a + val_batch]]) for a in range(0, len(val), val_batch)])
            val_loss = float(np.mean((out.astype(np.float64) - labels[val].astype(np.float64)) ** 2))
            history.append((float(np.mean(np.asarray(losses, f32).astype(np.float64))), val_loss))
            weights.append(env.pilot_weights())
    finally:
        env.pilot_train_end()
    return history, weights


def case(**kw):
    c = dict(h=SMALLEST[0], w=SMALLEST[1], epochs=3, batch=CARS, val_batch=None, augment=None, patience=None, convs=None, layers=None, lr=LR, alias=False)
    assert set(kw) <= set(c)
    c.update(kw)
    return c


def augment_of(c):
    from triton_racer_sim_amd.dataset import Augment
    return None if c["augment"] is None else Augment(**dict(c["augment"]))


TWINS = {}


def twin_fit(make_env, c):
    """The twin's trajectory of a case over all its epochs, computed once per process: the cases that differ in `patience` alone, or that run a prefix of
    another's epochs, share it."""
    convs = ALL_CONVS if c["alias"] else c["convs"]
    key = (c["h"], c["w"], c["batch"], c["val_batch"], c["augment"], convs, c["layers"], c["lr"])
    if key not in TWINS or len(TWINS[key][0]) < c["epochs"]:
        frames, rows = noisy_set(c["h"], c["w"])
        adam = {"lr": c["lr"]} if c["layers"] is None else {"lr": c["lr"], "layers": c["layers"]}
        t0 = time.perf_counter()
        twin = fresh(make_env, c["h"], c["w"], loaded_weights(c["h"], c["w"]))
        TWINS[key] = hand_fit(twin, frames, rows, c["epochs"], c["batch"], c["val_batch"], augment_of(c), convs=convs, **adam)
        print(f"twin {key}: {time.perf_counter() - t0:.2f} s; (train, val) per epoch " + ", ".join(f"({a:.6f}, {v:.6f})" for a, v in TWINS[key][0]))
    history, weights = TWINS[key]
    return history[:c["epochs"]], weights[:c["epochs"]]


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------------
def refused_without_a_session(env):
    rc = env.api.pilot_train_end(env._h)
    assert rc == -2 and "trs_pilot_train_begin first" in (env.api.last_error() or b"").decode(), (rc, env.api.last_error())


def can_tell(vals, epochs, patience, early):
    """The conditions on the twin's trajectory alone: no decision hangs on the summation order, and (early) the best epoch is neither the first nor the last run"""
    for i in range(len(vals)):
        for j in range(i):
            assert abs(vals[i] - vals[j]) > 1e-9 * max(vals[i], vals[j]), (i, j, vals)
    epochs_run, best = expected_run(vals, epochs, patience)
    if patience is not None:
        assert 1 <= best < epochs_run - 1 < epochs - 1, (best, epochs_run, vals)
    elif early:
        assert 1 <= best < epochs - 1 and epochs_run == epochs, (best, vals)
    return epochs_run, best


def compare(make_env, env, loaded, history, twin_history, twin_weights, epochs_run, best, n, batch, val_batch, trained, probe):
    """A finished fit on `env` (which held `loaded` before it) against the twin's trajectory.  trained: the numbers of the arrays the fit may move."""
    assert len(history) == epochs_run, (len(history), epochs_run, history)
    n_train = n_train_of(SPLIT, n)
    n_val = n - n_train
    val_batch = max(min(env.n, n_val), 1) if val_batch is None else val_batch
    train_terms, val_terms = n_train // batch, 2 * (n_val // val_batch) * val_batch
    for epoch, ((fit_t, fit_v), (twin_t, twin_v)) in enumerate(zip(history, twin_history)):
        gap_t, gap_v = abs(fit_t - twin_t) / twin_t, abs(fit_v - twin_v) / twin_v
        print(f"epoch {epoch}: train {fit_t:.9g} (twin {twin_t:.9g}, gap {gap_t:.1e} of {train_terms * EPS:.1e}), val {fit_v:.9g} (twin {twin_v:.9g}, gap {gap_v:.1e} of {val_terms * EPS:.1e})")
        assert abs(fit_t - twin_t) <= train_terms * EPS * twin_t, (epoch, fit_t, twin_t)
        assert abs(fit_v - twin_v) <= val_terms * EPS * twin_v, (epoch, fit_v, twin_v)
    got = env.pilot_weights()
    assert len(got) == 22
    for i in range(22):
        assert np.array_equal(bits(got[i]), bits(twin_weights[best][i])), (i, best)
        if i in trained:
            assert not np.array_equal(bits(got[i]), bits(loaded[i])), i          # the comparison above is of weights that moved
        else:
            assert np.array_equal(bits(got[i]), bits(loaded[i])), i
    third = fresh(make_env, env.H, env.W, twin_weights[best], n_envs=env.n)
    assert np.array_equal(bits(env.pilot_forward_host(probe)), bits(third.pilot_forward_host(probe)))
    refused_without_a_session(env)
    env.pilot_load(got)                                                          # and a load is taken again


def trained_arrays(convs, layers):
    tail = _ffi.TRAIN_LAYERS if layers is None else layers
    names = _ffi.PILOT_LAYERS[22]
    return {2 * names.index(nm) + j for nm in tuple(tail) + tuple(convs or ()) for j in (0, 1)}


def check_fit(make_env, c, env=None, ds=None, early=False):
    frames, rows = noisy_set(c["h"], c["w"])
    loaded = loaded_weights(c["h"], c["w"])
    twin_history, twin_weights = twin_fit(make_env, c)
    epochs_run, best = can_tell([v for _, v in twin_history], c["epochs"], c["patience"], early)
    env = fresh(make_env, c["h"], c["w"], loaded) if env is None else env
    ds = env.dataset(*writable(frames, rows), seed=SEED) if ds is None else ds
    assert (len(ds), ds.n_train, ds.n_val) == (RECORDS, 160, 40)
    kw = {k: c[k] for k in ("patience", "layers") if c[k] is not None}
    if c["val_batch"] is not None:
        kw["val_batch_size"] = c["val_batch"]
    if c["augment"] is not None:
        kw["augment"] = augment_of(c)
    t0 = time.perf_counter()
    if c["alias"]:
        history, convs = ds.fit(c["epochs"], c["batch"], lr=c["lr"], **kw), ALL_CONVS
    else:
        history, convs = ds.fit_tail(c["epochs"], c["batch"], convs=c["convs"], lr=c["lr"], **kw), c["convs"]
    print(f"fit {c['h']}x{c['w']}: {time.perf_counter() - t0:.2f} s, {len(history)} of {c['epochs']} epochs, best {best}")
    compare(make_env, env, loaded, history, twin_history, twin_weights, epochs_run, best, RECORDS, c["batch"], c["val_batch"], trained_arrays(convs, c["layers"]), frames[:8])
    return history


# ---- 1. plain ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [SMALLEST, CHAIN], ids=["93x100", "96x128"])
def test_a_plain_fit_equals_the_fit_driven_by_hand(make_env, h, w):
    check_fit(make_env, case(h=h, w=w))


# ---- 2. augmented ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_augmented_fit_draws_anew_every_epoch_and_validates_on_the_frames_as_collected(make_env):
    c = case(augment=AUGMENT)
    a = dict(AUGMENT)
    n_train = n_train_of(SPLIT, RECORDS)
    flags = []
    for epoch in range(c["epochs"]):
        used = order(SEED, RECORDS, n_train, 0, epoch)[:n_train // CARS * CARS]
        mirrored = augmentation(a["seed"], epoch, used, a["mirror"], a["gain"], a["bias"], a["per_channel"])[0]
        assert 0 < mirrored.sum() < len(used), epoch
        flags.append(augmentation(a["seed"], epoch, np.arange(RECORDS), a["mirror"], a["gain"], a["bias"], a["per_channel"])[0])
    assert not np.array_equal(flags[0], flags[1])
    history = check_fit(make_env, c)
    plain, _ = twin_fit(make_env, case())
    assert history[0][0] != plain[0][0]                                          # (the augmentation reached the step)


# ---- 3. layers, convs, the alias ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_layers_and_convs_reach_the_session_through_fit_tail(make_env):
    check_fit(make_env, case(layers=("dense2", "output_layer"), convs=("conv5", "conv7")))


@pytest.mark.gpu
def test_fit_is_fit_tail_with_the_last_four_convolutions(make_env):
    check_fit(make_env, case(alias=True))


# ---- 4. the validation batch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_val_batch_size_chooses_the_records_the_validation_loss_is_taken_on(make_env):
    two_of_16 = check_fit(make_env, case(val_batch=16))
    one_of_24 = check_fit(make_env, case())
    for (train_a, val_a), (train_b, val_b) in zip(two_of_16, one_of_24):
        assert train_a == train_b and val_a != val_b


# ---- 5. early stop -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("patience", [2, 1, None])
def test_early_stop_ends_the_run_by_the_rule_and_keeps_the_best_epoch(make_env, patience):
    history = check_fit(make_env, case(epochs=8, patience=patience), early=True)
    assert (len(history) == 8) == (patience is None)


# ---- 6. re-fit after aggregation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_refit_after_append_uses_the_split_and_order_of_the_larger_set(make_env):
    h, w = SMALLEST
    loaded = loaded_weights(h, w)
    env = fresh(make_env, h, w, loaded, auto_reset=True)
    env.set_expert()
    frames, rows = env.collect(ticks=30, every=5, skip=5)
    frames_1, rows_1 = env.to_host(frames), env.to_host(rows)
    ds = env.dataset(frames, rows, seed=SEED)                                  # the device handles, as the product's loop passes them
    n_1 = len(rows_1)
    assert n_1 == 5 * CARS == len(ds) and ds.n_train == n_train_of(SPLIT, n_1)
    first = ds.fit_tail(2, CARS, lr=LR)
    twin = fresh(make_env, h, w, loaded)
    twin_first, weights_first = hand_fit(twin, frames_1, rows_1, 2, CARS, lr=LR)
    print("first fit, twin (train, val): " + ", ".join(f"({a:.6f}, {v:.6f})" for a, v in twin_first))
    run_1, best_1 = can_tell([v for _, v in twin_first], 2, None, False)
    tail = trained_arrays(None, None)
    compare(make_env, env, loaded, first, twin_first, weights_first, run_1, best_1, n_1, CARS, None, tail, frames_1[:8])
    frames, rows = env.collect(ticks=30, every=5, skip=5, driver="pilot", beta=0.5)       # the pilot the first fit left drives: only this handle has these frames
    frames_2, rows_2 = env.to_host(frames), env.to_host(rows)
    ds.append(frames, rows)
    n = n_1 + len(rows_2)
    assert len(rows_2) >= 5 * CARS and len(rows_2) % CARS == 0
    assert len(ds) == n and ds.n_train == n_train_of(SPLIT, n) and ds.n_val == n - n_train_of(SPLIT, n)
    assert not np.array_equal(frames_2[:n_1], frames_1)
    second = ds.fit_tail(2, CARS, lr=LR)
    twin.pilot_load(weights_first[best_1])
    twin_second, weights_second = hand_fit(twin, np.concatenate([frames_1, frames_2]), np.concatenate([rows_1, rows_2]), 2, CARS, lr=LR)
    print(f"second fit on {n} records, twin (train, val): " + ", ".join(f"({a:.6f}, {v:.6f})" for a, v in twin_second))
    run_2, best_2 = can_tell([v for _, v in twin_second], 2, None, False)
    compare(make_env, env, weights_first[best_1], second, twin_second, weights_second, run_2, best_2, n, CARS, None, tail, frames_2[:8])


# ---- 7. a fit that cannot run ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_fit_that_cannot_run_leaves_the_handle_as_it_was(make_env):
    h, w = SMALLEST
    frames, rows = noisy_set(h, w)
    loaded = loaded_weights(h, w)
    env = fresh(make_env, h, w, loaded)
    ds = env.dataset(*writable(frames, rows), seed=SEED)
    blind, short = env.dataset(*writable(None, rows), seed=SEED), env.dataset(*writable(frames[:20], rows[:20]), seed=SEED)
    assert short.n_train == 16 < CARS
    ways = [(ds, dict(epochs=0), ValueError), (ds, dict(batch_size=CARS + 1), ValueError), (ds, dict(patience=0), ValueError), (blind, {}, RuntimeError),
            (short, {}, ValueError), (ds, dict(augment=dict(mirror=0.5)), TypeError), (ds, dict(convs=("conv3",)), ValueError)]
    for which, kw, error in ways:
        with pytest.raises(error):
            which.fit_tail(**dict(dict(epochs=3, batch_size=CARS, lr=LR), **kw))
        refused_without_a_session(env)
        got = env.pilot_weights()
        assert len(got) == 22 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, loaded)), kw
    check_fit(make_env, case(), env=env, ds=ds)


# ---- 8. resident step mode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_in_resident_mode_a_fit_equals_launch_mode_and_the_worker_steps_again(make_env):
    h, w = SMALLEST
    frames, rows = noisy_set(h, w)
    loaded = loaded_weights(h, w)
    launch, resident = (fresh(make_env, h, w, loaded, auto_reset=True) for _ in range(2))
    resident.set_step_mode(resident=True)
    steer = np.linspace(-1.0, 1.0, CARS, dtype=f32)
    histories = []
    for env in (launch, resident):
        for _ in range(5):
            env.step(steer, 0.7, 0.0)
        ds = env.dataset(*writable(frames, rows), seed=SEED)
        histories.append(ds.fit_tail(2, CARS, lr=LR))
        assert env.counters()[2] == 5
    assert histories[0] == histories[1]
    twin_history, twin_weights = twin_fit(make_env, case(epochs=2))
    run, best = can_tell([v for _, v in twin_history], 2, None, False)
    for env, history in zip((launch, resident), histories):
        compare(make_env, env, loaded, history, twin_history, twin_weights, run, best, RECORDS, CARS, None, trained_arrays(None, None), frames[:8])
    for a, b in zip(launch.pilot_weights(), resident.pilot_weights()):
        assert np.array_equal(bits(a), bits(b))
    for env in (launch, resident):
        env.step_pilot(5)
    for name in STATE + CTL:
        a, b = launch.fetch(name), resident.fetch(name)
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b), name
    assert np.array_equal(launch.fetch("img"), resident.fetch("img"))
    assert resident.step_mode()[0] == "resident" and launch.step_mode()[0] == "launch"
    assert resident.counters()[2] == 10 == launch.counters()[2]                  # five more steps were posted after the fit
    assert np.abs(launch.fetch("ctl_steer")).max() > 0                           # (the trained pilot steered them)
