"""Training the pilot's last convolutions on the device (include/trsim_spec.h, "training the pilot's last convolutions"; csrc/trsim_train_conv.hip) against
the numpy restatement of tests/test_train_conv_cpu.py.  The reference is computed in binary64, stage by stage, from what the device itself stored: x3 .. x7
(trs_pilot_debug_layer), the binary16 weight copies, the tail's delta1 and s, and for every layer the delta(l) the device handed on.  No ReLU decision can
differ (the masks are the stored activations' own), so no frame is left out.

Bounds are derived, not measured (the functions are the CPU test's, where the reference is shown to notice each mistake at ten times them): a matrix-core
sum of `terms` products that are exact in binary32 errs by at most (terms + 1) 2^-24 sum |terms| in any order (128 for G7, 9 COUT for a data gradient); a value
stored as binary16 under 2^s adds 2^-11 of itself or half a subnormal step; a weight or bias gradient is a running sum of at most per_slice x 64 terms per slice
and the slices added in order: (per_slice 64 + slices + 1) 2^-24 sum |terms|.  The largest |error| / bound per item is printed."""
import ctypes as C
import time

import numpy as np
import pytest

import test_train_conv_cpu as RC
import test_train_cpu as R
from test_pilot_slices import slice_frames
from test_train_gpu import bits, labels_for, tail_weights, worst
from triton_racer_sim_amd import _ffi

f32 = np.float32
LAYERS = _ffi.TRAIN_CONV_LAYERS
ALL, ONLY7, C5C7 = LAYERS, ("conv7",), ("conv5", "conv7")


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class ConvTrainer:
    """A handle with the pilot loaded and a session open that trains `convs`; batches go up through two scratch slots"""

    def __init__(self, make_env, h, w, n_cap, named, convs, **adam):
        self.env = make_env("hip", n_envs=n_cap, img_h=h, img_w=w)
        self.h, self.w, self.convs = h, w, convs
        self.env.pilot_load(named)
        self.env.pilot_train_begin(convs=convs, **adam)
        self.lowest = min(LAYERS.index(c) for c in convs) if convs else 4

    def upload(self, frames, y):
        n = len(frames)
        d_frames = self.env.scratch(20, (n, self.h, self.w, 3), np.uint8)
        d_y = self.env.scratch(21, (n, 2), np.float32)
        self.env.upload(d_frames, frames); self.env.upload(d_y, y)
        return d_frames, d_y

    def step(self, frames, y):
        d_frames, d_y = self.upload(frames, y)
        return self.env.pilot_train_step(d_frames, d_y, len(frames))

    def shape(self, j, n):
        """x(3 + j): j = 0 is x3, the input of conv4"""
        ih, iw = self.env.conv_input_size(j) if j < 4 else tuple(v - 2 for v in self.env.conv_input_size(3))
        return (n, ih, iw, 64 if j < 3 else 128)

    def acts(self, n):
        return [self.env.pilot_layer(2 + j, self.shape(j, n)) for j in range(5)]          # x3 .. x7 as stored

    def conv_state(self):
        e = self.env
        return {nm: {k: e.pilot_train_debug_conv(nm, k).copy() for k in ("gw", "gb", "mw", "vw", "mb", "vb", "pack")} for nm in LAYERS}


def check_conv_step(tr, named_h, n, tag):
    """One step's conv items against the restatement; named_h: {layer: binary16 kernel as float64} the step read.  Returns the gradients {layer: (gW, gb)}."""
    e = tr.env
    x = tr.acts(n)
    d1, s1 = e.pilot_train_debug("delta1").reshape(n, 100), int(e.pilot_train_debug("scale_exp")[0])
    q1 = R.quantise(d1, s1).astype(np.float64)
    w1h = named_h["dense1"]
    ratios, cus = {}, cu_count()
    G = RC.g7(x[4].reshape(n, -1), w1h, q1, s1).reshape(x[4].shape)
    G_abs, terms = RC.g7_abs(w1h, q1, s1).reshape(x[4].shape), 128
    grads = {}
    for j in range(3, tr.lowest - 1, -1):
        nm = LAYERS[j]
        s = int(e.pilot_train_debug_conv(nm, "scale_exp")[0])
        assert s == RC.scale_of(G), (tag, nm, s, RC.scale_of(G))
        delta = e.pilot_train_debug_conv(nm, "delta").reshape(x[j + 1].shape).astype(np.float64)
        ratios[f"delta{j + 4}"] = worst(delta, G, RC.stored_bound(G, G_abs, terms, s))
        q = delta * 2.0 ** s                                              # the binary16 values the kernels below read
        assert np.array_equal(q, q.astype(np.float16).astype(np.float64)) and np.abs(q).max() < 2.0 ** 15
        assert delta.any(), (tag, nm)
        if nm in tr.convs:
            gw, gb = RC.wgrad(x[j], q, s)
            bw, bb = RC.wgrad_bounds(x[j], q, s, cus)
            dev_w = e.pilot_train_debug_conv(nm, "gw").reshape(gw.shape)
            dev_b = e.pilot_train_debug_conv(nm, "gb")
            ratios[f"gW{j + 4}"], ratios[f"gb{j + 4}"] = worst(dev_w, gw, bw), worst(dev_b, gb, bb)
            grads[nm] = (dev_w, dev_b)
        if j > tr.lowest:
            G, G_abs, terms = RC.dgrad(q, named_h[nm], x[j], s), RC.dgrad_abs(q, named_h[nm], x[j], s), 9 * q.shape[3]
    print(f"{tag}: max |error| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)
    return grads


def halves(named):
    h = {nm: np.asarray(named[nm][0], f32).astype(np.float16).astype(np.float64) for nm in LAYERS}
    h["dense1"] = np.asarray(named["dense1"][0], f32).astype(np.float16).astype(np.float64)
    return h


def run_shape(make_env, h, w, batches, convs, seed=3):
    """One handle of max(batches) frames: every batch in turn (a later one reads the weights the earlier left), each checked; out of a step equals
    trs_pilot_forward bit for bit"""
    named, F = tail_weights(h, w, seed=seed)
    frames = slice_frames(h, w, max(batches), seed=1)
    tr = ConvTrainer(make_env, h, w, max(batches), named, convs)
    cur = halves(named)
    for n in batches:
        fwd = tr.env.pilot_forward_host(frames[:n])
        tr.step(frames[:n], labels_for(n, seed=n))
        assert np.array_equal(bits(tr.env.pilot_train_debug("out").reshape(n, 2)), bits(fwd)), (h, w, n)
        check_conv_step(tr, cur, n, f"{h}x{w} n = {n} {'+'.join(convs)}")
        for nm in LAYERS:
            cin, cout = RC.CHANNELS[LAYERS.index(nm)]
            cur[nm] = tr.env.pilot_train_debug_conv(nm, "pack").reshape(3, 3, cin, cout).astype(np.float64)
        cur["dense1"] = tr.env.pilot_train_debug("pack1").reshape(F, 100).astype(np.float64)
    return tr


@pytest.mark.gpu
@pytest.mark.parametrize("convs", [ALL, ONLY7, C5C7], ids=["all", "conv7", "conv5+conv7"])
def test_93x100_conv7_is_one_pixel_and_no_chain_is_planned(make_env, convs):
    run_shape(make_env, 93, 100, (3,), convs)


@pytest.mark.gpu
@pytest.mark.parametrize("convs", [ALL, C5C7], ids=["all", "conv5+conv7"])
def test_96x128_the_chain_runs_and_the_interior_is_materialised(make_env, convs):
    run_shape(make_env, 96, 128, (70, 3), convs)


@pytest.mark.gpu
@pytest.mark.parametrize("convs", [ALL, ONLY7], ids=["all", "conv7"])
def test_120x160_seventy_frames_then_three_on_the_same_handle(make_env, convs):
    run_shape(make_env, 120, 160, (70, 3), convs)


@pytest.mark.gpu
def test_96x128_a_smaller_batch_with_more_slices_than_the_largest(make_env):
    """A handle of 64 frames, a step of 64 and then one of 40: with 256 CUs conv4's 77 x 40 pixels are cut into 49 slices of one chunk, its 77 x 64 into 39 of
    two, so the smaller batch writes 49 x 36,928 partial sums where no layer of the larger writes more than 45 x 36,928 (conv5): the session's buffer holds
    the most slices any n <= n_envs can have (train_conv_max_slices), not the split at n_envs.  Checked like every other step."""
    _, _, s40 = RC.split(40 * 77, cu_count())
    _, _, s64 = RC.split(64 * 77, cu_count())
    print(f"conv4 at 96x128: {s64} slices at n = 64, {s40} at n = 40 ({cu_count()} CUs)")
    run_shape(make_env, 96, 128, (64, 40), ALL)


@pytest.mark.gpu
def test_130x300_a_frame_spans_several_reduction_chunks(make_env):
    run_shape(make_env, 130, 300, (5,), ALL)


@pytest.mark.gpu
def test_chain_against_single_layers(make_env):
    """96x128 and 120x160, chain on: conv7 recomputed by its single-layer kernel from the materialised x6 against the chain's x7.  Bit equality is asserted:
    both accumulate a pixel's 1,152 products over the k-steps in the same order from the same binary16 inputs."""
    for h, w in ((96, 128), (120, 160)):
        named, _ = tail_weights(h, w, seed=3)
        frames = slice_frames(h, w, 6, seed=1)
        env = make_env("hip", n_envs=6, img_h=h, img_w=w)
        env.pilot_load(named)
        env.pilot_forward_host(frames)
        ih, iw = env.conv_input_size(3)
        x7_chain = env.pilot_layer(6, (6, ih - 2, iw - 2, 128))
        single = make_env("hip", n_envs=6, img_h=h, img_w=w)
        single.pilot_tuning(chain_layers=0)
        single.pilot_load(named)
        single.pilot_forward_host(frames)
        x6_mat, x6_single = env.pilot_layer(5, (6, ih, iw, 128)), single.pilot_layer(5, (6, ih, iw, 128))
        assert np.array_equal(bits(x6_mat), bits(x6_single)), (h, w)
        x7_single = single.pilot_layer(6, (6, ih - 2, iw - 2, 128))
        diff = float(np.abs(x7_chain - x7_single).max())
        print(f"{h}x{w}: chain against single layers, max |x7 difference| {diff:.3e}")
        assert np.array_equal(bits(x7_chain), bits(x7_single)), (h, w, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("convs", [ALL, C5C7], ids=["all", "conv5+conv7"])
def test_adam_reproduces_bit_for_bit_and_a_clear_bit_keeps_every_bit(make_env, convs):
    """Steps t = 1, 2, 3 at 120x160: from the gradient the device hands out, the numpy float32 restatement gives m, v and the masters bit for bit; the packed
    binary16 copy is the master rounded (host_f2h's rounding), the bias is where the kernels read it (the reload test); a layer whose bit is clear keeps its
    copy, m and v; two handles agree bit for bit."""
    h, w = 120, 160
    named, F = tail_weights(h, w, seed=3)
    frames = slice_frames(h, w, 48, seed=1)
    tr, twin = (ConvTrainer(make_env, h, w, 16, named, convs, lr=2e-3) for _ in range(2))
    prev = {nm: [np.asarray(named[nm][k], f32).ravel().copy() for k in (0, 1)] for nm in LAYERS}
    mom = {nm: [np.zeros_like(a) for a in prev[nm]] * 2 for nm in LAYERS}           # mw, mb, vw, vb
    for t in (1, 2, 3):
        sl = slice(16 * (t - 1), 16 * t)
        y = labels_for(16, seed=40 + t)
        assert tr.step(frames[sl], y) == twin.step(frames[sl], y)
        st, st2, masters = tr.conv_state(), twin.conv_state(), tr.env.pilot_train_conv_weights()
        for nm in LAYERS:
            j = LAYERS.index(nm)
            for k in st[nm]:
                assert np.array_equal(bits(st[nm][k]), bits(st2[nm][k])), (t, nm, k)   # two runs are bit-identical
            got_w, got_b = masters[2 * j].ravel(), masters[2 * j + 1].ravel()
            if nm in convs:
                assert st[nm]["gw"].any() and st[nm]["gb"].any()
                mw, vw, ww = R.adam(st[nm]["gw"], mom[nm][0], mom[nm][2], prev[nm][0], t, lr=2e-3)
                mb, vb, wb = R.adam(st[nm]["gb"], mom[nm][1], mom[nm][3], prev[nm][1], t, lr=2e-3)
            else:
                (mw, mb, vw, vb), (ww, wb) = mom[nm], prev[nm]
                assert not st[nm]["gw"].any() and not st[nm]["gb"].any()
            for got, ref, what in ((st[nm]["mw"], mw, "mw"), (st[nm]["vw"], vw, "vw"), (st[nm]["mb"], mb, "mb"), (st[nm]["vb"], vb, "vb"), (got_w, ww, "w"), (got_b, wb, "b")):
                assert np.array_equal(bits(got), bits(ref)), (t, nm, what, int((bits(got) != bits(ref)).sum()))
            with np.errstate(over="ignore"):
                assert np.array_equal(bits(st[nm]["pack"]), bits(got_w.astype(np.float16).astype(f32))), (t, nm)
            mom[nm], prev[nm] = [mw, mb, vw, vb], [got_w.copy(), got_b.copy()]
    assert all(np.abs(prev[nm][0] - np.asarray(named[nm][0]).ravel()).max() > 1e-3 for nm in convs)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(120, 160), (93, 100)])
def test_reload_after_three_steps(make_env, h, w):
    """After three steps trs_pilot_forward on the trained handle equals that of a fresh handle given pilot_load(pilot_weights()), bit for bit: every copy
    the forward kernels read (the packed kernels, the biases, the chain's) was written by Adam.  pilot_train_end keeps them."""
    named, F = tail_weights(h, w, seed=3)
    frames = slice_frames(h, w, 24, seed=1)
    tr = ConvTrainer(make_env, h, w, 8, named, ALL, lr=2e-3)
    before = tr.env.pilot_forward_host(frames[:8])
    for t in range(3):
        tr.step(frames[8 * t:8 * t + 8], labels_for(8, seed=70 + t))
    out = tr.env.pilot_forward_host(frames[:8])
    assert np.abs(out - before).max() > 1e-4
    weights = tr.env.pilot_weights()
    assert all(np.array_equal(weights[i], tr.env._pilot_arrays[i]) for i in range(6))
    assert all(np.abs(weights[i] - tr.env._pilot_arrays[i]).max() > 0 for i in range(6, 22))
    fresh = make_env("hip", n_envs=8, img_h=h, img_w=w)
    fresh.pilot_load(weights)
    assert np.array_equal(bits(fresh.pilot_forward_host(frames[:8])), bits(out))
    tr.env.pilot_train_end()
    assert np.array_equal(bits(tr.env.pilot_forward_host(frames[:8])), bits(out))
    assert all(np.array_equal(a, b) for a, b in zip(tr.env.pilot_weights(), weights))


@pytest.mark.gpu
def test_a_session_without_the_call_is_the_tails_alone(make_env):
    """Three steps with convs=None against the unchanged entry points called directly (trs_pilot_train_begin / _step / _get): the same bits, and the
    convolutions keep every bit"""
    h, w = 120, 160
    named, F = tail_weights(h, w, seed=3)
    frames = slice_frames(h, w, 24, seed=1)
    a = ConvTrainer(make_env, h, w, 8, named, None)
    b = make_env("hip", n_envs=8, img_h=h, img_w=w)
    b.pilot_load(named)
    ptrs = (C.c_void_p * 8)(*[x.ctypes.data for x in b._pilot_arrays[14:22]])
    assert b.api.pilot_train_begin(b._h, None, ptrs) == 0
    d_frames, d_y = b.scratch(20, (8, h, w, 3), np.uint8), b.scratch(21, (8, 2), np.float32)
    for t in range(3):
        y = labels_for(8, seed=80 + t)
        a.step(frames[8 * t:8 * t + 8], y)
        b.upload(d_frames, frames[8 * t:8 * t + 8]); b.upload(d_y, y)
        assert b.api.pilot_train_step(b._h, d_frames.__cuda_array_interface__["data"][0], d_y.__cuda_array_interface__["data"][0], 8, None) == 0
    outs = [np.empty_like(x) for x in b._pilot_arrays[14:22]]
    assert b.api.pilot_train_get(b._h, (C.c_void_p * 8)(*[x.ctypes.data for x in outs]), None) == 0
    for x, y_ in zip(a.env.pilot_train_weights()[0], outs):
        assert np.array_equal(bits(x), bits(y_))
    assert np.array_equal(bits(a.env.pilot_forward_host(frames[:8])), bits(b.pilot_forward_host(frames[:8])))
    assert all(np.array_equal(x, y_) for x, y_ in zip(a.env.pilot_weights()[:14], a.env._pilot_arrays[:14]))
    with pytest.raises(RuntimeError, match="trs_pilot_train_convs first"):
        a.env.pilot_train_conv_weights()


@pytest.mark.gpu
def test_refusals_on_the_device(make_env):
    h, w = 93, 100
    named, F = tail_weights(h, w, seed=3)
    env = make_env("hip", n_envs=4, img_h=h, img_w=w)
    api, hd = env.api, env._h
    env.pilot_load(named)
    convs = (C.c_void_p * 8)(*[a.ctypes.data for a in env._pilot_arrays[6:14]])
    only7 = (C.c_void_p * 8)(*([None] * 6 + [a.ctypes.data for a in env._pilot_arrays[12:14]]))
    buf = np.zeros(9 * 128 * 128, f32)

    def refused(rc, code, text):
        assert rc == code, (rc, api.last_error())
        assert text in (api.last_error() or b"").decode(), api.last_error()

    for call in (lambda: api.pilot_train_convs(hd, 0xF, convs), lambda: api.pilot_train_get_convs(hd, convs), lambda: api.pilot_train_debug_conv(hd, 3, 1, buf.ctypes.data, buf.size)):
        refused(call(), -2, "trs_pilot_train_begin first")
    env.pilot_train_begin()
    refused(api.pilot_train_get_convs(hd, convs), -2, "trs_pilot_train_convs first")
    for mask in (0, 0x10, 0x1F):
        refused(api.pilot_train_convs(hd, mask, convs), -1, "conv_mask")
    refused(api.pilot_train_convs(hd, 0xF, None), -1, "NULL")
    refused(api.pilot_train_convs(hd, 0xC, only7), -1, "NULL")
    assert api.pilot_train_convs(hd, 0x8, only7) == 0                       # conv7 alone: the other entries may be NULL
    refused(api.pilot_train_convs(hd, 0x8, only7), -2, "already called")
    refused(api.pilot_train_debug_conv(hd, 3, 1, buf.ctypes.data, buf.size), -2, "no training step yet")
    frames = slice_frames(h, w, 4, seed=1)
    d_frames, d_y = env.scratch(20, (4, h, w, 3), np.uint8), env.scratch(21, (4, 2), np.float32)
    env.upload(d_frames, frames); env.upload(d_y, labels_for(4, 1))
    assert api.pilot_train_step(hd, d_frames.__cuda_array_interface__["data"][0], d_y.__cuda_array_interface__["data"][0], 4, None) == 0
    assert api.pilot_train_debug_conv(hd, 3, 1, buf.ctypes.data, buf.size) == 0 and buf.any()
    refused(api.pilot_train_debug_conv(hd, 4, 1, buf.ctypes.data, buf.size), -1, "layer must be")
    refused(api.pilot_train_debug_conv(hd, 3, 9, buf.ctypes.data, buf.size), -1, "unknown item")
    refused(api.pilot_train_debug_conv(hd, 3, 1, buf.ctypes.data, 5), -1, "size mismatch")
    refused(api.pilot_train_debug_conv(hd, 2, 0, buf.ctypes.data, 4 * 3 * 3 * 128), -1, "lowest trained layer")
    env.pilot_train_end()
    env.pilot_train_begin()
    env.pilot_train_step(d_frames, d_y, 4)
    refused(api.pilot_train_convs(hd, 0xF, convs), -2, "before the session's first step")
    env.pilot_train_end()
    with pytest.raises(ValueError, match="convs must come from"):
        env.pilot_train_begin(convs=("conv3",))


# ---- it learns --------------------------------------------------------------------------------------------------------------------------------
EPOCHS, BATCH = 8, 64
# The device's validation loss after the last epoch against the PyTorch fp32 mirror's, measured once (profiles/r32_train_convs.txt): MIRROR_GAP is the
# relative gap |device - mirror| / mirror found there, and the margin is twice it.
MIRROR_GAP = 0.153                              # device 0.001689 against the mirror's 0.001994 after 8 epochs (both past their best epoch, the 4th: 0.00109 and 0.00108)
MARGIN = 1.0 + 2.0 * MIRROR_GAP


def mirror_fit_convs(ds, ws, epochs, batch):
    """conv4 .. conv7 and the tail in PyTorch fp32 on the same GPU: conv1 .. conv3 frozen in fp32 (x3 is taken once), the same initial weights, the same
    batches in the same order (ds.order), 'mse' and Adam in Keras's form.  Returns the validation loss (mean squared error over [n][2]) before training and
    per epoch."""
    import torch
    import torch.nn.functional as Fn
    from test_pilot import SPEC
    dev = ds.device
    conv_w = lambda i: torch.from_numpy(ws[2 * i]).to(dev).permute(3, 2, 0, 1).contiguous()
    with torch.no_grad():
        feats = []
        for a in range(0, len(ds), 128):
            x = ds.frames[a:a + 128].float().div(255.0).permute(0, 3, 1, 2)
            for i in range(3):
                x = Fn.relu(Fn.conv2d(x, conv_w(i), torch.from_numpy(ws[2 * i + 1]).to(dev), stride=SPEC[i][1]))
            feats.append(x)
        X = torch.cat(feats)
    Y = torch.zeros((len(ds), 2), device=dev)
    for split, count in (("train", ds.n_train), ("val", ds.n_val)):                          # the labels of every record, by the loader's own rule
        for _, _, labels in ds.batches(count, 0, split, layout="nhwc", dtype="uint8"):
            Y[torch.as_tensor(ds.order(split, 0).astype(np.int64), device=dev)] = labels
    P = []
    for i in range(3, 7):
        P += [conv_w(i).requires_grad_(True), torch.from_numpy(ws[2 * i + 1].copy()).to(dev).requires_grad_(True)]
    P += [torch.from_numpy(ws[14 + j].copy()).to(dev).requires_grad_(True) for j in range(8)]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]

    def model(x):
        for i in range(4):
            x = Fn.relu(Fn.conv2d(x, P[2 * i], P[2 * i + 1]))
        z = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)                                    # Keras's Flatten on NHWC
        for j in range(4):
            z = z @ P[8 + 2 * j] + P[9 + 2 * j]
            z = Fn.relu(z) if j < 3 else z
        return z

    val_idx = torch.as_tensor(ds.order("val", 0)[:ds.n_val // batch * batch].astype(np.int64), device=dev)

    def val_loss():
        with torch.no_grad():
            return float(((model(X[val_idx]).double() - Y[val_idx].double()) ** 2).mean().item())

    curve, t = [val_loss()], 0
    for epoch in range(epochs):
        order = torch.as_tensor(ds.order("train", epoch).astype(np.int64), device=dev)
        for b in range(ds.n_train // batch):
            idx = order[b * batch:(b + 1) * batch]
            loss = ((model(X[idx]) - Y[idx]) ** 2).sum() / (2 * batch)
            grads = torch.autograd.grad(loss, P)
            t += 1
            alpha = float(R.alpha_t(1e-3, 0.9, 0.999, t))
            with torch.no_grad():
                for p, g, m, v in zip(P, grads, M, V):
                    m.mul_(0.9).add_(g, alpha=1.0 - 0.9)
                    v.mul_(0.999).addcmul_(g, g, value=1.0 - 0.999)
                    p.sub_(alpha * m / (v.sqrt() + 1e-7))
        curve.append(val_loss())
    return curve


@pytest.mark.gpu
def test_it_learns_with_the_last_convolutions(make_env):
    """64 cars, the scripted expert, collect(ticks=120, every=5, skip=20): 1,280 records, 16 training batches of 64 per epoch.  fit_tail(convs=conv4 .. conv7)
    for EPOCHS epochs from the fixture pilot with its dense layers drawn again, against the PyTorch fp32 mirror that trains the same layers."""
    from test_train_gpu import redrawn_fixture
    t0 = time.perf_counter()
    ws = redrawn_fixture()
    env = make_env("hip", n_envs=64, img_h=120, img_w=160, auto_reset=True)
    env.set_expert()
    frames, rows = env.collect(ticks=120, every=5, skip=20)
    ds = env.dataset(frames, rows, loader="speed_ctl", seed=7)
    assert len(ds) == 1280 and ds.n_train == 1024 and ds.n_val == 256
    env.pilot_load(ws)
    first = ds.pilot_loss("val", BATCH)
    history = ds.fit_tail(EPOCHS, BATCH, convs=ALL)
    assert len(history) == EPOCHS
    last = history[-1][1]
    kept = ds.pilot_loss("val", BATCH)                                   # the best epoch's weights, convolutions included, are in the handle
    assert kept == min(v for _, v in history)
    assert all(np.abs(a - b).max() > 0 for a, b in zip(env.pilot_weights()[6:14], ws[6:14]))
    mirror = mirror_fit_convs(ds, ws, EPOCHS, BATCH)
    gap = abs(last - mirror[-1]) / mirror[-1]
    print(f"device: val loss {first:.6f} -> {last:.6f} (best {kept:.6f}), train losses {[round(a, 5) for a, _ in history]}, val {[round(v, 5) for _, v in history]}")
    print(f"mirror: val loss {mirror[0]:.6f} -> {mirror[-1]:.6f}, per epoch {[round(v, 5) for v in mirror[1:]]}; relative gap of the final losses {gap:.2e}; "
          f"{time.perf_counter() - t0:.2f} s")
    assert abs(first - mirror[0]) <= 1e-3 * mirror[0]                    # the same start
    assert mirror[-1] < 0.25 * mirror[0]                                 # the mirror itself falls below a quarter of its start
    assert last < 0.5 * first
    assert last <= mirror[-1] * MARGIN, (last, mirror[-1], MARGIN)
