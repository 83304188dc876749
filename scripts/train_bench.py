#!/usr/bin/env python3
"""Training the pilot's tail (trs_pilot_train_step, include/trsim_spec.h "training the pilot's tail") on one box, at 1024 x 120x160 and 512 x 240x320, the
legs alternating three times inside one run:
  step     trs_pilot_train_step against trs_pilot_forward on the same frames (HIP events on the handle's stream): the difference is what training adds behind
           the forward pass (the forward's own tail kernel, about 6 us, is in trs_pilot_forward and not in the step: it is added back from the trace)
  torch    the step it replaces, on the same GPU: fp32 nn.Linear layers on conv7's features (already there, fp32), mse_loss, backward(), Adam.step()
  copies   plain device copies moving the bytes of the gW1 GEMM (n F 2 read, F 400 written) and of the Adam pass (4 fp32 arrays read, 3 written and the
           binary16 pack): half the total as a torch copy_, which reads and writes it once each.  No pass line: the ratios say what fusing Adam into the
           GEMM's epilogue could save.
With --drive N the script only runs N steps per shape: under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/train_bench.py
--drive 50` that gives the split by kernel, and `python scripts/train_bench.py --stats DIR` prints it.
Pass line: the part behind conv7 (every trs_train_* kernel) is faster than the torch step.
With --convs the session also trains conv4 .. conv7 (trs_pilot_train_convs, "training the pilot's last convolutions") and the torch leg is the step that
replaces: fp32 nn.Conv2d x 4 and the nn.Linear tail on x3 (already there, fp32), mse_loss, backward(), Adam.step().  Pass line: the step's part behind
conv3 is faster than that torch step; the script prints the WHOLE device step (conv1 .. conv3 included) beside it, which bounds that part from above, and
step - forward, what training adds to a forward pass.  --convs combines with --drive for the split by kernel (the data and weight gradients against the
forward chain kernel trs_conv_chain_kernel, about half their arithmetic); the copy leg moves the bytes of the convolutions' Adam pass (4 fp32 arrays read,
3 written, two binary16 copies: 32 bytes per weight).  TRS_BENCH_SHAPE=0 or 1 in the environment runs one of the two shapes alone (a trace per shape).
With --digest the script measures nothing: it prints `name sha256` lines of what three training steps with conv4 .. conv7 leave behind (every debug item of
the tail and of every layer, the masters, and trs_pilot_forward's output afterwards) on seeded weights, frames and labels, at two small shapes that between
them reach one and several chunks and slices of both weight-gradient GEMMs and all three channel shapes.  Two builds of the library (TRS_HIP_LIB) that
compute the same bits print the same lines.
With --dropout RATE the session drops at all four sites behind conv7 (trs_pilot_train_dropout, "training the pilot's tail, dropout"), the step's median is
printed beside its minimum, and a further copy leg moves the bytes of the mask pass over x7 (n F 2 read and written), the one part of dropout that moves
real bytes.  Pass line (profiles/r36_dropout.txt): the step's median with dropout less the median without, on the same box, is at most 1.25 x that copy
plus the spread of the runs without.
With --arch speed_feature the pilot is the 28-array cnn_2d_speed_as_feature ("training the pilot's tail, side branch"): the step is trs_pilot_train_step_ex with
a feature per frame, the forward leg trs_pilot_forward_ex, and the torch leg the step that replaces: the nn.Linear branch 1 -> 4 -> 8 -> 16 on the feature, its
output concatenated behind conv7's features, the nn.Linear tail, mse_loss, backward(), Adam.step().  The medians of the three runs are printed beside the minima.
Pass line: the part behind conv7 is faster than that torch step.
Run from the repository root: python scripts/train_bench.py [--convs] [--dropout RATE] [--arch speed_feature] [> profiles/rNN_train_tail.txt]"""
import csv
import glob
import os
import sys
sys.path.insert(0, ".")
import numpy as np

SHAPES = [(1024, 120, 160, 200), (512, 240, 320, 60)]        # (frames, H, W, calls per timing)
ROUNDS = 3
SPEC = [(5, 2, 3, 24), (5, 2, 24, 32), (5, 2, 32, 64), (3, 1, 64, 64), (3, 1, 64, 64), (3, 1, 64, 128), (3, 1, 128, 128)]


def weights(h, w, seed=0, side=False):
    """22 arrays; side: the 28 of cnn_2d_speed_as_feature (dense1 takes 16 more rows, feature1 .. feature3 follow output_layer)"""
    rng = np.random.default_rng(seed)
    ws, ih, iw = [], h, w
    for k, s, cin, cout in SPEC:
        ws += [(rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32), rng.uniform(-0.05, 0.05, cout).astype(np.float32)]
        ih, iw = (ih - k) // s + 1, (iw - k) // s + 1
    dims = [ih * iw * 128, 100, 50, 25, 2]
    pairs = list(zip([dims[0] + (16 if side else 0)] + dims[1:-1], dims[1:])) + ([(1, 4), (4, 8), (8, 16)] if side else [])
    for a, b in pairs:
        lim = np.sqrt(6.0 / (a + b))
        ws += [rng.uniform(-lim, lim, (a, b)).astype(np.float32), rng.uniform(-0.05, 0.05, b).astype(np.float32)]
    return ws, dims[0]


def stats(directory):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                if "trs_" in name:
                    short = name[name.index("trs_"):]
                    short = short[:short.index("_kernel") + 7] if "_kernel" in short else short.split("(")[0]
                    calls, total = int(r["Calls"]), float(r["TotalDurationNs"])
                    c, t = rows.get(short, (0, 0.0))
                    rows[short] = (c + calls, t + total)
    print("== kernels by name over both shapes (rocprofv3 --kernel-trace --stats): calls, average us ==")
    for name, (c, t) in sorted(rows.items()):
        print(f"  {name:40s} {c:6d} {t / c / 1e3:10.2f}")


# (H, W, n_envs, the batch sizes in turn, three steps each).  93x100: conv7 is one pixel, F = 128 is one gW1 workgroup, every reduction one partial chunk.
# 96x128, 70 frames: a second chunk of 6 frames for gW1; the convolutions' pixels in several slices, the last one short; then 3 frames: one partial chunk.
DIGEST_CASES = [(93, 100, 5, (5,)), (96, 128, 70, (70, 3))]


def digest():
    import hashlib
    import torch
    from triton_racer_sim_amd import _ffi
    from triton_racer_sim_amd.env import BatchedEnv

    def line(name, array):
        print(f"{name} {hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()}", flush=True)

    for case, (h, w, n_envs, batches) in enumerate(DIGEST_CASES, 1):
        ws, _ = weights(h, w)
        env = BatchedEnv(n_envs=n_envs, img_h=h, img_w=w, track=None)
        env.pilot_load(ws)
        env.pilot_train_begin(convs=_ffi.TRAIN_CONV_LAYERS)
        rng = np.random.default_rng(case)
        for n in batches:
            frames = torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()
            labels = torch.from_numpy(rng.uniform(-1, 1, (n, 2)).astype(np.float32)).cuda()
            for _ in range(3):
                env.pilot_train_step(frames, labels)
            tag = f"case{case}.n{n}"
            for item in _ffi.TRAIN_DEBUG:
                if item in ("m", "v"):
                    for a in range(8):
                        line(f"{tag}.tail.{item}{a}", env.pilot_train_debug(item, a))
                else:
                    line(f"{tag}.tail.{item}", env.pilot_train_debug(item))
            for layer in _ffi.TRAIN_CONV_LAYERS:
                for item in _ffi.TRAIN_CONV_DEBUG:
                    line(f"{tag}.{layer}.{item}", env.pilot_train_debug_conv(layer, item))
            for a, master in enumerate(env.pilot_train_weights()[0]):
                line(f"{tag}.tail.master{a}", master)
            for a, master in enumerate(env.pilot_train_conv_weights()):
                line(f"{tag}.conv.master{a}", master)
            out = torch.empty((n, 2), device="cuda")
            assert env.api.pilot_forward(env._h, int(frames.data_ptr()), n, int(out.data_ptr())) == 0
            env.sync()
            line(f"{tag}.forward", out.cpu().numpy())
        env.pilot_train_end()
        env.close()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        return stats(sys.argv[2])
    if "--digest" in sys.argv:
        return digest()
    convs = "--convs" in sys.argv
    if convs:
        sys.argv.remove("--convs")
    dropout = None
    if "--dropout" in sys.argv:
        at = sys.argv.index("--dropout")
        dropout = float(sys.argv[at + 1])
        del sys.argv[at:at + 2]
    side = False
    if "--arch" in sys.argv:
        at = sys.argv.index("--arch")
        if sys.argv[at + 1] not in ("speed_ctl", "speed_feature"):
            sys.exit("--arch takes speed_ctl (22 arrays, the default) or speed_feature (28 arrays)")
        side = sys.argv[at + 1] == "speed_feature"
        del sys.argv[at:at + 2]
    drive = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--drive" else 0
    import torch
    from triton_racer_sim_amd.env import BatchedEnv

    def timed(env, calls, fn):
        env.sync()
        env.event_record(0)
        for _ in range(calls):
            fn()
        env.event_record(1)
        env.sync()
        return env.event_elapsed_ms(0, 1) * 1e3 / calls

    def torch_timed(calls, fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    def show(name, runs):
        print(f"  {name:72s} {min(runs):10.2f} us  (runs: {', '.join(f'{v:.2f}' for v in runs)})", flush=True)

    only = os.environ.get("TRS_BENCH_SHAPE")                            # "0" or "1": one shape alone (the split by kernel under the tracer, per shape)
    for n, h, w, calls in (SHAPES if only is None else [SHAPES[int(only)]]):
        ws, F = weights(h, w, side=side)
        env = BatchedEnv(n_envs=n, img_h=h, img_w=w, track=None)
        env.pilot_load(ws)
        env.pilot_train_begin(convs=("conv4", "conv5", "conv6", "conv7") if convs else None, **({} if dropout is None else {"dropout": dropout}))
        frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        labels = torch.rand((n, 2), device="cuda") * 2 - 1
        out = torch.empty((n, 2), device="cuda")
        torch.cuda.synchronize()
        pf, pl, po = int(frames.data_ptr()), int(labels.data_ptr()), int(out.data_ptr())
        step = lambda: env.api.pilot_train_step(env._h, pf, pl, n, None)
        fwd = lambda: env.api.pilot_forward(env._h, pf, n, po)
        if side:                                                        # a feature per frame: speed / 20 for the step, the speed itself for the forward pass
            speed = torch.rand((n, 1), device="cuda") * 20
            feats = speed / 20
            torch.cuda.synchronize()
            ps, pq = int(speed.data_ptr()), int(feats.data_ptr())
            step = lambda: env.api.pilot_train_step_ex(env._h, pf, pq, pl, n, None)
            fwd = lambda: env.api.pilot_forward_ex(env._h, pf, ps, None, n, po)
        assert step() == 0 and fwd() == 0
        if drive:
            timed(env, drive, step)
            timed(env, drive, fwd)
            env.close()
            continue
        # the torch step on the same features
        x7 = torch.rand((n, F), device="cuda")
        model = torch.nn.Sequential(torch.nn.Linear(F, 100), torch.nn.ReLU(), torch.nn.Linear(100, 50), torch.nn.ReLU(), torch.nn.Linear(50, 25), torch.nn.ReLU(),
                                    torch.nn.Linear(25, 2)).cuda()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-7)
        if side and not convs:                                          # the branch on the feature, concatenated behind conv7's features in front of dense1

            class SideTail(torch.nn.Module):
                def __init__(self):
                    super().__init__()
                    lin, relu = torch.nn.Linear, torch.nn.ReLU
                    self.branch = torch.nn.Sequential(lin(1, 4), relu(), lin(4, 8), relu(), lin(8, 16), relu())
                    self.tail = torch.nn.Sequential(lin(F + 16, 100), relu(), lin(100, 50), relu(), lin(50, 25), relu(), lin(25, 2))

                def forward(self, x):
                    return self.tail(torch.cat([x, self.branch(feats)], 1))

            model = SideTail().cuda()
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-7)

        if convs:                                                       # the torch step from x3 on: conv4 .. conv7 in fp32 NCHW, Keras's Flatten, the tail
            ih, iw = env.conv_input_size(0)
            x7 = torch.rand((n, 64, ih, iw), device="cuda")
            chans, layers = [(64, 64), (64, 64), (64, 128), (128, 128)], []
            for cin, cout in chans:
                layers += [torch.nn.Conv2d(cin, cout, 3), torch.nn.ReLU()]
            model = torch.nn.Sequential(*layers, torch.nn.Flatten(), *list(model.children())).cuda()
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-7)

        def torch_step():
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.mse_loss(model(x7), labels).backward()
            opt.step()

        gemm_bytes, adam_bytes = n * F * 2 + F * 400, int(7.5 * F * 400)
        if convs:
            adam_bytes = 32 * 295296                                    # conv4 .. conv7: 295,296 weights and biases
        src_g, src_a = torch.empty(gemm_bytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(adam_bytes // 2, dtype=torch.uint8, device="cuda")
        dst_g, dst_a = torch.empty_like(src_g), torch.empty_like(src_a)
        src_x = torch.empty(n * F * 2, dtype=torch.uint8, device="cuda")
        dst_x = torch.empty_like(src_x)
        res = {}
        for _ in range(ROUNDS):
            res.setdefault("fwd", []).append(timed(env, calls, fwd))
            res.setdefault("step", []).append(timed(env, calls, step))
            res.setdefault("torch", []).append(torch_timed(calls, torch_step))
            res.setdefault("copy_g", []).append(torch_timed(calls, lambda: dst_g.copy_(src_g)))
            res.setdefault("copy_a", []).append(torch_timed(calls, lambda: dst_a.copy_(src_a)))
            res.setdefault("copy_x", []).append(torch_timed(calls, lambda: dst_x.copy_(src_x)))
        print(f"== {n} frames of {h}x{w}, F = {F}; one MI355X; figures are the minimum of {ROUNDS} alternating runs of {calls} calls ==")
        show("trs_pilot_forward (conv1..7, dense1, the driving tail)", res["fwd"])
        show("trs_pilot_train_step (conv1..7, dense1, tail forward + backward, gW1, Adam)", res["step"])
        show("torch: 4 x nn.Conv2d + 4 x nn.Linear fp32 on x3, mse_loss, backward(), Adam.step()" if convs else
             "torch: 4 x nn.Linear fp32 on conv7's features, mse_loss, backward(), Adam.step()", res["torch"])
        show(f"copy_ of {gemm_bytes // 2 / 1e6:.1f} MB: the gW1 GEMM's {gemm_bytes / 1e6:.1f} MB, read + written", res["copy_g"])
        show(f"copy_ of {adam_bytes // 2 / 1e6:.1f} MB: the Adam pass's {adam_bytes / 1e6:.1f} MB, read + written", res["copy_a"])
        show(f"copy_ of {n * F * 2 / 1e6:.1f} MB: x7's bytes, read + written (what dropout's mask pass moves)", res["copy_x"])
        print(f"  trs_pilot_train_step{'' if dropout is None else f' --dropout {dropout:g}'}: median {sorted(res['step'])[1]:.2f} us, spread {max(res['step']) - min(res['step']):.2f} us; "
              f"copy of x7: median {sorted(res['copy_x'])[1]:.2f} us", flush=True)
        added = min(res["step"]) - min(res["fwd"])
        if convs:
            print(f"  step - forward = {added:.2f} us (what training conv4 .. conv7 and the tail adds to a forward pass); the whole step, conv1 .. conv3 included, "
                  f"against the torch step behind conv3: torch / step = {min(res['torch']) / min(res['step']):.2f} x", flush=True)
        else:
            print(f"  step - forward = {added:.2f} us (the part behind conv7 less the driving tail kernel); torch step / that = {min(res['torch']) / added:.2f} x", flush=True)
        if side:
            med = {k: sorted(v)[1] for k, v in res.items()}
            print(f"  --arch speed_feature, medians: forward {med['fwd']:.2f} us, step {med['step']:.2f} us, step - forward {med['step'] - med['fwd']:.2f} us, "
                  f"torch step {med['torch']:.2f} us; torch step / (step - forward) = {med['torch'] / (med['step'] - med['fwd']):.2f} x", flush=True)
        env.pilot_train_end()
        env.close()


if __name__ == "__main__":
    main()
