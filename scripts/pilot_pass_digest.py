#!/usr/bin/env python3
"""Do two builds of the library compute the same pilot?  (One MI355X, seconds.)

    python scripts/pilot_pass_digest.py <libtrsim A> <libtrsim B>     both in a fresh process each (TRS_HIP_LIB), then the comparison
    python scripts/pilot_pass_digest.py                               the lines of the library in use

For every case — frame size, batch, 22 or 42 weight arrays, tuning — on seeded weights and frames the script prints `name sha256` of the raw outputs of a
forward pass, of all eight pilot_layer arrays read in descending and then in ascending order (the first read of conv6 materialises the chain's interior,
the last of the descending ones conv1 behind the fused head; the ascending reads find them valid), and of the controls after 20 step_pilot ticks.  The cases:
93x100 with 5 frames (the fallback kernels), 96x128 with 37, 120x160 with 64 (a chain whose interior is materialised) and with no_fuse / without the chain,
240x320 with 8.  Two builds whose kernels are the same code (scripts/kernel_diff.py) and whose host side launches them alike print the same lines: the
kernels use no floating-point atomics."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(93, 100, 5, {}), (96, 128, 37, {}), (120, 160, 64, {}), (240, 320, 8, {}), (120, 160, 64, {"no_fuse": 1}), (120, 160, 64, {"chain_layers": 0})]


def digest():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from test_pilot import SPEC, make_weights
    from test_pilot_types import make_named_weights
    from triton_racer_sim_amd.env import BatchedEnv

    def line(name, array):
        print(f"{name} {hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()}", flush=True)

    for h, w, n, tuning in CASES:
        for arrays in (22, 42):
            tag = f"{h}x{w}.n{n}.a{arrays}" + "".join(f".{k}{v}" for k, v in tuning.items())
            kind = "cnn_2d_speed_control" if arrays == 22 else "cnn_2d_full_house"
            env = BatchedEnv(n_envs=n, img_h=h, img_w=w, auto_reset=True)
            if tuning:
                env.pilot_tuning(**tuning)
            env.pilot_load(make_weights(h, w, seed=3) if arrays == 22 else make_named_weights(h, w, kind, seed=3)[0])
            rng = np.random.default_rng(h * w + n)
            frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
            side = {} if arrays == 22 else {"speed": rng.uniform(0, 20, n).astype(np.float32), "segment": rng.uniform(0, 1, n).astype(np.float32)}
            line(f"{tag}.raw", env.pilot_forward_host(frames, **side))
            shapes, ih, iw = [], h, w
            for k, s, _, cout in SPEC:
                ih, iw = (ih - k) // s + 1, (iw - k) // s + 1
                shapes.append((n, ih, iw, cout))
            shapes.append((n, 100))
            for order, layers in (("down", range(7, -1, -1)), ("up", range(8))):
                for i in layers:
                    line(f"{tag}.{order}.layer{i}", env.pilot_layer(i, shapes[i]))
            env.step_synthetic(2, 1)
            env.step_pilot(20, {"model_type": kind})
            env.sync()
            for name in ("ctl_steer", "ctl_thr", "ctl_brk"):
                line(f"{tag}.loop.{name}", env.fetch(name))
            env.close()


def main():
    if len(sys.argv) < 3:
        return digest()
    runs = []
    for lib in sys.argv[1:3]:
        out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, TRS_HIP_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=600)
        if out.returncode:
            sys.exit(f"{lib}: exit {out.returncode}\n{out.stderr[-3000:]}")
        runs.append(dict(l.split() for l in out.stdout.splitlines() if len(l.split()) == 2))
    a, b = runs
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in sorted(a):
        print(f"{'equal    ' if k not in differ else 'DIFFERENT'} {k} {a[k]}" + ("" if k not in differ else f" | {b.get(k)}"))
    print(f"{len(a)} digests of {sys.argv[1]}, {len(b)} of {sys.argv[2]}: {len(differ)} differ")
    return 1 if differ or not a else 0


if __name__ == "__main__":
    sys.exit(main())
