"""trs_conv_lt_kernel (csrc/trsim_pilot_layers.hpp, the quad-load kernel: the pilot's one generic fallback) and the default plans of large frames, which reach
it without any tuning.  The checker is the PyTorch mirror of tests/test_pilot.py, layer by layer on the kernel's OWN previous activation, with that file's two rules
unchanged: per element |got - want| <= 2^-10 |want| + 2e-4 (one fp16 ulp + the floor for sums that cancel), and fewer than 2 % of the elements differ by more than 1e-6
(dense1's mirror sums K in float64 here: mirror_layer).

FALLBACK turns every fused and frame kernel and the span kernel off: conv1 runs on trs_conv_u8_kernel, conv2 on trs_conv_lt_kernel<1>, conv3..conv7 on <2>, and
every activation is stored, so pilot_layer(i) reads what the kernel wrote.  Every test first asserts through the planner that the layers it checks are served by the
kernel it names.  The edges of the kernel, window_base and store_tile_at, and where they are reached:
  1. a ragged last tile (M = n OH OW no multiple of 32: the loader's clamp, the epilogue's m_limit): most layers of every case, e.g. conv7 of A with M = 36, 180, 45 and 37
  2. a tile that spans many frames (window_base's wrap loop and its division by OW): 96x100, where conv7 has one pixel a frame (a tile is 32 frames, OW = 1)
     and conv6 nine (OW = 3); 100x132, where conv7 has five
  3. two channel slices (blockIdx.y = 1, cbase = 64): conv6 and conv7 in every case; conv7 on 7 waves in 162,624 bytes of LDS
  4. <1> with kernel rows of 15 granules padded to 16: the sixteenth load of a row reads the next pixel's 16 bytes against zero weights.  A frame is a multiple
     of 4 wide (trs_create), so conv1's width W / 2 - 2 is even, conv2's windows end one column short of it, and for conv2's last column that pixel is the spare
     last column of the same row (tests/test_pilot_plan_cpu.py pins it): no legal frame size makes the load cross a row, a frame or in_bytes.  What a larger
     earlier batch left behind in_bytes must still not reach a sum: B
  5. the persistent loop (more tiles than resident waves: tile += stride, the next tile's first trips requested before the epilogue): C
  6. K of 80, 100, 72 and 144 granules against the ring of 4 kConvPrefetch: every case
A's comparison of the two plans found a defect outside the fallback: conv7 one pixel wide (frames 96 and 100 wide) on the chain and the frame kernel, whose
division by OW has no 32-bit factor for 1.  The plan now keeps such a layer on the quad-load kernel: test_conv7_one_pixel_wide_on_the_default_plan.
The nt_out store policies (activations above 128 MB) are not tested: no activation a check reads here is that large.  (C's conv3 case does push conv1's
activation, 172 MB on trs_conv_u8_kernel, over that line; only conv3 is compared there.)  Measured figures: profiles/r27_pilot_fallback.txt."""
import numpy as np
import pytest

from test_pilot import SPEC, make_weights, planner, served, torch_layer, torch_pure, torch_tail     # noqa: F401  (planner is a fixture)
from test_pilot_plan_cpu import FALLBACK, persistent_batch, tiles_and_waves

pytestmark = pytest.mark.gpu

ON_THE_FALLBACK = ["u8", "lt<1>", "lt<2>", "lt<2>", "lt<2>", "lt<2>", "lt<2>"]


def shapes_of(h, w, n):
    """the activations of conv1..conv7 and dense1 for n frames"""
    shapes = []
    for k, s, _, cout in SPEC:
        h, w = (h - k) // s + 1, (w - k) // s + 1
        shapes.append((n, h, w, cout))
    return shapes + [(n, 100)]


def noise_and_white(rng, n, h, w):
    """A white frame in front of n - 1 noise frames (the last tile, the ragged one, holds noise); a single frame is noise with a white lower half."""
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if n > 1:
        frames[0] = 255
    else:
        frames[0, h // 2:] = 255
    return frames


def mirror_layer(layer, x, ws):
    """tests/test_pilot.py's mirror of layer 0..7 on the activation x.  dense1 (layer 7) is the same arithmetic - fp16-rounded weights, fp32 bias, ReLU, an fp32
    result - with the K sum in float64: at K = 432,768 (480x640) torch's fp32 matrix product on the CPU lay up to 2.1e-6 from the float64 sum
    of the same products (4 of 200 outputs beyond 1e-6; 1.3e-6 at 360x480, 5.7e-7 at 240x320), the kernel 7.4e-8 - the "elements that differ" were the
    reference's, not the kernel's (profiles/r27_pilot_fallback.txt).  The convolutions' K is 1,152 at most: torch_layer as it is."""
    if layer < 7:
        return torch_layer(layer, x, ws)
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).reshape(x.shape[0], -1).double()
    z = flat @ torch.from_numpy(ws[14]).half().double() + torch.from_numpy(ws[15]).double()
    return torch.relu(z).float().numpy()


def check_against_mirror(where, layer, got, want):
    """test_forward_matches_torch_fp32's two rules; the figures are printed first"""
    diff = np.abs(got - want)
    ratio = float((diff / (2.0 ** -10 * np.abs(want) + 2e-4)).max())
    share = float(np.mean(diff > 1e-6))
    print(f"{where} layer {layer}: worst |got - want| / (2^-10 |want| + 2e-4) = {ratio:.3f}, {100 * share:.3f} % of {diff.size} elements differ, "
          f"max |got - want| {float(diff.max()):.2e}, max want {float(want.max()):.3f}")
    assert want.max() > 0, (where, layer)
    assert (diff <= 2.0 ** -10 * np.abs(want) + 2e-4).all(), f"{where} layer {layer}: worst {float(diff.max())}, {ratio:.2f} x the bound"
    assert share < 0.02, f"{where} layer {layer}: {100 * share:.2f}% of the elements differ"


def layers_against_mirror(where, env, frames, ws, layers=range(8)):
    """pilot_layer(i) against the mirror's layer i on pilot_layer(i - 1), for every i; the kernel's dense1 activation comes back"""
    shapes = shapes_of(frames.shape[1], frames.shape[2], frames.shape[0])
    x = frames
    for layer in layers:
        got = env.pilot_layer(layer, shapes[layer])
        check_against_mirror(where, layer, got, mirror_layer(layer, x, ws))
        x = got
    return x


@pytest.mark.parametrize("size,n", [((120, 160), 1), ((120, 160), 5), ((100, 132), 9), ((96, 100), 37)])
def test_every_layer_on_the_fallback_matches_the_mirror(make_env, planner, size, n):
    """A.  One frame of 120x160: conv7 has M = 36, its second tile holds 4 pixels.  100x132: a frame row of 396 bytes, conv7 with 5 pixels a frame.  37 frames of
    96x100: conv7's tile 0 spans 32 frames and tile 1 holds 5 pixels, conv6 has OW = 3.  End to end the outputs lie within 4e-4 of fp32 PyTorch at 120x160
    (profiles/r03_pilot_precision.txt; printed at the other sizes), within 2e-3 of the default plan's on the same frames (two summation orders end to end, as in
    test_fused_head_equals_the_two_layers), and a second pass returns the same bits."""
    h, w = size
    where = f"A {h}x{w} n={n}"
    plan, default_plan = planner.plan(h, w, n, **FALLBACK), planner.plan(h, w, n)
    assert served(plan) == ON_THE_FALLBACK and plan["head"]["runs"] == 0 and plan["chain"]["first"] == -1
    assert not any(k.startswith("lt") for k in served(default_plan)[:6])          # the other run is one on other kernels (conv7, one pixel wide at 96x100, aside)
    l6 = plan["layers"][5], plan["layers"][6]
    assert [(l["res_nb"], l["res_ysplit"]) for l in l6] == [(2, 2), (2, 2)] and (l6[1]["res_block"], l6[1]["res_lds"]) == (448, 162624)
    ws = make_weights(h, w, seed=3)
    frames = noise_and_white(np.random.default_rng(17), n, h, w)
    env = make_env("hip", n_envs=n, img_h=h, img_w=w)
    env.pilot_tuning(**FALLBACK)
    env.pilot_load(ws)
    out = env.pilot_forward_host(frames)
    h1 = layers_against_mirror(where, env, frames, ws)
    assert np.max(np.abs(out - torch_tail(h1, ws))) <= 1e-4          # fp32 tail on identical inputs
    assert np.array_equal(env.pilot_forward_host(frames), out)
    assert env.pilot_range_check().sum() == 0
    pure = torch_pure(frames, ws)
    print(f"{where}: max |fallback - fp32 torch| = {float(np.abs(out - pure).max()):.3e}")
    if size == (120, 160):
        assert np.max(np.abs(out - pure)) <= 4e-4, float(np.max(np.abs(out - pure)))
    other = make_env("hip", n_envs=n, img_h=h, img_w=w)
    other.pilot_load(ws)
    out_default = other.pilot_forward_host(frames)
    print(f"{where}: max |fallback - default plan| = {float(np.abs(out - out_default).max()):.3e}")
    assert np.max(np.abs(out - out_default)) <= 2e-3
    assert n == 1 or np.std(out[:, 0]) > 1e-5


def test_a_smaller_batch_after_a_larger_one(make_env, planner):
    """B.  A handle of 9 frames of 100x132 forwards 9, then the first 3: behind in_bytes its activations still hold frames 3..8 of the pass before.  A handle of 3
    that never saw those gives the same bits, in the outputs and in conv2 (on <1>, whose padding granule reads a neighbouring pixel), conv3 and conv7.  Bit equality
    of two runs cannot see an error both make: conv2 of the run after the larger batch is also held against the mirror."""
    h, w = 100, 132
    for n_cap in (9, 3):
        plan = planner.plan(h, w, n_cap, **FALLBACK)
        assert served(plan) == ON_THE_FALLBACK and plan["head"]["runs"] == 0
        assert (plan["layers"][1]["run_pad"], plan["layers"][1]["IW"]) == (16, 64)
    ws = make_weights(h, w, seed=7)
    frames = np.random.default_rng(19).integers(0, 256, (9, h, w, 3), dtype=np.uint8)
    shapes = shapes_of(h, w, 3)
    res = []
    for n_cap in (9, 3):
        env = make_env("hip", n_envs=n_cap, img_h=h, img_w=w)
        env.pilot_tuning(**FALLBACK)
        env.pilot_load(ws)
        if n_cap == 9:
            env.pilot_forward_host(frames)
        out = env.pilot_forward_host(frames[:3])
        res.append([out] + [env.pilot_layer(i, shapes[i]) for i in (1, 2, 6)])
        if n_cap == 9:
            check_against_mirror(f"B {h}x{w}", 1, res[0][1], torch_layer(1, env.pilot_layer(0, shapes[0]), ws))
    for a, b in zip(*res):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.std(res[0][0][:, 0]) > 1e-5


@pytest.mark.parametrize("layer,kernel", [(1, "lt<1>"), (2, "lt<2>")])
def test_more_tiles_than_resident_waves(make_env, planner, layer, kernel):
    """C.  96x100 under FALLBACK, the smallest odd batch at which the layer's launch has more 32-pixel tiles than waves (asserted from the plan): on 256 CUs 267
    frames for conv2 (462 pixels a frame; 3,855 tiles on 768 workgroups of 5 waves) and 1,619 for conv3 (81 pixels a frame; 4,099 tiles on 256 workgroups of 16
    waves - conv4 and conv5 would need 2,675 and 5,243 frames for the same launch shape, so conv3 is the cheapest).  The first waves take a second tile; the last
    tile is ragged.  Only this layer is compared, with the mirror fed the kernel's own input."""
    h, w = 96, 100
    n = persistent_batch(planner.plan(h, w, 1, **FALLBACK), layer, planner.cus)
    plan = planner.plan(h, w, n, **FALLBACK)
    assert served(plan) == ON_THE_FALLBACK and served(plan)[layer] == kernel
    tiles, waves = tiles_and_waves(plan, planner.call(h, w, n, n, **FALLBACK), layer, n)
    px = plan["layers"][layer]["OH"] * plan["layers"][layer]["OW"]
    print(f"C conv{layer + 1} on {kernel}: n = {n}, {tiles} tiles on {waves} waves ({planner.cus} CUs), last tile {n * px % 32} pixels")
    assert tiles > waves and n * px % 32 != 0 and n % 2 == 1
    ws = make_weights(h, w, seed=11)
    frames = noise_and_white(np.random.default_rng(23), n, h, w)
    env = make_env("hip", n_envs=n, img_h=h, img_w=w)
    env.pilot_tuning(**FALLBACK)
    env.pilot_load(ws)
    out = env.pilot_forward_host(frames)
    shapes = shapes_of(h, w, n)
    check_against_mirror(f"C n={n}", layer, env.pilot_layer(layer, shapes[layer]), torch_layer(layer, env.pilot_layer(layer - 1, shapes[layer - 1]), ws))
    assert np.isfinite(out).all() and np.std(out[:, 0]) > 1e-5


@pytest.mark.parametrize("size,n", [((360, 480), 3), ((480, 640), 2)])
def test_large_frames_on_the_default_plan(make_env, planner, size, n):
    """D.  No tuning.  360x480: the head cut in 3 parts, conv3 in 14 bands, conv7 on trs_conv_lt_kernel<2>; 480x640: 4 parts, 29 bands of 2 rows, conv4..conv7 on
    <2> - the first GPU run of each of these.  Every layer against the mirror (layer 0 behind the fused head is trs_conv_u8_kernel's; the failing layer says which
    kernel is wrong).  No end-to-end bound has been measured at these sizes: the difference to fp32 PyTorch is printed and must be finite."""
    h, w = size
    where = f"D {h}x{w} n={n}"
    plan = planner.plan(h, w, n)
    big = size == (480, 640)
    assert (plan["head"]["runs"], plan["head"]["wsplit"], plan["layers"][2]["frame5_bands"]) == (1, 4 if big else 3, 29 if big else 14)
    assert served(plan) == ["band<split>", "band<split>", "frame5"] + (["lt<2>"] * 4 if big else ["frame"] * 3 + ["lt<2>"])
    ws = make_weights(h, w, seed=3)
    frames = noise_and_white(np.random.default_rng(29), n, h, w)
    env = make_env("hip", n_envs=n, img_h=h, img_w=w)
    env.pilot_load(ws)
    out = env.pilot_forward_host(frames)
    h1 = layers_against_mirror(where, env, frames, ws)
    assert np.max(np.abs(out - torch_tail(h1, ws))) <= 1e-4
    diff = float(np.abs(out - torch_pure(frames, ws)).max())
    print(f"{where}: max |HIP - fp32 torch| = {diff:.3e} (outputs {out[0]})")
    assert np.isfinite(out).all() and np.isfinite(diff)
    assert env.pilot_range_check().sum() == 0
    assert np.std(out[:, 0]) > 1e-5 and not np.array_equal(out[0], out[1])


@pytest.mark.parametrize("size,n", [((96, 100), 37), ((120, 100), 5)])
def test_conv7_one_pixel_wide_on_the_default_plan(make_env, planner, size, n):
    """Frames 96 and 100 wide leave conv7 one pixel wide (and, 96 high, one pixel in all).  The kernels that keep frames in LDS divide a pixel index by OW with a
    32-bit factor that does not exist for 1: until A's comparison of the two plans at 96x100 showed it, the chain computed conv7 of the second frame of every
    workgroup from the first frame's window (outputs off by 1e-2), and the frame kernel would have read a 4 x 1 output's rows as columns.  The default plan now
    serves such a layer on trs_conv_lt_kernel<2> (asserted); every layer is held against the mirror, and the outputs against fp32 PyTorch within the 4e-4 of
    test_forward_matches_torch_fp32."""
    h, w = size
    where = f"F {h}x{w} n={n}"
    plan = planner.plan(h, w, n)
    assert plan["layers"][6]["OW"] == 1 and served(plan)[2:] == ["frame5", "frame", "frame", "frame", "lt<2>"] and plan["chain"]["first"] == -1
    ws = make_weights(h, w, seed=3)
    frames = noise_and_white(np.random.default_rng(31), n, h, w)
    env = make_env("hip", n_envs=n, img_h=h, img_w=w)
    env.pilot_load(ws)
    out = env.pilot_forward_host(frames)
    h1 = layers_against_mirror(where, env, frames, ws)
    assert np.max(np.abs(out - torch_tail(h1, ws))) <= 1e-4
    diff = float(np.abs(out - torch_pure(frames, ws)).max())
    print(f"{where}: max |HIP - fp32 torch| = {diff:.3e}")
    assert diff <= 4e-4
    assert np.std(out[:, 0]) > 1e-5
