"""Image path, the parts the single-batch tests leave alone: hysteresis that really propagates, workgroups that take a second and a
third frame, the frame sizes that select the other chunking / scratch / two-pass code, the normalize kernel's stride loop.

The CPU tests pin the oracle's Canny to an independent whole-array numpy statement of the algorithm in the header comment of
canny_u8c3 (cv2 is absent).  The GPU tests compare the HIP kernels with the oracle, bit for bit, on inputs whose properties (weak pixels
promoted and left alone, sweeps needed, frames per workgroup) are asserted from the numpy reference and the queried CU count first."""
import functools

import numpy as np
import pytest

from test_image_path import EDGE, numpy_trim

# ---- reference -----------------------------------------------------------------------------------------------------------------


def _dilate8(m):
    """8-neighbour dilation of a boolean image (the pixel itself included)."""
    p = np.pad(m, 1)
    h, w = m.shape
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def np_canny(img, a, b):
    """cv2.Canny(img, a, b) on uint8[H,W,3], aperture 3, L1 norm, as the header comment of the oracle's canny_u8c3 states it.
    Returns (edge uint8[H,W] in {0,255}, nms int8[H,W] with 0 = weak / 1 = none / 2 = strong, rounds of dilation that changed a pixel)."""
    low, high = min(a, b), max(a, b)
    p = np.pad(img.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")                  # replicated borders
    tl, tc, tr = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    ml, mr = p[1:-1, :-2], p[1:-1, 2:]
    bl, bc, br = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    dx3 = (tr + 2 * mr + br) - (tl + 2 * ml + bl)
    dy3 = (bl + 2 * bc + br) - (tl + 2 * tc + tr)
    ch = np.argmax(np.abs(dx3) + np.abs(dy3), axis=2)[..., None]                             # the first channel that reaches the maximum
    xs, ys = np.take_along_axis(dx3, ch, 2)[..., 0], np.take_along_axis(dy3, ch, 2)[..., 0]
    m = np.abs(xs) + np.abs(ys)
    mp = np.pad(m, 1)                                                                        # magnitudes outside the image are 0
    h, w = m.shape
    nb = lambda dy, dx: mp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ax, ay = np.abs(xs), np.abs(ys) << 15
    tg22 = ax * 13573                                                                        # tan 22.5 deg in 2^-15
    tg67 = tg22 + (ax << 16)
    horizontal, vertical = ay < tg22, (ay >= tg22) & (ay > tg67)
    same_sign = (xs ^ ys) >= 0
    is_max = np.where(horizontal, (m > nb(0, -1)) & (m >= nb(0, 1)),
                      np.where(vertical, (m > nb(-1, 0)) & (m >= nb(1, 0)),
                               np.where(same_sign, (m > nb(-1, -1)) & (m > nb(1, 1)), (m > nb(-1, 1)) & (m > nb(1, -1)))))
    is_max &= m > low
    nms = np.where(is_max, np.where(m > high, 2, 0), 1).astype(np.int8)
    weak, edge, rounds = nms == 0, nms == 2, 0
    front = edge
    while True:                                                                              # hysteresis: fixed point of the dilation restricted to weak pixels
        front = _dilate8(front) & weak & ~edge                                               # (only the pixels added last can reach new ones)
        if not front.any():
            break
        edge, rounds = edge | front, rounds + 1
    return (edge * np.uint8(255)).astype(np.uint8), nms, rounds


def canny_stats(img, a, b):
    """(promoted, weak left unpromoted, rounds) of one frame, from the reference alone."""
    edge, nms, rounds = np_canny(img, a, b)
    weak = nms == 0
    return int((weak & (edge == 255)).sum()), int((weak & (edge == 0)).sum()), rounds


# ---- inputs ----------------------------------------------------------------------------------------------------------------------


def _box(a, axis, r=3):
    """Box blur of radius r along one axis by cumulative sums, borders replicated."""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r + 1, r)
    c = np.cumsum(np.pad(a, pad, mode="edge"), axis=axis)
    n = a.shape[axis]
    hi = np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis)
    lo = np.take(c, np.arange(0, n), axis=axis)
    return (hi - lo) / (2 * r + 1)


def smooth_frames(n, h, w, seed):
    """Blurred Gaussian noise, std 60 around 128: gradients spread over the whole range of the thresholds, long weak ridges."""
    a = np.random.default_rng(seed).standard_normal((n, h, w, 3))
    for _ in range(3):
        a = _box(_box(a, 1), 2)
    a = a / a.std() * 60.0 + 128.0
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def snake_steps(lo, hi):
    """Grey steps for the thresholds lo < hi: an edge of step `weak` has magnitude 4 weak in (lo, hi], one of step `strong` lies above hi."""
    weak, strong = lo // 4 + 1, hi // 4 + 15
    assert lo < 4 * weak <= hi and 4 * strong > hi and weak < strong <= 255, (lo, hi)
    return weak, strong


def snake(h, w, lo, hi, cut=False):
    """One serpentine of 6-pixel bars on black whose whole outline is a weak edge, seeded by 8 strong rows at the far end of the last bar:
    hysteresis has to walk the outline, bar by bar.  cut: a few black rows across the middle bar - the outline beyond stays unpromoted."""
    weak, strong = snake_steps(lo, hi)
    img = np.zeros((h, w), np.uint8)
    top, bot = min(3, h // 4), h - min(3, h // 4)
    xs = list(range(3, w - 8, 12))
    for k, x in enumerate(xs):
        img[top:bot, x:x + 6] = weak
        if k + 1 < len(xs):                                                                  # joined alternately at the bottom and at the top
            rows = slice(max(top, bot - 6), bot) if k % 2 == 0 else slice(top, min(bot, top + 6))
            img[rows, x:x + 18] = weak
    if xs:
        far = slice(top, min(bot, top + 8)) if len(xs) % 2 == 0 else slice(max(top, bot - 8), bot)   # the free end of the last bar
        img[far, xs[-1]:xs[-1] + 6] = strong
        if cut:
            x = xs[len(xs) // 2]
            img[h // 2 - 2:h // 2 + 2, x - 1:x + 7] = 0
    return np.repeat(img[..., None], 3, axis=2)


PAIRS = [(60, 100), (100, 60), (200, 400), (150, 150), (-5, 50), (3000, 5000)]
DESIGN = (200, 400)          # the pair the pool is made for: the smooth frames are weak-rich there, and the snake takes its steps from it
BLACK, WHITE, NOISE, SNAKE, CUT, SMOOTH0 = 0, 1, 2, 3, 4, 5
N_SMOOTH = 4


@functools.lru_cache(maxsize=None)
def pool(h, w, pair=DESIGN):
    """[black, 255, noise, snake, cut snake, smooth x 4] for the thresholds `pair` (read-only)."""
    lo, hi = min(pair), max(pair)
    out = np.empty((SMOOTH0 + N_SMOOTH, h, w, 3), np.uint8)
    out[BLACK], out[WHITE] = 0, 255
    out[NOISE] = np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out[SNAKE], out[CUT] = snake(h, w, lo, hi), snake(h, w, lo, hi, cut=True)
    out[SMOOTH0:] = smooth_frames(N_SMOOTH, h, w, seed=2)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pool_stats(h, w, pair=DESIGN):
    return [canny_stats(f, *pair) for f in pool(h, w, pair)]


def check_pool(h, w, pair=DESIGN):
    """The input conditions, from np_canny alone: without them a comparison of edge maps says little about hysteresis."""
    st = pool_stats(h, w, pair)
    assert st[BLACK][:2] == (0, 0) and st[WHITE][:2] == (0, 0)                               # no weak pixel at all
    if h * w >= 64 * 64:
        promoted, left, rounds = st[SNAKE]
        assert rounds >= (700 if h * w >= 120 * 160 else 100), (h, w, st[SNAKE])
        assert left == 0 and promoted >= rounds                                              # the whole outline hangs on the seed
        assert st[CUT][1] >= 50 and st[CUT][0] >= 50, (h, w, st[CUT])                        # beyond the cut: weak, never promoted
    if h * w >= 120 * 160:
        assert any(p >= 200 and l >= 1000 and r >= 10 for p, l, r in st[SMOOTH0:]), (h, w, st)
    return st


def trimmed(img, cfg):
    """numpy_trim; a frame without brightness rows (H <= 40) has channel means 0 (the oracle's convention for the empty img[40:119])."""
    if img.shape[0] > 40:
        return numpy_trim(img, cfg)
    a = img.astype(np.float32)
    if cfg.get("preprocessing_dynamic_brightness_enabled", False):
        a += (cfg.get("preprocessing_brightness_baseline", 550) - 0.0) / 3
    a -= cfg.get("preprocessing_contrast_enhancement_offset", 125)
    a *= cfg.get("preprocessing_contrast_enhancement_ratio", 1.0)
    a += cfg.get("preprocessing_contrast_enhancement_offset", 125)
    return np.clip(a, 0, 255).astype(np.uint8)


def edge_cfg(pair, ch=2, **more):
    return dict(EDGE, preprocessing_edge_detection_threshold_a=pair[0], preprocessing_edge_detection_threshold_b=pair[1],
                preprocessing_edge_detection_destination_channel=ch, **more)


# the combination bench.py times: dynamic brightness, contrast 1.2, the default white / yellow masks (channels 0 and 1)
FULL = {"preprocessing_dynamic_brightness_enabled": True, "preprocessing_contrast_enhancement_ratio": 1.2, "preprocessing_color_filter_enabled": True}

FLAT_A, FLAT_B = 90, 200


@functools.lru_cache(maxsize=None)
def batch(h, w, n, stride):
    """n distinct frames for workgroups that take frames i, i + stride, i + 2 stride: rolled pool frames, brighter by 20 per round, and in the
    first three columns of that schedule the designed successions (snake -> black -> weak-rich | flat -> weak-rich -> 255 | weak-rich -> flat -> cut snake)."""
    P = pool(h, w)
    fill = P[[NOISE, SNAKE, CUT] + list(range(SMOOTH0, SMOOTH0 + N_SMOOTH))]
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        f = np.roll(fill[(3 * i) % len(fill)], (i // w % h, i % w), axis=(0, 1))
        out[i] = np.minimum(f.astype(np.int32) + 20 * (i // stride), 255)
    flat = lambda v: np.full((h, w, 3), v, np.uint8)
    plan = [[P[SNAKE], P[BLACK], P[SMOOTH0]], [flat(FLAT_A), P[SMOOTH0 + 1], P[WHITE]], [P[SMOOTH0 + 2], flat(FLAT_B), P[CUT]]]
    for r, column in enumerate(plan):
        for k, f in enumerate(column):
            if r + k * stride < n:
                out[r + k * stride] = f
    out.setflags(write=False)
    return out


def brightness_total(frames):
    """Sum of the three channel means of rows 40..118: what the dynamic-brightness delta is made from."""
    roi = frames[:, 40:119].astype(np.int64)
    return roi.sum(axis=(1, 2, 3)) / float(roi.shape[1] * roi.shape[2])


def check_batch(src, stride, edge):
    """(a) no two frames equal; (b) frames i and i + stride differ by >= 3 in the brightness total, i.e. by >= 1 in the dynamic-brightness delta,
    so the other frame's sums or trim table move every unclipped byte; (c), (d) the designed successions are in place and are what they claim."""
    n, h, w = src.shape[:3]
    assert len({f.tobytes() for f in src}) == n                                              # (a)
    tot = brightness_total(src)
    assert n > stride and np.abs(tot[stride:] - tot[:-stride]).min() >= 3.0                  # (b)
    P = pool(h, w)
    assert np.array_equal(src[0], P[SNAKE]) and np.array_equal(src[stride], P[BLACK])        # (d) black follows snake
    if n > 2 * stride + 2:
        assert np.array_equal(src[2 * stride], P[SMOOTH0]) and np.array_equal(src[1 + stride], P[SMOOTH0 + 1]) and np.array_equal(src[2], P[SMOOTH0 + 2])
        assert (src[1] == FLAT_A).all() and (src[2 + stride] == FLAT_B).all() and (src[1 + 2 * stride] == 255).all()
    if edge:                                                                                 # (c) weak-rich <-> no weak pixel, from the reference
        st = check_pool(h, w)
        assert st[SNAKE][0] > 0 and st[BLACK][:2] == (0, 0) and st[WHITE][:2] == (0, 0)
        for v in (FLAT_A, FLAT_B):
            assert canny_stats(np.full((h, w, 3), v, np.uint8), *DESIGN)[:2] == (0, 0)
        rich = st[SMOOTH0:SMOOTH0 + 3]
        assert all(p > 0 and l > 0 and r >= 2 for p, l, r in rich), rich
        if h * w >= 120 * 160:
            assert all(p >= 200 and l >= 1000 and r >= 10 for p, l, r in rich), rich


# ---- CPU: the oracle against the reference ---------------------------------------------------------------------------------------

B_SIZES = [(2, 4), (16, 24), (64, 64), (120, 160), (120, 200), (136, 200), (8, 2048)]


def test_reference_on_hand_made_frames():
    """The reference itself, on frames whose answer is known without it."""
    img = np.zeros((12, 16, 3), np.uint8)
    img[:, 8:] = 200                                                                         # a vertical step: thinned to one column, border to border
    edge, nms, rounds = np_canny(img, 60, 100)
    cols = np.flatnonzero(edge.any(0))
    assert len(cols) == 1 and cols[0] in (7, 8) and (edge[:, cols[0]] == 255).all() and rounds == 0 and (nms != 0).all()
    img[:, 8:] = 16                                                                          # 4 * 16 = 64: weak everywhere, nothing to hang on
    edge, nms, rounds = np_canny(img, 100, 60)
    assert not edge.any() and (nms == 0).sum() == 12 and rounds == 0
    img[:3, 8:] = 40                                                                         # a strong top: the weak column is walked row by row
    edge, nms, rounds = np_canny(img, 60, 100)
    assert (edge == 255).sum() >= 12 and rounds >= 8


@pytest.mark.parametrize("size", B_SIZES)
def test_inputs_meet_their_conditions(size):
    h, w = size
    check_pool(h, w)
    st60 = pool_stats(h, w, (60, 100))                                                       # the snake made for the default thresholds walks as far
    if h * w >= 64 * 64:
        assert st60[SNAKE][2] >= (700 if h * w >= 120 * 160 else 100) and st60[SNAKE][1] == 0 and st60[CUT][1] >= 50


@pytest.mark.parametrize("stride", [256, 304, 64])
@pytest.mark.parametrize("size", [(64, 64), (136, 200)])
def test_batches_meet_their_conditions(size, stride):
    """The batch builder for CU counts other than the one at hand (the GPU tests check the batch they run again)."""
    h, w = size
    check_batch(batch(h, w, 2 * stride + 3, stride), stride, edge=size == (64, 64))
    check_batch(batch(h, w, stride + 1, stride), stride, edge=False)


def test_trim_batches_meet_their_conditions():
    check_batch(batch(64, 64, 8 * 256 + 5, 8 * 256), 8 * 256, edge=False)
    check_batch(batch(128, 256, 2 * 256 + 3, 2 * 256), 2 * 256, edge=False)


@pytest.mark.parametrize("size", B_SIZES)
def test_oracle_canny_equals_numpy(make_env, size):
    h, w = size
    env = make_env("oracle", n_envs=1, track=None, render=False, img_h=h, img_w=w)
    for k, pair in enumerate(PAIRS):
        src = pool(h, w, pair if pair in ((60, 100), (200, 400)) else DESIGN)
        ch = k % 3                                                                           # every channel twice per size
        got = env.preprocess_host(src, edge_cfg(pair, ch))
        for i, f in enumerate(src):
            assert np.array_equal(got[i, ..., ch], np_canny(f, *pair)[0]), (size, pair, i)
            for c in range(3):
                if c != ch:
                    assert np.array_equal(got[i, ..., c], f[..., c]), (size, pair, i, c)     # identity trim elsewhere
        if pair == (3000, 5000):
            assert not got[..., ch].any()
        if pair == (-5, 50) and h * w >= 64 * 64:
            assert got[NOISE, ..., ch].mean() > 40                                           # noise: a local maximum almost everywhere it can be


@pytest.mark.parametrize("ch", [0, 1, 2])
@pytest.mark.parametrize("size", [(16, 24), (64, 64), (120, 160), (136, 200)])
def test_oracle_canny_sees_the_trimmed_frame_and_is_merged_last(make_env, size, ch):
    """Contrast, dynamic brightness and colour masks on: Canny runs on the trimmed frame (not on the raw one, not on the masks),
    and its layer replaces whatever the masks put into its channel."""
    h, w = size
    env = make_env("oracle", n_envs=1, track=None, render=False, img_h=h, img_w=w)
    src = pool(h, w)
    cfg = edge_cfg(DESIGN, ch, **FULL)
    got = env.preprocess_host(src, cfg)
    masks = env.preprocess_host(src, FULL)
    differs = 0
    for i, f in enumerate(src):
        t = trimmed(f, cfg)
        want = np_canny(t, *DESIGN)[0]
        assert np.array_equal(got[i, ..., ch], want), (size, i)
        differs += int(not np.array_equal(want, np_canny(f, *DESIGN)[0]))
        for c in range(3):
            if c != ch:
                assert np.array_equal(got[i, ..., c], masks[i, ..., c]), (size, i, c)
    assert differs >= 3                                                                      # the trim matters to the edges of these frames


# ---- GPU: the kernels against the oracle, bit for bit -----------------------------------------------------------------------------


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def pair_envs(make_env, h, w, **kw):
    kw = dict(dict(n_envs=1, track=None, render=False), **kw)
    return make_env("hip", img_h=h, img_w=w, **kw), make_env("oracle", img_h=h, img_w=w, **kw)


def first_difference(got, want):
    d = np.argwhere(got != want)
    return None if len(d) == 0 else (len(d), d[0].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("size", B_SIZES + [(240, 320)])
def test_gpu_hysteresis_on_designed_frames(make_env, size):
    """One frame per workgroup, content that makes the sweeps, the backward walk, strip crossings and the weak vote matter."""
    h, w = size
    check_pool(h, w)
    g, o = pair_envs(make_env, h, w)
    for k, pair in enumerate(PAIRS):
        src = pool(h, w, pair if pair in ((60, 100), (200, 400)) else DESIGN)
        cfg = edge_cfg(pair, k % 3)
        got, want = g.preprocess_host(src, cfg), o.preprocess_host(src, cfg)
        assert np.array_equal(got, want), (size, pair, first_difference(got, want))
    cfg = edge_cfg(DESIGN, 0, **FULL)
    got, want = g.preprocess_host(pool(h, w), cfg), o.preprocess_host(pool(h, w), cfg)
    assert np.array_equal(got, want), (size, "full", first_difference(got, want))


EDGE_BATCHES = [((64, 64), 1, 1), ((64, 64), 2, 3), ((120, 160), 1, 1), ((120, 160), 2, 3), ((120, 200), 1, 1), ((136, 200), 2, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", EDGE_BATCHES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1]}G+{s[2]}")
def test_gpu_edge_kernel_more_frames_than_workgroups(make_env, shape):
    """n = G + 1 and 2 G + 3 frames on min(n, G) workgroups: second and third trips through the frame loop (prefetch, sums and trim
    table by parity, re-zeroed sums and borders, reused work arrays), a ragged last round."""
    (h, w), mul, add = shape
    G = cu_count()
    n = mul * G + add
    grid = min(n, G)                                                                         # trs_preprocess: one workgroup per CU at most
    assert n > grid
    src = batch(h, w, n, G)
    check_batch(src, G, edge=True)
    g, o = pair_envs(make_env, h, w)
    for cfg in (edge_cfg(DESIGN), edge_cfg(DESIGN, 2, **FULL)):
        got, want = g.preprocess_host(src, cfg), o.preprocess_host(src, cfg)
        assert np.array_equal(got, want), (shape, cfg, first_difference(got, want))


TRIM_CFGS = [
    {"preprocessing_contrast_enhancement_ratio": 1.37, "preprocessing_contrast_enhancement_offset": 110},          # static trim: <false>, one pass
    {"preprocessing_dynamic_brightness_enabled": True},                                                            # <true>, the frame in registers
    {"preprocessing_dynamic_brightness_enabled": True, "preprocessing_contrast_enhancement_ratio": 1.2, "preprocessing_color_filter_enabled": True},   # <true> on 256 threads, <false> on 1024
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [((64, 64), 8, 5), ((128, 256), 2, 3)], ids=["64x64-8G+5", "128x256-2G+3"])
def test_gpu_trim_kernel_more_frames_than_workgroups(make_env, shape):
    (h, w), mul, add = shape
    G = cu_count()
    assert (mul == 2) == (h * w // 4 >= 8192)                                                # 1024-thread workgroups, 2 per CU, from 8,192 groups on
    grid = mul * G
    n = grid + add
    assert n > grid
    src = batch(h, w, n, grid)
    check_batch(src, grid, edge=False)
    g, o = pair_envs(make_env, h, w)
    for cfg in TRIM_CFGS:
        got, want = g.preprocess_host(src, cfg), o.preprocess_host(src, cfg)
        assert np.array_equal(got, want), (shape, cfg, first_difference(got, want))


@pytest.mark.gpu
def test_gpu_normalize_stride_loop(make_env):
    h, w = 120, 160
    G = cu_count()
    per_frame = h * w * 3 // 4
    n = 16 * G * 256 // per_frame + 2
    n4 = n * per_frame
    assert (n4 + 255) // 256 > 16 * G and n4 > 16 * G * 256                                  # more dwords than threads: the loop's second trip
    src = batch(h, w, n, n)
    g, _ = pair_envs(make_env, h, w)
    want = src.astype(np.float32) / 255
    assert np.array_equal(g.normalize_host(src), want)


@pytest.mark.gpu
def test_gpu_preprocess_latest_more_envs_than_workgroups(make_env):
    """Device source, the env's own destination: n = G + 44 rendered frames, so 44 workgroups take a second one (the frame loop only:
    rendered frames are poor in weak pixels)."""
    torch = pytest.importorskip("torch")
    G = cu_count()
    n = G + 44
    assert n > min(n, G)
    g = make_env("hip", n_envs=n, auto_reset=True, img_h=64, img_w=64)
    o = make_env("oracle", n_envs=n, auto_reset=True, img_h=64, img_w=64)
    for env in (g, o):
        env.step_synthetic(20, 1)
    cfg = edge_cfg((60, 100), 2, preprocessing_dynamic_brightness_enabled=True, preprocessing_color_filter_enabled=True)
    want = o.preprocess_host(o.fetch("img"), cfg)
    handle = g.preprocess_latest(cfg)
    g.sync()
    dev = torch.as_tensor(handle, device="cuda").cpu().numpy()
    assert np.array_equal(dev, want), first_difference(dev, want)
