"""The tub image format ("tub image (JPEG)", include/trsim_spec.h) restated in numpy from the spec text — header, tables, colour, edges,
DCT, quantiser and entropy coder — and pinned three ways: against Pillow byte for byte (where Pillow imports), against the files Pillow wrote
for the committed frames of tests/golden/jpeg_pillow.npz (where it does not), and against what the host header csrc/trsim_jpeg_tables.hpp
produces (tests/jpeg_driver.cpp, built with the address and undefined-behaviour sanitizers).  tests/test_jpeg_gpu.py takes its reference from here."""
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
# JPEG standard, Annex K: quantisation bases (natural order), Huffman table specifications (counts per code length 1..16, symbols), zig-zag
LUM_BASE = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHR_BASE = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFF_SPECS = [("dc0", 0x00, DC_LUM), ("ac0", 0x10, AC_LUM), ("dc1", 0x01, DC_CHR), ("ac1", 0x11, AC_CHR)]     # the header's order
HEADER_BYTES = 623


def zigzag():
    """natural index of the k-th coefficient of the zig-zag scan"""
    order, r, c, up = [], 0, 0, True
    for _ in range(64):
        order.append(r * 8 + c)
        if up:
            if c == 7:
                r, up = r + 1, False
            elif r == 0:
                c, up = c + 1, False
            else:
                r, c = r - 1, c + 1
        else:
            if r == 7:
                c, up = c + 1, True
            elif c == 0:
                r, up = r + 1, True
            else:
                r, c = r + 1, c - 1
    return order


ZZ = zigzag()


def quant_tables(quality):
    """(luminance, chrominance), natural order"""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (LUM_BASE, CHR_BASE))


def huff_codes(spec):
    """symbol -> (code, length) of a table specification: codes of one length count up, and double when the length grows"""
    counts, symbols = spec
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[symbols[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return table


def header(h, w, quality):
    be16 = lambda v: bytes([v >> 8, v & 255])
    out = b"\xff\xd8" + b"\xff\xe0" + be16(16) + b"JFIF\x00" + bytes([1, 1, 0]) + be16(1) + be16(1) + bytes([0, 0])
    for i, q in enumerate(quant_tables(quality)):
        out += b"\xff\xdb" + be16(67) + bytes([i]) + bytes(q[ZZ[k]] for k in range(64))
    out += b"\xff\xc0" + be16(17) + bytes([8]) + be16(h) + be16(w) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for _, ident, (counts, symbols) in HUFF_SPECS:
        out += b"\xff\xc4" + be16(19 + len(symbols)) + bytes([ident]) + bytes(counts) + bytes(symbols)
    out += b"\xff\xda" + be16(12) + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return out


def geometry(h, w):
    """MCU rows and columns, and dummy[my, mx, k]: the Y block k (Y00 Y01 Y10 Y11) of that MCU lies wholly beyond the image's block rows or columns"""
    mh, mw = -(-h // 16), -(-w // 16)
    rows, cols = -(-h // 8), -(-w // 8)
    my, mx, k = np.meshgrid(np.arange(mh), np.arange(mw), np.arange(4), indexing="ij")
    dummy = (2 * my + k // 2 >= rows) | (2 * mx + k % 2 >= cols)
    return mh, mw, dummy


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """one pass of the integer forward DCT along the last axis of d (int64[..., 8])"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def _blocks(plane, q):
    """quantised coefficients int64[rows/8, cols/8, 64] in zig-zag order of a padded sample plane"""
    r, c = plane.shape
    b = plane.reshape(r // 8, 8, c // 8, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    b = _dct_pass(b, True)                                            # rows
    b = _dct_pass(b.swapaxes(-1, -2), False).swapaxes(-1, -2)         # columns
    qv = (np.asarray(q, np.int64) << 3).reshape(8, 8)
    a = np.abs(b) + (qv >> 1)
    v = np.where(a >= qv, a // qv, 0) * np.sign(b)
    return v.reshape(r // 8, c // 8, 64)[..., ZZ]


def coefficients(img, quality):
    """int64[n_mcu, 6, 64]: the quantised blocks of every MCU (Y00 Y01 Y10 Y11 Cb Cr, zig-zag order), MCUs in raster order, dummy blocks filled in"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w = img.shape[:2]
    mh, mw, dummy = geometry(h, w)
    fix = lambda x: int(x * 65536 + 0.5)
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16
    ql, qc = quant_tables(quality)
    y = np.pad(y, ((0, -h % 8), (0, -w % 8)), mode="edge")
    zy = np.zeros((2 * mh, 2 * mw, 64), np.int64)
    zy[:y.shape[0] // 8, :y.shape[1] // 8] = _blocks(y, ql)
    zy = zy.reshape(mh, 2, mw, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, 4, 64)
    for k in range(1, 4):                                             # dummy blocks: no AC, the DC of the block before them in the MCU
        zy[..., k, 1:] = np.where(dummy[..., k, None], 0, zy[..., k, 1:])
        zy[..., k, 0] = np.where(dummy[..., k], zy[..., k - 1, 0], zy[..., k, 0])
    assert not dummy[..., 0].any()
    chroma = []
    for p in (cb, cr):
        p = np.pad(p, ((0, h % 2), (0, 16 * mw - w)), mode="edge")
        bias = np.tile(np.array([1, 2], np.int64), p.shape[1] // 4)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        p = np.pad(p, ((0, 8 * mh - p.shape[0]), (0, 0)), mode="edge")
        chroma.append(_blocks(p, qc).reshape(mh, mw, 1, 64))
    return np.concatenate([zy] + chroma, axis=2).reshape(mh * mw, 6, 64)


def _bit_length(v):
    v = np.asarray(v, np.int64)
    n = np.zeros(v.shape, np.int64)
    for k in range(12):
        n += (v >> k) > 0
    return n


def _lut(spec, size):
    code, length = np.zeros(size, np.int64), np.zeros(size, np.int64)
    for s, (c, l) in huff_codes(spec).items():
        code[s], length[s] = c, l
    return code, length


def entropy(z):
    """(scan bytes with stuffing and the padded last byte, statistics) of coefficients()'s blocks"""
    n = z.shape[0]
    comp = np.array([0, 0, 0, 0, 1, 2])
    diff = np.zeros((n, 6), np.int64)
    for c in range(3):
        dc = z[:, comp == c, 0].reshape(-1)
        diff[:, comp == c] = np.diff(dc, prepend=0).reshape(n, -1)
    chroma = (comp > 0)[None, :, None]
    # per coefficient up to 4 tokens (3 ZRL + the coefficient's own code with its extra bits appended), then one EOB slot per block
    code, length = np.zeros((n, 6, 65, 4), np.int64), np.zeros((n, 6, 65, 4), np.int64)
    v = z.copy()
    v[:, :, 0] = diff
    cat = _bit_length(np.abs(v))
    extra = np.where(v < 0, v - 1, v) & ((1 << cat) - 1)
    k = np.broadcast_to(np.arange(64), v.shape)
    nz = v != 0
    nz_ac = nz.copy()
    nz_ac[:, :, 0] = False
    last = np.maximum.accumulate(np.where(nz_ac, k, 0), axis=2)                         # the last non-zero AC position up to and including k
    prev = np.concatenate([np.zeros((n, 6, 1), np.int64), last[:, :, :-1]], axis=2)     # ... before k
    run = k - prev - 1
    dcc = [_lut(DC_LUM, 12), _lut(DC_CHR, 12)]
    acc = [_lut(AC_LUM, 256), _lut(AC_CHR, 256)]
    sym = np.where(nz_ac, ((run & 15) << 4) | cat, 0)
    ac_code, ac_len = np.where(chroma, acc[1][0][sym], acc[0][0][sym]), np.where(chroma, acc[1][1][sym], acc[0][1][sym])
    dc_code = np.where(chroma[..., 0], dcc[1][0][cat[:, :, 0]], dcc[0][0][cat[:, :, 0]])
    dc_len = np.where(chroma[..., 0], dcc[1][1][cat[:, :, 0]], dcc[0][1][cat[:, :, 0]])
    code[:, :, :64, 3] = np.where(nz_ac, (ac_code << cat) | extra, 0)
    length[:, :, :64, 3] = np.where(nz_ac, ac_len + cat, 0)
    code[:, :, 0, 3], length[:, :, 0, 3] = (dc_code << cat[:, :, 0]) | extra[:, :, 0], dc_len + cat[:, :, 0]
    n_zrl = np.where(nz_ac, run >> 4, 0)
    for j in range(3):
        on = n_zrl > j
        code[:, :, :64, j] = np.where(on, np.where(chroma, acc[1][0][0xF0], acc[0][0][0xF0]), 0)
        length[:, :, :64, j] = np.where(on, np.where(chroma, acc[1][1][0xF0], acc[0][1][0xF0]), 0)
    eob = last[:, :, 63] < 63
    code[:, :, 64, 0] = np.where(eob, np.where(chroma[..., 0], acc[1][0][0], acc[0][0][0]), 0)
    length[:, :, 64, 0] = np.where(eob, np.where(chroma[..., 0], acc[1][1][0], acc[0][1][0]), 0)
    code, length = code.reshape(-1), length.reshape(-1)
    keep = length > 0
    code, length = code[keep], length[keep]
    total = int(length.sum())
    owner = np.repeat(np.arange(length.size), length)
    within = np.arange(total) - np.repeat(np.cumsum(length) - length, length)
    bits = ((code[owner] >> (length[owner] - 1 - within)) & 1).astype(np.uint8)
    pad = -total % 8
    raw = np.packbits(np.concatenate([bits, np.ones(pad, np.uint8)])).tobytes()
    ac_cat = np.where(nz_ac, cat, 0)
    stats = {"stuffed": raw.count(b"\xff"), "zrl": int(n_zrl.sum()), "ac_sizes": sorted(set(np.unique(ac_cat).tolist()) - {0}),
             "max_category": int(cat.max()), "pad_bits": pad, "only_dc_and_eob": bool(not nz_ac.any() and eob.all())}
    return raw.replace(b"\xff", b"\xff\x00"), stats


def encode(img, quality=75, with_stats=False):
    """the file the spec defines for one uint8[H][W][3] frame"""
    img = np.asarray(img)
    scan, stats = entropy(coefficients(img, quality))
    data = header(img.shape[0], img.shape[1], quality) + scan + b"\xff\xd9"
    return (data, stats) if with_stats else data


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
SIZES = [(8, 12), (24, 40), (50, 100), (60, 80), (120, 160), (240, 320)]
QUALITIES = [75, 50, 95, 100, 10]


def frame(kind, h, w, seed=0):
    if kind == "noise":
        return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([(255 * xx) // max(w - 1, 1), (255 * yy) // max(h - 1, 1), (255 * (xx + yy)) // max(h + w - 2, 1)], axis=-1).astype(np.uint8)
    if kind == "flat0":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "flat255":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    raise ValueError(kind)


def pillow_bytes(img, quality=None):
    from PIL import Image
    buf = io.BytesIO()
    if quality is None:
        Image.fromarray(img).save(buf, format="JPEG")
    else:
        Image.fromarray(img).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


# ---- 1. against Pillow -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_restatement_equals_pillow(h, w):
    pytest.importorskip("PIL")
    for q in QUALITIES:
        for kind in ("noise", "ramp", "flat0", "flat255"):
            img = frame(kind, h, w)
            assert encode(img, q) == pillow_bytes(img, q), (kind, h, w, q)
    img = frame("checker", h, w)
    assert encode(img, 100) == pillow_bytes(img, 100), ("checker", h, w)
    assert encode(frame("ramp", h, w)) == pillow_bytes(frame("ramp", h, w)), "the default quality is 75"


# ---- 2. against the committed files ------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_committed_pillow_files():
    z = np.load(os.path.join(GOLDEN, "jpeg_pillow.npz"))
    names = sorted(k[len("frame_"):] for k in z.files if k.startswith("frame_"))
    assert len(names) >= 6 and "rendered_120x160" in names
    assert str(z["pillow_version"]) and str(z["libjpeg_version"])
    for name in names:
        q = int(z["quality_" + name])
        assert encode(z["frame_" + name], q) == z["file_" + name].tobytes(), name


# ---- 3. against the host header ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jpeg_driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("jpeg") / "jpeg_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "jpeg_driver.cpp")])
    return str(exe)


def run_driver(exe, *args):
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-2000:]
    return [line.split() for line in out.stdout.splitlines()]


def test_host_header_equals_the_restatement(jpeg_driver):
    """quant tables, header bytes, the Huffman tables as the kernel reads them (length << 16 | code per symbol) and the block predicates"""
    for q in QUALITIES + [1, 49, 51]:
        rows = run_driver(jpeg_driver, "quant", q)
        assert [[int(x) for x in r[1:]] for r in rows] == [list(t) for t in quant_tables(q)], q
    for h, w in SIZES:
        for q in QUALITIES:
            (row,) = run_driver(jpeg_driver, "header", h, w, q)
            assert bytes.fromhex(row[0]) == header(h, w, q), (h, w, q)
    rows = run_driver(jpeg_driver, "huffman")
    assert [r[0] for r in rows] == ["dc0", "ac0", "dc1", "ac1"]
    for r, (name, _, spec) in zip(rows, HUFF_SPECS):
        want = [0] * (12 if name[0] == "d" else 256)
        for s, (c, l) in huff_codes(spec).items():
            want[s] = l << 16 | c
        assert [int(x) for x in r[1:]] == want, name
    assert run_driver(jpeg_driver, "zigzag") == [[str(v) for v in ZZ]]
    for h, w in SIZES + [(16, 16), (17, 33), (9, 8)]:
        rows = run_driver(jpeg_driver, "geometry", h, w)
        mh, mw, dummy = geometry(h, w)
        assert [int(x) for x in rows[0]] == [mh, mw, 6 * mw, HEADER_BYTES]
        assert rows[1][0] == "".join("01"[int(d)] for d in dummy.reshape(-1)), (h, w)
        # the sample a padded plane position reads: Y and full-resolution chroma clamp, the downsampled chroma plane replicates its last row
        yy = [int(x) for x in rows[2]]
        assert yy == [min(r, h - 1) for r in range(16 * mh)]
        cc = [[int(x) for x in p.split(",")] for p in rows[3]]
        last = -(-h // 2) - 1
        assert cc == [[min(2 * min(r, last), h - 1), min(2 * min(r, last) + 1, h - 1)] for r in range(8 * mh)]


def test_host_arithmetic_equals_the_restatement(jpeg_driver, tmp_path):
    """colour, edge rules, downsampling, both DCT passes and the quantiser of the host header — the functions the kernel calls — give the restatement's blocks"""
    for (h, w), kind, q in [((8, 12), "noise", 75), ((24, 40), "noise", 100), ((50, 100), "noise", 10), ((60, 80), "ramp", 95), ((24, 40), "checker", 100),
                            ((50, 100), "ramp", 50), ((9, 8), "noise", 75), ((17, 33), "noise", 75)]:
        img = frame(kind, h, w)
        path = tmp_path / "frame.rgb"
        path.write_bytes(img.tobytes())
        got = np.array([[int(x) for x in r] for r in run_driver(jpeg_driver, "blocks", h, w, q, path)], np.int64).reshape(-1, 6, 64)
        want = coefficients(img, q)
        _, _, dummy = geometry(h, w)
        dummy = np.concatenate([dummy.reshape(-1, 4), np.zeros((want.shape[0], 2), bool)], axis=1)
        assert np.array_equal(got[..., 1:], want[..., 1:]), (h, w, kind, q)
        assert np.array_equal(got[..., 0][~dummy], want[..., 0][~dummy]), (h, w, kind, q)
    rows = np.array([[int(x) for x in r] for r in run_driver(jpeg_driver, "bits")], np.int64)
    v = rows[:, 0]
    assert np.array_equal(v, np.arange(-2047, 2048))
    cat = _bit_length(np.abs(v))
    assert np.array_equal(rows[:, 1], cat) and np.array_equal(rows[:, 2], np.where(v < 0, v - 1, v) & ((1 << cat) - 1))
