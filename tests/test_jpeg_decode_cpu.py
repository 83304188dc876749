"""Reading a tub image ("tub image (JPEG), decoding", include/trsim_spec.h) restated in numpy and plain Python from the spec text — marker walk,
tables from the file, entropy decoding, dequantiser, inverse DCT, triangle upsampling, colour and the status decision — and pinned against Pillow's
decoder byte for byte (where Pillow imports), against the frames Pillow decoded for the committed files of tests/golden/jpeg_decode_pillow.npz (where
it does not), and against what the shared header csrc/trsim_jpeg_decode.hpp computes on the host (tests/jpeg_decode_driver.cpp, built with the
address and undefined-behaviour sanitizers, files in exact-size heap buffers).  tests/test_jpeg_decode_gpu.py takes its reference from here."""
import io
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_jpeg_cpu import QUALITIES, SIZES, ZZ, encode, frame

DECODED, SKIPPED, UNSUPPORTED, SIZE_DIFFERS, CORRUPT = 0, 1, 2, 3, 4


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def parse(data, h=None, w=None):
    """The marker walk SOI..SOS -> the tables and sizes the scan needs; raises _Stop(status).  (h, w): the size the caller expects, None: the file's."""
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise _Stop(CORRUPT)
    pos, dqt, dht, sof = 2, {}, {}, None
    while True:
        if pos + 4 > n or data[pos] != 0xFF:
            raise _Stop(CORRUPT)
        m = data[pos + 1]
        if m == 0xFF:                                                  # fill bytes: legal, never written by the encoders this reads
            raise _Stop(UNSUPPORTED)
        if m <= 0x01 or 0xD0 <= m <= 0xD9:                             # markers without a segment have no place before the scan
            raise _Stop(CORRUPT)
        length = data[pos + 2] << 8 | data[pos + 3]
        seg, end = pos + 4, pos + 2 + length
        if length < 2 or end > n:
            raise _Stop(CORRUPT)
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            if m == 0xEE and end - seg >= 5 and data[seg:seg + 5] == b"Adobe":
                raise _Stop(UNSUPPORTED)
        elif m == 0xDB:
            q = seg
            while q < end:
                if data[q] >> 4:
                    raise _Stop(UNSUPPORTED)                           # 16-bit tables
                if (data[q] & 15) > 3 or q + 65 > end:
                    raise _Stop(CORRUPT)
                dqt[data[q] & 15] = list(data[q + 1:q + 65])           # zig-zag order
                q += 65
        elif m == 0xC4:
            q = seg
            while q < end:
                cls, ident = data[q] >> 4, data[q] & 15
                if cls > 1 or ident > 3 or q + 17 > end:
                    raise _Stop(CORRUPT)
                if ident > 1:
                    raise _Stop(UNSUPPORTED)                           # baseline has two tables per class
                counts = list(data[q + 1:q + 17])
                total, code = sum(counts), 0
                for length_ in range(1, 17):                           # more codes of a length than there is room for
                    code += counts[length_ - 1]
                    if code > 1 << length_:
                        raise _Stop(CORRUPT)
                    code <<= 1
                if total > 256 or q + 17 + total > end:
                    raise _Stop(CORRUPT)
                dht[cls, ident] = (counts, list(data[q + 17:q + 17 + total]))
                q += 17 + total
        elif m == 0xC0:
            if sof is not None or length < 8 or length != 8 + 3 * data[seg + 5]:
                raise _Stop(CORRUPT)
            if data[seg] != 8 or data[seg + 5] != 3:
                raise _Stop(UNSUPPORTED)
            comps = [tuple(data[seg + 6 + 3 * c:seg + 9 + 3 * c]) for c in range(3)]
            if [c[:2] for c in comps] != [(1, 0x22), (2, 0x11), (3, 0x11)]:
                raise _Stop(UNSUPPORTED)
            if any(c[2] > 3 for c in comps):
                raise _Stop(CORRUPT)
            sof = (data[seg + 1] << 8 | data[seg + 2], data[seg + 3] << 8 | data[seg + 4], [c[2] for c in comps])
        elif m == 0xDA:
            if sof is None or length < 6 or length != 6 + 2 * data[seg]:
                raise _Stop(CORRUPT)
            if data[seg] != 3:
                raise _Stop(UNSUPPORTED)
            sel = [(data[seg + 1 + 2 * c], data[seg + 2 + 2 * c]) for c in range(3)]
            if [s[0] for s in sel] != [1, 2, 3] or any(s[1] >> 4 > 1 or s[1] & 15 > 1 for s in sel):
                raise _Stop(UNSUPPORTED)
            if tuple(data[seg + 7:seg + 10]) != (0, 63, 0):
                raise _Stop(UNSUPPORTED)
            fh, fw, tq = sof
            if fw <= 4:
                raise _Stop(UNSUPPORTED)                               # a chroma plane of width <= 2: libjpeg-turbo leaves the triangle filter
            if (fh, fw) != (fh if h is None else h, fw if w is None else w) or fh < 1:
                raise _Stop(SIZE_DIFFERS)
            for c in range(3):
                if tq[c] not in dqt or (0, sel[c][1] >> 4) not in dht or (1, sel[c][1] & 15) not in dht:
                    raise _Stop(CORRUPT)
            return {"h": fh, "w": fw, "scan": end, "q": [dqt[tq[c]] for c in range(3)],
                    "dc": [dht[0, sel[c][1] >> 4] for c in range(3)], "ac": [dht[1, sel[c][1] & 15] for c in range(3)]}
        else:                                                          # other frame types (progressive, extended, arithmetic), DRI, DNL, ...
            raise _Stop(UNSUPPORTED)
        pos = end


def _lut16(spec):
    """symbol and code length by the next 16 bits (length 0: no code of the table starts them)"""
    counts, symbols = spec
    sym, ln = np.zeros(1 << 16, np.int64), np.zeros(1 << 16, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            lo = code << (16 - length)
            sym[lo:lo + (1 << (16 - length))], ln[lo:lo + (1 << (16 - length))] = symbols[k], length
            code, k = code + 1, k + 1
        code <<= 1
    return sym.tolist(), ln.tolist()


def entropy_decode(data, info):
    """int64[n_mcu, 6, 64] coefficients in zig-zag order (not yet dequantised) and statistics; raises _Stop(CORRUPT)"""
    scan = bytes(data[info["scan"]:])
    m = re.search(b"\xff[^\x00]", scan, re.S)                          # the scan's bytes end at the first marker, or with the file
    if m:
        scan = scan[:m.start()]
    elif scan.endswith(b"\xff"):
        scan = scan[:-1]
    raw = scan.replace(b"\xff\x00", b"\xff")
    total = 8 * len(raw)
    bits = np.concatenate([np.unpackbits(np.frombuffer(raw, np.uint8)), np.zeros(32, np.uint8)]).astype(np.int64)
    win = np.zeros(total + 16, np.int64)
    for k in range(16):
        win |= bits[k:k + total + 16] << (15 - k)
    win = win.tolist()
    luts = {}
    for spec in info["dc"] + info["ac"]:
        key = (tuple(spec[0]), tuple(spec[1]))
        if key not in luts:
            luts[key] = _lut16(spec)
    dc = [luts[tuple(s[0]), tuple(s[1])] for s in info["dc"]]
    ac = [luts[tuple(s[0]), tuple(s[1])] for s in info["ac"]]
    n_mcu = -(-info["h"] // 16) * -(-info["w"] // 16)
    z = np.zeros((n_mcu, 6, 64), np.int64)
    pred = [0, 0, 0]
    pos = 0
    stats = {"zrl": 0, "ac_sizes": set(), "dc_eob_blocks": 0, "block_bits": []}

    def take(n):
        nonlocal pos
        if pos + n > total:
            raise _Stop(CORRUPT)                                       # a bit at or beyond the scan's end
        v = win[pos] >> (16 - n) if n else 0
        pos += n
        return v

    def symbol(lut):
        nonlocal pos
        length = lut[1][win[pos]] if pos < total else 0
        if not length or pos + length > total:
            raise _Stop(CORRUPT)                                       # no code of the table, or one that runs past the end
        s = lut[0][win[pos]]
        pos += length
        return s

    def extend(v, s):
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1

    for i in range(n_mcu):
        for b in range(6):
            c = (0, 0, 0, 0, 1, 2)[b]
            stats["block_bits"].append(pos)
            s = symbol(dc[c])
            if s > 11:
                raise _Stop(CORRUPT)
            pred[c] += extend(take(s), s) if s else 0
            z[i, b, 0] = pred[c]
            k, plain = 1, True
            while k < 64:
                rs = symbol(ac[c])
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        break                                          # EOB
                    k += 16
                    stats["zrl"] += 1
                    plain = False
                    continue
                k += r
                if k > 63 or s > 10:
                    raise _Stop(CORRUPT)
                z[i, b, k] = extend(take(s), s)
                stats["ac_sizes"].add(s)
                k += 1
                plain = False
            else:
                if k > 64:
                    raise _Stop(CORRUPT)                               # a ZRL that runs beyond the block
            stats["dc_eob_blocks"] += plain
    stats["ac_sizes"] = sorted(stats["ac_sizes"])
    stats["scan_bits"] = pos
    stats["pad_bits"] = -pos % 8
    stats["stuffed"] = scan[:len(scan)].count(b"\xff\x00")
    # the file offset behind the byte that holds the scan's last bit
    used, off = (pos + 7) // 8, info["scan"]
    for _ in range(used):
        off += 2 if data[off] == 0xFF else 1
    stats["scan_end"] = off
    return z, stats


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(d, n):
    """one pass of the integer inverse DCT along the last axis of d (int64[..., 8])"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., i] for i in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([_descale(o, n) for o in out], axis=-1)


def samples(z, q):
    """uint8-valued int64[..., 8, 8] samples of zig-zag coefficient blocks z[..., 64] with the quantisation table q (zig-zag order)"""
    nat = np.zeros(z.shape, np.int64)
    nat[..., ZZ] = z * np.asarray(q, np.int64)
    b = nat.reshape(z.shape[:-1] + (8, 8))
    b = _idct_pass(b.swapaxes(-1, -2), 11).swapaxes(-1, -2)            # columns first
    b = _idct_pass(b, 18)                                              # rows
    return np.clip(b + 128, 0, 255)


def upsample(c, h, w):
    """the 2 x 2 triangle filter over the ceil(h / 2) x ceil(w / 2) real samples of a chroma plane -> int64[h, w]"""
    c = c[:-(-h // 2), :-(-w // 2)]
    above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    s = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    s[0::2], s[1::2] = 3 * c + above, 3 * c + below
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4       # (3 s + s = 4 s in the first and the last column)
    return out[:h, :w]


def decode(data, h=None, w=None):
    """(frame uint8[h][w][3] or None, status, statistics) of one file; (h, w): the size the caller expects (None: the file's own)"""
    data = bytes(data)
    try:
        info = parse(data, h, w)
        z, stats = entropy_decode(data, info)
    except _Stop as stop:
        return None, stop.status, {}
    h, w = info["h"], info["w"]
    mh, mw = -(-h // 16), -(-w // 16)
    z = z.reshape(mh, mw, 6, 64)
    y = samples(z[:, :, :4], info["q"][0]).reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(16 * mh, 16 * mw)[:h, :w]
    cb, cr = (upsample(samples(z[:, :, 4 + c], info["q"][1 + c]).transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw), h, w) - 128 for c in range(2))
    fix = lambda x: int(x * 65536 + 0.5)
    r = y + ((fix(1.402) * cr + 32768) >> 16)
    g = y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    b = y + ((fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8), DECODED, stats


# ---- files for the tests (tests/test_jpeg_decode_gpu.py takes them from here too) ------------------------------------------------------------------
def segments(data):
    """(marker, offset of the 0xFF, offset behind the segment) of every segment up to and including SOS"""
    pos, out = 2, []
    while True:
        m, end = data[pos + 1], pos + 2 + (data[pos + 2] << 8 | data[pos + 3])
        out.append((m, pos, end))
        if m == 0xDA:
            return out
        pos = end


def merge_dqt(data):
    """the same file with its two DQT segments merged into one segment that holds both tables"""
    seg = [s for s in segments(data) if s[0] == 0xDB]
    assert len(seg) == 2 and seg[0][2] == seg[1][1]
    tables = data[seg[0][1] + 4:seg[0][2]] + data[seg[1][1] + 4:seg[1][2]]
    return data[:seg[0][1]] + b"\xff\xdb" + bytes([(2 + len(tables)) >> 8, (2 + len(tables)) & 255]) + tables + data[seg[1][2]:]


def insert_dri(data):
    sos = [s for s in segments(data) if s[0] == 0xDA][0]
    return data[:sos[1]] + b"\xff\xdd\x00\x04\x00\x08" + data[sos[1]:]


def splice_ones(data, stats, scan):
    """sixteen 1-bits put between two blocks in the middle of the scan: the scan's bits are unstuffed, cut at a block boundary and stuffed again"""
    raw = data[scan:stats["scan_end"]].replace(b"\xff\x00", b"\xff")
    bits = np.unpackbits(np.frombuffer(raw, np.uint8))[:stats["scan_bits"]]
    cut = stats["block_bits"][len(stats["block_bits"]) // 2]
    bits = np.concatenate([bits[:cut], np.ones(16, np.uint8), bits[cut:]])
    bits = np.concatenate([bits, np.ones(-bits.size % 8, np.uint8)])
    return data[:scan] + np.packbits(bits).tobytes().replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


def golden_decode():
    return np.load(os.path.join(GOLDEN, "jpeg_decode_pillow.npz"))


def foreign_files(h, w):
    """{kind: file} of the kinds of JPEG the decoder leaves to the host — from Pillow where it imports, else the committed 24 x 40 ones"""
    try:
        from PIL import Image
    except ImportError:
        assert (h, w) == (24, 40)
        z = golden_decode()
        return {k: z["foreign_" + k].tobytes() for k in ("progressive", "grayscale", "s444")}
    out = {}
    img = Image.fromarray(frame("noise", h, w))
    for kind, im, kw in (("progressive", img, {"progressive": True}), ("grayscale", img.convert("L"), {}), ("s444", img, {"subsampling": 0})):
        buf = io.BytesIO()
        im.save(buf, format="JPEG", quality=75, **kw)
        out[kind] = buf.getvalue()
    return out


def status_cases(h, w):
    """[(name, file, the status include/trsim_spec.h gives it)], each made from a valid h x w file"""
    data = encode(frame("noise", h, w), 75)
    _, st, stats = decode(data, h, w)
    assert st == DECODED
    scan = parse(data, h, w)["scan"]
    end = stats["scan_end"]
    assert data[end:] == b"\xff\xd9" and end - scan > 64
    cases = [(k, f, UNSUPPORTED) for k, f in foreign_files(h, w).items()]
    cases += [("dri", insert_dri(data), UNSUPPORTED),
              ("other size", encode(frame("noise", h + 8, w), 75), SIZE_DIFFERS),
              ("truncated in the header", data[:scan // 2], CORRUPT),
              ("truncated mid-MCU", data[:scan + (end - scan) // 2], CORRUPT),
              ("truncated one byte before the last MCU ends", data[:end - 1], CORRUPT),
              ("sixteen 1-bits", splice_ones(data, stats, scan), CORRUPT),
              ("early EOI", data[:scan + 40] + b"\xff\xd9" + data[scan + 40:], CORRUPT)]
    return data, cases


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def pillow_file(img, quality, optimize=False):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, optimize=optimize)
    return buf.getvalue()


# ---- 1. against Pillow's decoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_restatement_equals_pillow_decoder(h, w):
    pytest.importorskip("PIL")
    files = []
    for q in QUALITIES:
        for kind in ("noise", "ramp", "flat0", "flat255"):
            files.append(((kind, q), encode(frame(kind, h, w), q)))
        if h * w <= 120 * 160 or q in (75, 10):
            for kind in ("noise", "ramp"):
                files.append(((kind, q, "optimize"), pillow_file(frame(kind, h, w), q, optimize=True)))
    files.append((("checker", 100), encode(frame("checker", h, w), 100)))
    files.append((("merged DQT",), merge_dqt(encode(frame("noise", h, w, seed=1), 75))))
    for name, data in files:
        got, status, _ = decode(data, h, w)
        assert status == DECODED, name
        assert np.array_equal(got, pillow_decode(data)), (h, w) + name
    assert files[-1][1] != encode(frame("noise", h, w, seed=1), 75) and len(files[-1][1]) == len(encode(frame("noise", h, w, seed=1), 75)) - 4
    opt = [d for n_, d in files if n_[-1] == "optimize"]
    assert all(parse(d)["dc"][0] != parse(files[0][1])["dc"][0] or parse(d)["ac"][0] != parse(files[0][1])["ac"][0] for d in opt), "optimised tables are not the standard's"


# ---- 2. against the committed frames ---------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_committed_pillow_frames():
    z = golden_decode()
    names = sorted(k[len("frame_"):] for k in z.files if k.startswith("frame_"))
    assert len(names) >= 12 and any("opt" in n for n in names)
    assert str(z["pillow_version"]) and str(z["libjpeg_version"])
    for name in names:
        want = z["frame_" + name]
        assert want.shape[0] <= 60 and want.shape[1] <= 80
        got, status, _ = decode(z["file_" + name].tobytes(), want.shape[0], want.shape[1])
        assert status == DECODED and np.array_equal(got, want), name
    for kind in ("progressive", "grayscale", "s444"):
        assert decode(z["foreign_" + kind].tobytes(), 24, 40)[1] == UNSUPPORTED, kind
    for key in ("24x40", "50x100", "60x80", "120x160", "240x320"):
        hh, ww = (int(v) for v in key.split("x"))
        assert decode(z["optfile_" + key].tobytes(), hh, ww)[1] == DECODED, key


# ---- 3. statuses -----------------------------------------------------------------------------------------------------------------------------
def test_status_cases():
    data, cases = status_cases(24, 40)
    assert {name for name, _, _ in cases} >= {"progressive", "grayscale", "s444", "dri"}
    for name, file, want in cases:
        got, status, _ = decode(file, 24, 40)
        assert status == want, (name, status)
        assert got is None
    assert decode(data, 24, 48)[1] == SIZE_DIFFERS and decode(data, 32, 40)[1] == SIZE_DIFFERS
    assert decode(b"", 24, 40)[1] == CORRUPT and decode(b"\xff\xd8", 24, 40)[1] == CORRUPT
    assert decode(encode(frame("noise", 8, 4), 75))[1] == UNSUPPORTED                  # a chroma plane two samples wide
    try:                                                                               # every status-2 file here is one Pillow does decode
        for name, file, want in cases:
            if want == UNSUPPORTED and name != "grayscale":
                assert pillow_decode(file).shape == (24, 40, 3), name
    except ImportError:
        pass


# ---- 4. against the shared header, on the host and under the sanitizers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("jpeg_decode") / "jpeg_decode_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "jpeg_decode_driver.cpp")])
    return str(exe)


def run_decode_driver(exe, *args):
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return [line.split() for line in out.stdout.splitlines()]


def test_shared_header_equals_the_restatement(decode_driver, tmp_path):
    """the marker walk, table building, bit reader, block decoding, both IDCT passes, upsampling and colour of csrc/trsim_jpeg_decode.hpp — the functions
    the kernel calls — on files held in heap buffers of exactly their length"""
    z = golden_decode()
    for h, w in [(8, 12), (24, 40), (50, 100), (60, 80), (120, 160)]:
        files = [encode(frame(kind, h, w), q) for kind, q in (("noise", 75), ("noise", 100), ("noise", 10), ("ramp", 50), ("checker", 100), ("flat255", 95))]
        files.append(merge_dqt(files[0]))
        if f"optfile_{h}x{w}" in z.files:
            files.append(z[f"optfile_{h}x{w}"].tobytes())
        files += [f for _, f, _ in status_cases(h, w)[1]] if (h, w) == (24, 40) else []
        files += [b"", b"\xff", files[0][:2]]
        paths = []
        for i, data in enumerate(files):
            paths.append(tmp_path / f"f{h}_{i}.jpg")
            paths[-1].write_bytes(data)
        rows = run_decode_driver(decode_driver, "decode", h, w, *paths)
        assert len(rows) == len(files)
        for i, (row, data) in enumerate(zip(rows, files)):
            want, status, _ = decode(data, h, w)
            assert int(row[0]) == status, (h, w, i)
            if status == DECODED:
                assert bytes.fromhex(row[1]) == want.tobytes(), (h, w, i)
            else:
                assert len(row) == 1


def test_shared_header_survives_truncated_and_altered_files(decode_driver, tmp_path):
    """every prefix of one 24 x 40 file, and the file with each header byte altered in turn (three ways): any status will do; a sanitizer report (a read
    beyond the exact-size buffer, an overflow) or a run that does not end fails"""
    path = tmp_path / "whole.jpg"
    data = encode(frame("noise", 24, 40), 75)
    path.write_bytes(data)
    (row,) = run_decode_driver(decode_driver, "fuzz", 24, 40, path)
    counts = [int(v) for v in row]
    assert sum(counts) == len(data) + 1 + 3 * parse(data)["scan"]
    assert counts[SKIPPED] == 0 and counts[DECODED] >= 3 and counts[CORRUPT] >= len(data) - 3 and counts[UNSUPPORTED] >= 1 and counts[SIZE_DIFFERS] >= 1
