"""Writes tests/golden/jpeg_decode_pillow.npz: JPEG files and the frames Pillow decodes them to — the pin of tests/test_jpeg_decode_cpu.py where Pillow
does not import.  Run from the repository root with Pillow installed:  python tests/golden/gen_jpeg_decode_golden.py
  file_<name>, frame_<name>   files of frames up to 60 x 80 (plain and optimize=True, five qualities) and np.asarray(Image.open(file))
  foreign_<kind>              24 x 40 files the decoder reports as unsupported: progressive, grayscale, 4:4:4 (files only)
  optfile_<H>x<W>             one optimize=True file per size of tests/test_jpeg_decode_gpu.py (files only: smooth content keeps them small)"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_jpeg_cpu import frame  # noqa: E402


def save(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format="JPEG", **kw)
    return buf.getvalue()


def smooth(h, w):
    """a ramp with one block of noise and one checkered block: a few long codes among many short ones"""
    g = frame("ramp", h, w)
    g[:8, :8] = frame("noise", 8, 8)
    g[8:16, 8:16] = frame("checker", 8, 8)
    return g


out = {"pillow_version": np.array(PIL.__version__), "libjpeg_version": np.array(str(features.version("jpg")))}
for h, w in [(8, 12), (17, 33), (24, 40), (60, 80)]:
    for kind, q, opt in [("noise", 75, False), ("ramp", 50, True), ("checker", 100, False), ("noise", 10, True), ("flat255", 95, False), ("ramp", 100, False)]:
        data = save(Image.fromarray(frame(kind, h, w)), quality=q, optimize=opt)
        name = f"{kind}_{h}x{w}_q{q}" + ("_opt" if opt else "")
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["frame_" + name] = np.asarray(Image.open(io.BytesIO(data)))
img = Image.fromarray(frame("noise", 24, 40))
out["foreign_progressive"] = np.frombuffer(save(img, quality=75, progressive=True), np.uint8)
out["foreign_grayscale"] = np.frombuffer(save(img.convert("L"), quality=75), np.uint8)
out["foreign_s444"] = np.frombuffer(save(img, quality=75, subsampling=0), np.uint8)
for h, w in [(24, 40), (50, 100), (60, 80), (120, 160), (240, 320)]:
    out[f"optfile_{h}x{w}"] = np.frombuffer(save(Image.fromarray(smooth(h, w)), quality=75, optimize=True), np.uint8)
path = os.path.join(HERE, "jpeg_decode_pillow.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
