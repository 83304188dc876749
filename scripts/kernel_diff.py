#!/usr/bin/env python3
"""Are the gfx950 kernels of two source trees the same code?  (CPU only: hipcc cross-compiles to assembly.)

    python scripts/kernel_diff.py <tree A> <tree B> [-j N] [--rename OLD=NEW]...

A tree is a checkout of this repository (`git archive <rev> | tar -x -C <dir>` gives one of any commit).  Every `*.hip` under its
triton-racer-sim_amd/csrc is compiled with `-S --cuda-device-only` and the library's flags as that tree states them (HIPCC_FLAGS of its own __graft_entry__.py).  For every
kernel symbol the instruction text between its label and its `.Lfunc_end` is compared — comments stripped, the function-order index of local labels
(`.LBB<k>_` -> `.LBB_`) removed — and so is its metadata: register counts, LDS and scratch sizes, spill counts.  A kernel may live in another
translation unit of the other tree: kernels are matched by name.  `--rename OLD=NEW` (mangled symbols; repeatable) compares kernel OLD of tree A with
kernel NEW of tree B, for a kernel whose symbol changed only because a parameter's type moved to another namespace: its own name inside the text is
replaced before the comparison, and it is listed under NEW.  Exit status 0: the same set of kernels, each in exactly one unit, text and metadata
identical."""
import argparse
import concurrent.futures
import glob
import os
import re
import runpy
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")


def assemble(tree, flags, src, out):
    run = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(tree, "include"), "-o", out, src], capture_output=True, text=True)
    if run.returncode:
        sys.exit(f"{src} does not compile:\n{run.stderr[-4000:]}")
    return open(out).read()


def need(match, what):
    if not match:
        sys.exit(f"the assembly has no {what}: has the compiler's output format changed?")
    return match


def kernels_of(text):
    """{kernel symbol: (normalised instruction text, {metadata})} of one unit's assembly."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    meta = {}
    for block in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s*\d+", text, flags=re.S):
        sym = need(re.search(r"\.symbol:\s*'?([^\s']+?)\.kd'?\s", block), ".symbol in a kernel's metadata").group(1)
        meta[sym] = {k: need(re.search(r"\." + k + r":\s*(\d+)", block), f".{k} for {sym}").group(1) for k in META}
    out = {}
    for name in names:
        m = need(re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M), f"label ... .Lfunc_end for {name}")   # (the kernel descriptor's directives lie inside)
        body = []
        for line in m.group(1).splitlines():
            line = line.split(";", 1)[0].rstrip()
            if line.strip():
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        out[name] = ("\n".join(body), need(meta.get(name), f"metadata for {name}"))
    return out


def tree_kernels(tree, tmp, tag, jobs):
    srcs = sorted(glob.glob(os.path.join(tree, "triton-racer-sim_amd", "csrc", "*.hip")))
    flags = [f for f in runpy.run_path(os.path.join(tree, "__graft_entry__.py"), run_name="kernel_diff")["HIPCC_FLAGS"] if f not in ("-shared", "-fPIC", "-ldl")]
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        texts = list(pool.map(lambda s: assemble(tree, flags, s, os.path.join(tmp, tag + "_" + os.path.basename(s) + ".s")), srcs))
    found = {}                                                     # kernel -> [(unit, text, meta)]
    for src, text in zip(srcs, texts):
        for name, (body, meta) in kernels_of(text).items():
            found.setdefault(name, []).append((os.path.basename(src), body, meta))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("-j", type=int, default=4, help="units compiled at a time")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="kernel OLD of tree A is kernel NEW of tree B (mangled symbols)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a = tree_kernels(os.path.abspath(args.tree_a), tmp, "a", args.j)
        b = tree_kernels(os.path.abspath(args.tree_b), tmp, "b", args.j)
    for pair in args.rename:
        old, _, new = pair.partition("=")
        if old not in a or not new or new in a:
            sys.exit(f"--rename {pair}: tree A has no kernel {old}, or already has {new}")
        a[new] = [(unit, text.replace(old, new), meta) for unit, text, meta in a.pop(old)]
    bad = 0
    print(f"A = {args.tree_a}: {len(a)} kernels | B = {args.tree_b}: {len(b)} kernels")
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"ONLY IN {'A' if name in a else 'B'}  {name}")
            bad += 1
            continue
        if len(a[name]) != 1 or len(b[name]) != 1:
            print(f"DUPLICATE  {name}: A {[u for u, _, _ in a[name]]} B {[u for u, _, _ in b[name]]}")
            bad += 1
            continue
        (ua, ta, ma), (ub, tb, mb) = a[name][0], b[name][0]
        same_text, same_meta = ta == tb, ma == mb
        bad += not (same_text and same_meta)
        where = ua if ua == ub else f"{ua} -> {ub}"
        counts = " ".join(f"{k.replace('_count', '').replace('_segment_fixed_size', '')}={ma[k]}" for k in META)
        print(f"{'same' if same_text and same_meta else 'DIFFERENT'}  {name}  [{where}]  {len(ta.splitlines())} lines  {counts}"
              + ("" if same_text else "  TEXT DIFFERS") + ("" if same_meta else f"  METADATA A {ma} B {mb}"))
    moved = sum(1 for n in a if n in b and len(a[n]) == 1 and len(b[n]) == 1 and a[n][0][0] != b[n][0][0])
    print(f"{len(set(a) & set(b))} kernels in both trees, {moved} in another unit, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
