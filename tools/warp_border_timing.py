#!/usr/bin/env python3
"""What LR_WARP_BORDER costs: each border mode against the same launch without the bit, and the unbordered launch against the
parent's.

    python tools/warp_border_timing.py [--out profiles/warp_border.txt] [--sections resources,kernels,parent]
                                       [--parent-tree DIR] [--reps 20] [--repeats 3]

Sections (each appends to --out):
  resources  no GPU: kernels_warp.hip (and this tree's kernels_warp_border.hip) of this tree and of --parent-tree (a checkout of the parent commit) compiled for gfx950
             with the build's flags, the assembly kept; VGPRs, SGPRs, LDS and scratch of every kernel from the code object's
             metadata (as tools/jpeg_decode_resources.py reads them).  Every kernel of the parent must be there under its own
             name with the parent's four numbers and, comments aside, the parent's instruction stream; exits 1 otherwise.
  kernels    kernel time from `rocprofv3 --kernel-trace`, a run of its own per case and sampling rule, the program
             after `--` (the trace, not --stats: every mode is the same kernel): the launch without the bit, then with the bit and every frame's word naming constant (a non-zero
             value), replicate, reflect, reflect-101.  Cases: tools/warp_cubic_timing.py's four, the single frames under a
             rectifying map that leaves wedges on all four sides.  The figure is each mode's time over the unbordered time.
  parent     the unbordered launches of the same cases from the parent's tree (with its library built) and from this one,
             alternating, --repeats runs each: the difference is read against the parent's own spread.
Every GPU step is a child process under a time limit; the first that fails ends the run.  Needs a GPU except `resources`.
"""
import argparse
import csv
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from warp_cubic_timing import CASES, CUBIC, WARM, import_package, step  # noqa: E402

BORDER = 0x40000
MODES = [("constant", 0), ("replicate", 1), ("reflect", 2), ("reflect101", 4)]
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
KERNEL = re.compile(r"(warp_perspective_kernel|warp_ragged_kernel|warp_ragged_border_kernel)<\s*(?:\(lr_pixel_format\))?(\d)\s*,\s*(true|false|\(bool\)[01]|[01])\s*>")


def wedge_map(L, w, h):
    """(M, (out_width, out_height)) of a rectifying transform whose picture has wedges on all four sides"""
    t = L.ImageTransform()
    t.width, t.height = w, h
    corners = [(-0.06 * w, -0.08 * h), (1.07 * w, -0.03 * h), (0.05 * w, 0.93 * h), (0.94 * w, 0.96 * h)]
    t.top_left, t.top_right, t.bottom_left, t.bottom_right = [L.Point(float(x), float(y), 0.0) for x, y in corners]
    _, M, size = L.rectification_homography(t, 3.0)
    return M, size


def child_kernels(a):
    L = import_package(a.tree)
    ctx = L.Context(0)
    ctx.set_seed(0)
    rule = CUBIC if a.rule == "cubic" else 0
    if a.case == "ragged64":
        from ragged_batch_timing import load_frames, make_bases, one_region

        make_bases(a.inputs)
        host, sources = one_region(load_frames(a.inputs, 64, 1))
        d_src = ctx.device_upload(host)
        _, _, table, d_dst, total = ctx.rectify_frames_device(d_src, sources, L.PIX_U8X3, max_size=1200)
        assert (table[:, 9] > 0).all()
        fmt = L.PIX_U8X3

        def launch(word):
            t = table.copy()
            t[:, 17] = 0 if word is None else word
            ctx.warp_perspective_ragged_device(d_src, len(host), fmt | rule | (0 if word is None else BORDER), t, d_dst, total)
    else:
        w, h, fmt, bpp = CASES[a.case]
        src = np.random.default_rng(0).integers(0, 256, w * h * bpp, dtype=np.uint8)
        if fmt == L.PIX_F32:
            src = np.random.default_rng(0).random(w * h, dtype=np.float32).view(np.uint8)
        M, (ow, oh) = wedge_map(L, w, h)
        d_src = ctx.device_upload(src)
        d_dst = ctx.device_upload(np.zeros(ow * oh * bpp, np.uint8))

        def launch(word):
            m = M.reshape(9) if word is None else np.concatenate([M.reshape(9), [float(word)]])
            ctx.warp_perspective_device(d_src, src.nbytes, 1, w, h, w * bpp, fmt | rule | (0 if word is None else BORDER), m, d_dst, ow * oh * bpp, ow, oh, ow * bpp)
    value = {L.PIX_U8: 255, L.PIX_U8X3: (255, 255, 255), L.PIX_F32: 1.0}[fmt]
    words = [None] + ([] if a.unbordered_only else [L.border_word(("constant", value) if name == "constant" else name, fmt) for name, _ in MODES])
    for k, word in enumerate(words):  # (a leg's launches are consecutive, so the trace's order gives the leg)
        for _ in range(WARM + a.reps):
            launch(word)
            ctx.synchronize()
    print("RESULT case=%s legs=%d launches_per_leg=%d" % (a.case, len(words), WARM + a.reps))
    ctx.device_free(d_src)
    ctx.device_free(d_dst)
    ctx.close()


def profiled(a, case, tree, rule, unbordered_only, log):
    """the legs' kernel times, [(average, min, max) in us] in launch order (unbordered first), from one rocprofv3 run's trace"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "warp", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "kernels", "--case", case, "--rule", rule,
               "--reps", str(a.reps), "--inputs", a.inputs] + (["--tree", tree] if tree else []) + (["--unbordered-only"] if unbordered_only else [])
        out = step(cmd, log)
        rows = []
        for s in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for rec in csv.DictReader(open(s)):
                if KERNEL.search(rec["Kernel_Name"]):
                    rows.append((int(rec["Start_Timestamp"]), (int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e3))
    rows.sort()
    legs, per = int(re.search(r"legs=(\d+)", out).group(1)), WARM + a.reps
    times = [t for _, t in rows][-legs * per:]  # (ragged64's run begins with rectify_frames_device's own warp launch)
    assert len(times) == legs * per, (len(times), legs, per)
    res = []
    for k in range(legs):
        v = times[k * per + WARM: (k + 1) * per]
        res.append((statistics.mean(v), min(v), max(v)))
    return res


def section_kernels(a, log):
    log("\n== kernels: every border mode against the same launch without the bit; one rocprofv3 --kernel-trace run per case and rule ==")
    log("   (%d timed launches a leg after %d warm-up launches; average us (min - max); ratio = mode / unbordered)" % (a.reps, WARM))
    for case in a.cases.split(","):
        for rule in ("linear", "cubic"):
            res = profiled(a, case, None, rule, False, log)
            base = res[0][0]
            line = "  %-9s %-6s unbordered %8.1f (%.1f - %.1f)" % (case, rule, res[0][0], res[0][1], res[0][2])
            for (name, _), r in zip(MODES, res[1:]):
                line += "   %s %8.1f x%.2f" % (name, r[0], r[0] / base)
            log(line)


def section_parent(a, log):
    if not a.parent_tree:
        raise SystemExit("--sections parent needs --parent-tree")
    log("\n== parent: the unbordered bilinear launch from the parent's tree and from this one, alternating, %d runs each (average us of a run) ==" % a.repeats)
    for case in a.cases.split(","):
        runs = {"parent": [], "new": []}
        for _ in range(a.repeats):
            for name, tree in (("parent", a.parent_tree), ("new", None)):
                runs[name].append(profiled(a, case, tree, "linear", True, log)[0][0])
        p, n = runs["parent"], runs["new"]
        diff = statistics.median(n) - statistics.median(p)
        log("  %-9s parent %s   new %s   median difference %+.1f us, parent's spread %.1f us: %s" % (
            case, " ".join("%8.1f" % v for v in p), " ".join("%8.1f" % v for v in n), diff, max(p) - min(p),
            "within" if abs(diff) <= max(p) - min(p) else ("below" if diff < 0 else "ABOVE")))


def resources(tree):
    """{kernel: ((VGPRs, SGPRs, LDS bytes, scratch bytes), instruction stream)} of a tree's warp kernels"""
    sys.path.insert(0, ROOT)
    from librectify_amd import build

    text = ""
    for unit in ("kernels_warp.hip", "kernels_warp_border.hip"):  # (the second: this tree's bordered kernels, a code object of their own)
        src = os.path.join(tree, "librectify_amd", "csrc", unit)
        if not os.path.exists(src):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.check_call([build._hipcc()] + build.FLAGS + ["-x", "hip", "-c", src, "-o", os.path.join(tmp, "w.o"), "-save-temps=obj"], cwd=tmp)
            asm = [f for f in os.listdir(tmp) if f.endswith(".s") and "amdgcn" in f]
            with open(os.path.join(tmp, asm[0])) as f:
                text += "\n" + f.read()
    out = {}
    for entry in re.split(r"\n  - \.agpr_count", text)[1:]:
        get = lambda key: re.search(r"\.%s:\s*(\S+)" % key, entry).group(1)  # noqa: E731
        symbol = get("name")
        k = KERNEL.search(subprocess.run(["c++filt", symbol], capture_output=True, text=True, check=True).stdout)
        if not k:
            continue
        name = "%s<%s, %s>" % (k.group(1), k.group(2), "cubic" if k.group(3) in ("true", "(bool)1", "1") else "linear")
        body = re.search(r"\n%s:[^\n]*\n(.*?)\n\.Lfunc_end" % re.escape(symbol), text, re.S).group(1)
        # (comments off; a local label .LBB<function>_<block> without the function's number, which counts the kernels before it)
        stream = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*", "", line)).strip() for line in body.splitlines()]
        out[name] = (tuple(int(get(f)) for f in FIELDS), [line for line in stream if line])
    return out


def section_resources(a, log):
    if not a.parent_tree:
        raise SystemExit("--sections resources needs --parent-tree")
    log("\n== resources: kernels_warp.hip for gfx950, from the code objects' metadata: VGPRs / SGPRs / LDS bytes / scratch bytes ==")
    new, old = resources(ROOT), resources(a.parent_tree)
    fmt = lambda r: "%3d / %3d / %5d / %d" % r  # noqa: E731
    same = True
    for name in sorted(new):
        now, stream = new[name]
        line = "  %-40s %-24s" % (name, fmt(now))
        if name in old:
            equal, lines = old[name][0] == now, old[name][1] == stream
            same = same and equal and lines
            line += " parent %-24s %s; %d instructions and labels, %s" % (fmt(old[name][0]), "equal" if equal else "DIFFERENT", len(stream),
                                                                     "the parent's line for line" if lines else "NOT the parent's (%d)" % len(old[name][1]))
        else:
            line += " (new)"
        log(line)
    same = same and all(name in new for name in old)
    log("   every kernel of the parent is here with the parent's numbers and instruction stream: %s" % ("yes" if same else "NO"))
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_border.txt"))
    ap.add_argument("--sections", default="resources,kernels,parent")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--parent-tree")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inputs")
    ap.add_argument("--child", choices=("kernels",))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--rule", default="linear", choices=("linear", "cubic"))
    ap.add_argument("--unbordered-only", action="store_true")
    ap.add_argument("--tree")
    a = ap.parse_args()
    if a.child:
        child_kernels(a)
        raise SystemExit(0)
    f = open(a.out, "a")

    def log(text):
        print(text, flush=True)
        f.write(text + "\n")
        f.flush()

    with tempfile.TemporaryDirectory() as inputs:
        a.inputs = a.inputs or inputs
        for s in a.sections.split(","):
            {"resources": section_resources, "kernels": section_kernels, "parent": section_parent}[s](a, log)
