#!/usr/bin/env python3
"""What LR_WARP_CUBIC costs: the bicubic launch against the bilinear launch on the same frames and maps.

    python tools/warp_cubic_timing.py [--out profiles/warp_cubic.txt] [--sections resources,kernels,parent,e2e,bench]
                                      [--parent-tree DIR] [--reps 30] [--repeats 3]

Sections (each appends to --out):
  resources  no GPU: kernels_warp.hip compiled with -Rpass-analysis=kernel-resource-usage, VGPRs, SGPRs, scratch, LDS and
             occupancy of every instantiation, of this tree and (--parent-tree) of the parent's: the six bilinear
             instantiations must show the parent's figures, the six bicubic ones no scratch.
  kernels    kernel time from `rocprofv3 --kernel-trace --stats`, a run of its own per case, the program after `--`; in one
             run both rules on the same frames and maps.  Cases: tools/warp_timing.py's two (3840x2160 u8x3, 8192x8192 f32,
             its perspective map), the 3840x2160 u8 frame, and the 64 mixed colour frames of tools/ragged_batch_timing.py in
             one ragged launch (tables from rectify_frames_device(max_size=1200), as there).  Per case: the two times, their
             ratio, and the effective rate counting source and output bytes once (both rules move the same bytes: the ratio
             is the price of 16 taps in loads and VALU).
  parent     the bilinear launches of the same cases from the parent's tree (--parent-tree: a checkout of the parent commit
             with its library built) and from this one, alternating, --repeats runs each: the bilinear path must cost what
             it cost, i.e. the difference lies within the parent's own spread ("below": faster by more than that; "ABOVE": slower).
  e2e        rectify_batch(files, jpeg=95, interp="cubic") against interp="linear" on the 64 files of
             tools/jpeg_decode_timing.py, by host clock around the synchronous call, alternating, with the spread.
  bench      bench.py --gpus 1 --steps 20 --warmup 5 from the parent's tree and from this one, alternating, --repeats runs
             each (nothing bench.py times was touched).
Every GPU step is a child process under a time limit; the first that fails ends the run.  Needs a GPU except `resources`.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ragged_batch_timing import load_frames, make_bases, one_region  # noqa: E402
from warp_timing import perspective  # noqa: E402

STEP_TIMEOUT = 420
WARM = 3
CUBIC = 0x8000
CASES = {  # name: (width, height, format, bytes per pixel); "ragged64" is the list of mixed frames
    "4k_u8x3": (3840, 2160, 1, 3),
    "8k_f32": (8192, 8192, 2, 4),
    "4k_u8": (3840, 2160, 0, 1),
    "ragged64": None,
}
KERNEL = re.compile(r"(warp_perspective_kernel|warp_ragged_kernel)<\s*(?:\(lr_pixel_format\))?(\d)\s*(?:,\s*(true|false|\(bool\)[01]|[01])\s*)?>")


def import_package(tree):
    sys.path.insert(0, tree or ROOT)
    import librectify_amd as L

    return L


def child_kernels(a):
    L = import_package(a.tree)
    ctx = L.Context(0)
    ctx.set_seed(0)
    rules = [0 if r == "linear" else CUBIC for r in a.rules.split(",")]
    if a.case == "ragged64":
        make_bases(a.inputs)
        frames = load_frames(a.inputs, 64, 1)
        host, sources = one_region(frames)
        d_src = ctx.device_upload(host)
        _, _, table, d_dst, total = ctx.rectify_frames_device(d_src, sources, L.PIX_U8X3, max_size=1200)
        assert (table[:, 9] > 0).all()
        moved = len(host) + int((table[:, 9] * table[:, 10]).sum()) * 3
        launch = lambda rule: ctx.warp_perspective_ragged_device(d_src, len(host), L.PIX_U8X3 | rule, table, d_dst, total)  # noqa: E731
    else:
        w, h, fmt, bpp = CASES[a.case]
        src = np.random.default_rng(0).integers(0, 256, w * h * bpp, dtype=np.uint8)
        d_src = ctx.device_upload(src)
        d_dst = ctx.device_upload(np.zeros(w * h * bpp, np.uint8))
        M = perspective(w, h)
        moved = 2 * src.nbytes
        launch = lambda rule: ctx.warp_perspective_device(d_src, src.nbytes, 1, w, h, w * bpp, fmt | rule, M, d_dst, src.nbytes, w, h, w * bpp)  # noqa: E731
    for rule in rules:
        for _ in range(WARM + a.reps):
            launch(rule)
            ctx.synchronize()
    print("RESULT case=%s bytes=%d launches_per_rule=%d" % (a.case, moved, WARM + a.reps))
    ctx.device_free(d_src)
    ctx.device_free(d_dst)
    ctx.close()


def child_e2e(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from jpeg_decode_timing import pil_files

    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    make_bases(a.inputs)
    files = pil_files(load_frames(a.inputs, 64, 1))
    legs = ("linear", "cubic")
    out = {k: ctx.rectify_batch(files, jpeg=95, interp=k) for k in legs}  # (warm-up of both)
    print("NOTE %d files, %.1f MB; products %.1f MB (linear), %.1f MB (cubic)" % (
        len(files), sum(map(len, files)) / 1e6, sum(len(x[2]) for x in out["linear"]) / 1e6, sum(len(x[2]) for x in out["cubic"]) / 1e6))
    for r in range(a.repeats):
        for k in legs:
            t0 = time.perf_counter()
            ctx.rectify_batch(files, jpeg=95, interp=k)
            print("E2E %s %.1f" % (k, (time.perf_counter() - t0) * 1e3))
    ctx.close()


def step(cmd, log, cwd=None):
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True, cwd=cwd)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def profiled(a, case, tree, rules, log):
    """{(kernel, format, cubic): (average, min, max) in us} and the bytes a launch moves, from one rocprofv3 run"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "warp", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "kernels", "--case", case, "--rules", rules,
               "--reps", str(a.reps), "--inputs", a.inputs] + (["--tree", tree] if tree else [])
        out = step(cmd, log)
        res = {}
        for s in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for rec in csv.DictReader(open(s)):
                m = KERNEL.search(rec["Name"])
                if m:
                    cubic = m.group(3) in ("true", "(bool)1", "1")
                    res[(m.group(1), int(m.group(2)), cubic)] = (float(rec["AverageNs"]) / 1e3, float(rec["MinNs"]) / 1e3, float(rec["MaxNs"]) / 1e3, int(rec["Calls"]))
    moved = int(re.search(r"RESULT case=\S+ bytes=(\d+)", out).group(1))
    return res, moved


def pick(res, case, cubic):
    name = "warp_ragged_kernel" if case == "ragged64" else "warp_perspective_kernel"
    fmt = 1 if case == "ragged64" else CASES[case][2]
    # (ragged64's run also holds the ragged launch of rectify_frames_device: one bilinear call among the timed ones)
    return res[(name, fmt, cubic)]


def section_kernels(a, log):
    log("\n== kernels: bicubic against bilinear, same frames and maps, one rocprofv3 --kernel-trace --stats run per case ==")
    log("   (%d timed launches a rule after %d warm-up launches, all counted; us; rate = source + output bytes once / average time)" % (a.reps, WARM))
    for case in a.cases.split(","):
        res, moved = profiled(a, case, None, "linear,cubic", log)
        lin, cub = pick(res, case, False), pick(res, case, True)
        log("  %-9s %6.1f MB  bilinear avg %8.1f (min %8.1f max %8.1f) %5.0f GB/s   bicubic avg %8.1f (min %8.1f max %8.1f) %5.0f GB/s   ratio %.2f" % (
            case, moved / 1e6, lin[0], lin[1], lin[2], moved / lin[0] / 1e3, cub[0], cub[1], cub[2], moved / cub[0] / 1e3, cub[0] / lin[0]))


def section_parent(a, log):
    if not a.parent_tree:
        raise SystemExit("--sections parent needs --parent-tree")
    log("\n== parent: the bilinear launch from the parent's tree and from this one, alternating, %d runs each (average us of a run) ==" % a.repeats)
    for case in a.cases.split(","):
        runs = {"parent": [], "new": []}
        for _ in range(a.repeats):
            for name, tree in (("parent", a.parent_tree), ("new", None)):
                res, _ = profiled(a, case, tree, "linear", log)
                runs[name].append(pick(res, case, False)[0])
        p, n = runs["parent"], runs["new"]
        diff = statistics.median(n) - statistics.median(p)
        log("  %-9s parent %s   new %s   median difference %+.1f us, parent's spread %.1f us: %s" % (
            case, " ".join("%8.1f" % v for v in p), " ".join("%8.1f" % v for v in n), diff, max(p) - min(p),
            "within" if abs(diff) <= max(p) - min(p) else ("below" if diff < 0 else "ABOVE")))


def section_e2e(a, log):
    log("\n== e2e: rectify_batch(64 files, jpeg=95), interp linear against cubic, host clock around the call, alternating ==")
    out = step([sys.executable, os.path.abspath(__file__), "--child", "e2e", "--repeats", str(a.repeats), "--inputs", a.inputs], log)
    for line in out.splitlines():
        if line.startswith("NOTE"):
            log("  " + line[5:])
    for k in ("linear", "cubic"):
        v = [float(x.split()[2]) for x in out.splitlines() if x.startswith("E2E " + k)]
        log("  %-7s median %7.1f ms  min %7.1f  max %7.1f  runs: %s" % (k, statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))


def section_bench(a, log):
    if not a.parent_tree:
        raise SystemExit("--sections bench needs --parent-tree")
    log("\n== bench: bench.py --gpus 1 --steps 20 --warmup 5, parent's tree and this one alternating, %d runs each ==" % a.repeats)
    runs = {"parent": [], "new": []}
    for _ in range(a.repeats):
        for name, tree in (("parent", os.path.abspath(a.parent_tree)), ("new", ROOT)):
            out = step([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], log, cwd=tree)
            runs[name].append(json.loads([x for x in out.splitlines() if x.startswith("{")][-1]))
    keys = [k for k, v in runs["new"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
    for k in keys:
        log("  %-28s parent %s   new %s" % (k, " ".join("%10.4g" % r.get(k, float("nan")) for r in runs["parent"]), " ".join("%10.4g" % r[k] for r in runs["new"])))


def resources(tree):
    """{instantiation: (VGPRs, SGPRs, scratch, LDS, occupancy)} of a tree's kernels_warp.hip"""
    sys.path.insert(0, ROOT)
    from librectify_amd import build

    src = os.path.join(tree, "librectify_amd", "csrc", "kernels_warp.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o", os.path.join(tmp, "w.o")],
                           capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-3000:])
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            d = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout
            k = KERNEL.search(d)
            name = "%s<%s, %s>" % (k.group(1), k.group(2), "cubic" if k.group(3) in ("true", "(bool)1", "1") else "linear") if k else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1).split()[0]] = int(m.group(2))
    return out


def section_resources(a, log):
    log("\n== resources: kernels_warp.hip, -Rpass-analysis=kernel-resource-usage (VGPRs, SGPRs, scratch bytes / lane, LDS bytes, waves / SIMD) ==")
    new = resources(ROOT)
    old = resources(a.parent_tree) if a.parent_tree else {}
    fmt = lambda d: "%4d %4d %4d %4d %3d" % (d["VGPRs"], d["TotalSGPRs"], d["ScratchSize"], d["LDS"], d["Occupancy"])  # noqa: E731
    for name in sorted(new):
        line = "  %-42s new %s" % (name, fmt(new[name]))
        if name.endswith("linear>") and old:
            line += "   parent %s   %s" % (fmt(old[name]), "same" if old[name] == new[name] else "DIFFERENT")
        log(line)
    assert all(d["ScratchSize"] == 0 for d in new.values()), "an instantiation uses scratch"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_cubic.txt"))
    ap.add_argument("--sections", default="resources,kernels,e2e")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--parent-tree")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inputs")
    ap.add_argument("--child", choices=("kernels", "e2e"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--rules", default="linear,cubic")
    ap.add_argument("--tree")
    a = ap.parse_args()
    if a.child:
        {"kernels": child_kernels, "e2e": child_e2e}[a.child](a)
        raise SystemExit(0)
    f = open(a.out, "a")

    def log(text):
        print(text, flush=True)
        f.write(text + "\n")
        f.flush()

    with tempfile.TemporaryDirectory() as inputs:
        a.inputs = a.inputs or inputs
        for s in a.sections.split(","):
            {"resources": section_resources, "kernels": section_kernels, "parent": section_parent, "e2e": section_e2e, "bench": section_bench}[s](a, log)
