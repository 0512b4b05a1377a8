#!/usr/bin/env python3
"""What LR_WARP_AREA costs: the area launch against the only thing the code without it can do (the plain warp with the fine
map at the fine size, whose output would still have to be averaged), against the aliased warp straight to the small size, and
end to end; and that a call without the bit runs what it ran.

    python tools/warp_area_timing.py [--out profiles/warp_area.txt] [--sections resources,kernels,plain,e2e,bench]
                                     [--parent-tree DIR] [--reps 20] [--repeats 3]

Sections (each appends to --out):
  resources  no GPU: the four warp translation units compiled with -Rpass-analysis=kernel-resource-usage: VGPRs, SGPRs,
             scratch, LDS and occupancy of the twelve warp_ragged_area_kernel instantiations, none of which may use scratch,
             and of every kernel of kernels_warp.hip, kernels_warp_border.hip and kernels_warp_lens.hip from this tree and
             from --parent-tree (a checkout of the parent commit), which must be equal; exits 1 otherwise.
  kernels    kernel time from `rocprofv3 --kernel-trace`, a run of its own per case and sampling rule, the program after
             `--`: in one process three launches alternating -- the area launch; the plain warp with the fine map into the
             S times larger picture (the same samples, S^2 times the bytes written); the plain warp straight into the small
             picture (2 x 2 or 4 x 4 taps per pixel whatever the shrink: the aliased floor).  Cases: the 3840x2160 u8x3 frame
             of tools/warp_cubic_timing.py under its perspective map, written at a half and at a quarter of its size, and the
             64 mixed colour frames of tools/ragged_batch_timing.py in one ragged launch bounded to 2048 pixels.
  plain      the launch without the bit from --parent-tree's library and from this one, alternating runs of the same kind: the
             kernels are the parent's; the medians beside the span of the parent's medians and beside the min - max of the
             parent's launches.
  e2e        rectify_batch(64 files, jpeg=95) with and without out_max_size=2048, by host clock around the synchronous call,
             alternating; the bytes the pictures hold in HBM and the bytes returned.
  bench      bench.py --gpus 1 --steps 20 --warmup 5 from the parent's tree and from this one, alternating, --repeats runs
             each (nothing bench.py times was touched).
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
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ragged_batch_timing import load_frames, make_bases, one_region  # noqa: E402
from warp_cubic_timing import CASES, CUBIC, WARM, import_package, section_bench, step  # noqa: E402
from warp_timing import perspective  # noqa: E402

AREA = 0x400000
AREA_CASES = ("4k_half", "4k_quarter", "ragged64")
UNITS = ("kernels_warp.hip", "kernels_warp_border.hip", "kernels_warp_lens.hip", "kernels_warp_area.hip")
KERNEL = re.compile(r"(warp_perspective_kernel|warp_ragged_kernel|warp_ragged_border_kernel|warp_ragged_lens_kernel|warp_ragged_area_kernel)<([^>]*)>")
LEGS = ("area", "fine", "small")


def child_kernels(a):
    """per iteration: the area launch, the plain launch with the fine map at the fine size, the plain launch at the small size
    (--legs plain: the plain launch at the full size alone, from --tree's library)"""
    L = import_package(a.tree)
    ctx = L.Context(0)
    ctx.set_seed(0)
    rule = CUBIC if a.rule == "cubic" else 0
    fmt, note = L.PIX_U8X3, ""
    if a.case == "ragged64":
        make_bases(a.inputs)
        host, sources = one_region(load_frames(a.inputs, 64, 1))
        d_src = ctx.device_upload(host)
        _, _, table, d_full, total = ctx.rectify_frames_device(d_src, sources, fmt, max_size=1200)
        assert (table[:, 9] > 0).all()
        plain = lambda: ctx.warp_perspective_ragged_device(d_src, len(host), fmt | rule, table, d_full, total)  # noqa: E731
        if a.legs != "plain":
            Ms, sizes, fines, fine_sizes, factors = [], [], [], [], []
            for row in table:
                _, M, size, S = L.shrink_homography(None, row[:9], (int(row[9]), int(row[10])), 2048)
                Ms.append(M)
                sizes.append(size)
                factors.append(S)
                fines.append(L.area_fine_map(M, S))
                fine_sizes.append((S * size[0], S * size[1]))
            src = np.array(sources, np.int64)
            t_area, small_bytes = L.ragged_table(np.stack(Ms), np.array(sizes, np.int64), src, 3, area=factors)
            t_small = t_area[:, :18]
            t_fine, fine_bytes = L.ragged_table(np.stack(fines), np.array(fine_sizes, np.int64), src, 3)
            d_small, d_fine = ctx.device_upload(np.zeros(small_bytes, np.uint8)), ctx.device_upload(np.zeros(fine_bytes, np.uint8))
            legs = [lambda: ctx.warp_perspective_ragged_device(d_src, len(host), fmt | rule | AREA, t_area, d_small, small_bytes),
                    lambda: ctx.warp_perspective_ragged_device(d_src, len(host), fmt | rule, t_fine, d_fine, fine_bytes),
                    lambda: ctx.warp_perspective_ragged_device(d_src, len(host), fmt | rule, t_small, d_small, small_bytes)]
            note = "factors %s, full %.1f MB, fine %.1f MB, small %.1f MB" % (
                " ".join("%dx%d" % (factors.count(s), s) for s in sorted(set(factors))), total / 1e6, fine_bytes / 1e6, small_bytes / 1e6)
    else:
        w, h, _, bpp = CASES["4k_u8x3"]
        src = np.random.default_rng(0).integers(0, 256, w * h * bpp, dtype=np.uint8)
        d_src = ctx.device_upload(src)
        M = perspective(w, h)
        one = lambda word, m, d, ow, oh: ctx.warp_perspective_device(d_src, src.nbytes, 1, w, h, w * bpp, word, m, d, ow * oh * bpp, ow, oh, ow * bpp)  # noqa: E731
        d_full = ctx.device_upload(np.zeros(src.nbytes, np.uint8))
        plain = lambda: one(fmt | rule, M, d_full, w, h)  # noqa: E731
        if a.legs != "plain":
            _, Ms, (ow, oh), S = L.shrink_homography(None, M, (w, h), w // (2 if a.case == "4k_half" else 4))
            F = L.area_fine_map(Ms, S)
            d_small, d_fine = ctx.device_upload(np.zeros(ow * oh * bpp, np.uint8)), ctx.device_upload(np.zeros(S * ow * S * oh * bpp, np.uint8))
            legs = [lambda: one(fmt | rule | AREA, np.concatenate([Ms.reshape(9), [S]]), d_small, ow, oh),
                    lambda: one(fmt | rule, F, d_fine, S * ow, S * oh),
                    lambda: one(fmt | rule, Ms, d_small, ow, oh)]
            note = "S = %d, %dx%d -> %dx%d, fine %dx%d" % (S, w, h, ow, oh, S * ow, S * oh)
    if a.legs == "plain":
        legs = [plain]
    for _ in range(WARM + a.reps):
        for leg in legs:
            leg()
            ctx.synchronize()
    print("RESULT case=%s legs=%d launches_per_leg=%d %s" % (a.case, len(legs), WARM + a.reps, note))
    ctx.close()


def profiled(a, case, rule, legs, tree, log):
    """([(median, min, max in us) per leg], the child's note) of one rocprofv3 run's trace; the legs alternate launch by launch"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "warp", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "kernels", "--case", case, "--rule", rule, "--legs", legs,
               "--reps", str(a.reps), "--inputs", a.inputs] + (["--tree", tree] if tree else [])
        out = step(cmd, log)
        rows = []
        for s in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for rec in csv.DictReader(open(s)):
                if KERNEL.search(rec["Kernel_Name"]):
                    rows.append((int(rec["Start_Timestamp"]), (int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e3))
    rows.sort()
    m = re.search(r"RESULT case=\S+ legs=(\d+) launches_per_leg=(\d+) ?(.*)", out)
    n, per = int(m.group(1)), int(m.group(2))
    times = [t for _, t in rows][-n * per:]  # (ragged64's run begins with rectify_frames_device's own warp launch)
    assert len(times) == n * per, (len(times), n, per)
    res = []
    for k in range(n):
        v = times[k::n][WARM:]
        res.append((statistics.median(v), min(v), max(v)))
    return res, m.group(3)


def section_kernels(a, log):
    log("\n== kernels: the area launch | the plain warp with the fine map at the fine size (what the code without the bit can do; its output still to be averaged) | the aliased plain warp straight to the small size; alternating in one process, one rocprofv3 --kernel-trace run per case and rule ==")
    log("   (%d timed launches a leg after %d warm-up launches; median us (min - max))" % (a.reps, WARM))
    for case in AREA_CASES:
        for rule in ("linear", "cubic"):
            (ar, fi, sm), note = profiled(a, case, rule, "all", None, log)
            log("  %-10s %-6s area %8.1f (%.1f - %.1f)   fine %8.1f (%.1f - %.1f)   small %8.1f (%.1f - %.1f)   area / fine %.2f   area / small %.2f   [%s]" % (
                case, rule, ar[0], ar[1], ar[2], fi[0], fi[1], fi[2], sm[0], sm[1], sm[2], ar[0] / fi[0], ar[0] / sm[0], note))


def section_plain(a, log):
    if not a.parent_tree:
        raise SystemExit("--sections plain needs --parent-tree")
    log("\n== plain: the launch without the bit at the full size, the parent's library and this tree's, %d runs each, alternating; median us (min - max) of %d launches a run ==" % (a.repeats, a.reps))
    for case, rules in (("4k_half", ("linear", "cubic")), ("ragged64", ("linear",))):
        for rule in rules:
            runs ={"parent": [], "new": []}
            for _ in range(a.repeats):
                for name, tree in (("parent", os.path.abspath(a.parent_tree)), ("new", None)):
                    runs[name].append(profiled(a, case, rule, "plain", tree, log)[0][0])
            span = lambda v: "%s   span of medians %.1f - %.1f" % (" ".join("%.1f (%.1f - %.1f)" % r for r in v), min(r[0] for r in v), max(r[0] for r in v))  # noqa: E731
            lo, hi = min(r[0] for r in runs["parent"]), max(r[0] for r in runs["parent"])
            inside = all(lo <= r[0] <= hi for r in runs["new"])
            lo2, hi2 = min(r[1] for r in runs["parent"]), max(r[2] for r in runs["parent"])
            within = all(lo2 <= r[0] <= hi2 for r in runs["new"])
            log("  %-10s %-6s parent %s" % ("4k_u8x3" if case == "4k_half" else case, rule, span(runs["parent"])))
            log("  %-10s %-6s new    %s   medians inside the span of the parent's medians: %s; inside the parent's launches' min - max (%.1f - %.1f): %s" % (
                "", "", span(runs["new"]), "yes" if inside else "no", lo2, hi2, "yes" if within else "no"))


def child_e2e(a):
    from jpeg_decode_timing import pil_files

    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    make_bases(a.inputs)
    frames = load_frames(a.inputs, 64, 1)
    files = pil_files(frames)
    legs = (("without", None), ("bound", 2048))
    out = {k: ctx.rectify_batch(files, jpeg=95, out_max_size=v) for k, v in legs}  # (warm-up of both)
    held = {}
    for k, v in legs:  # (the bytes the pictures hold in HBM: the packed region the warp writes)
        sizes = []
        for f, r in zip(frames, out[k]):
            if r[2] is None:
                continue
            _, M, size = L.rectification_homography(r[1], 3.0)
            sizes.append(L.shrink_homography(None, M, size, v)[2] if v else size)
        held[k] = L.warp_table(np.stack([np.eye(3)] * len(sizes)), np.array(sizes, np.int64), 3)[1]
    print("NOTE %d files, %.1f MB; pictures in HBM %.1f MB (without), %.1f MB (bound); bytes returned %.1f MB (without), %.1f MB (bound)" % (
        len(files), sum(map(len, files)) / 1e6, held["without"] / 1e6, held["bound"] / 1e6,
        sum(len(x[2]) for x in out["without"] if x[2]) / 1e6, sum(len(x[2]) for x in out["bound"] if x[2]) / 1e6))
    for r in range(a.repeats):
        for k, v in legs:
            t0 = time.perf_counter()
            ctx.rectify_batch(files, jpeg=95, out_max_size=v)
            print("E2E %s %.1f" % (k, (time.perf_counter() - t0) * 1e3))
    ctx.close()


def section_e2e(a, log):
    log("\n== e2e: rectify_batch(64 files, jpeg=95) without and with out_max_size=2048, host clock around the call, alternating ==")
    out = step([sys.executable, os.path.abspath(__file__), "--child", "e2e", "--repeats", str(a.repeats), "--inputs", a.inputs], log)
    for line in out.splitlines():
        if line.startswith("NOTE"):
            log("  " + line[5:])
    for k in ("without", "bound"):
        v = [float(x.split()[2]) for x in out.splitlines() if x.startswith("E2E " + k)]
        log("  %-7s median %7.1f ms  min %7.1f  max %7.1f  runs: %s" % (k, statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))


def resources(tree):
    """{unit: {kernel: (VGPRs, SGPRs, scratch, LDS, occupancy)}} of a tree's warp translation units"""
    sys.path.insert(0, ROOT)
    from librectify_amd import build

    out = {}
    for unit in UNITS:
        src = os.path.join(tree, "librectify_amd", "csrc", unit)
        if not os.path.exists(src):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o", os.path.join(tmp, "w.o")],
                               capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-3000:])
        kernels, name = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                k = KERNEL.search(subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout)
                name = "%s<%s>" % (k.group(1), re.sub(r"\(lr_pixel_format\)|\(bool\)", "", k.group(2))) if k else None
                if name:
                    kernels[name] = {}
            elif name:
                kernels[name][m.group(1).split()[0]] = int(m.group(2))
        out[unit] = {k: (d["VGPRs"], d["TotalSGPRs"], d["ScratchSize"], d["LDS"], d["Occupancy"]) for k, d in kernels.items()}
    return out


def section_resources(a, log):
    if not a.parent_tree:
        raise SystemExit("--sections resources needs --parent-tree")
    log("\n== resources: -Rpass-analysis=kernel-resource-usage for gfx950: VGPRs / SGPRs / scratch bytes a lane / LDS bytes / waves a SIMD ==")
    new, old = resources(ROOT), resources(a.parent_tree)
    fmt = lambda r: "%3d / %3d / %d / %d / %d" % r  # noqa: E731
    log("  kernels_warp_area.hip, warp_ragged_area_kernel<format, cubic, lens> (new):")
    for name, r in sorted(new["kernels_warp_area.hip"].items()):
        log("    %-44s %s" % (name, fmt(r)))
    ok = len(new["kernels_warp_area.hip"]) == 12 and all(r[2] == 0 for r in new["kernels_warp_area.hip"].values())
    log("   twelve instantiations, none with scratch: %s" % ("yes" if ok else "NO"))
    for unit in UNITS[:3]:
        log("  %s, this tree and the parent's:" % unit)
        for name in sorted(set(new[unit]) | set(old[unit])):
            n, o = new[unit].get(name), old[unit].get(name)
            ok = ok and n == o
            log("    %-44s %-26s parent %-26s %s" % (name, fmt(n) if n else "-", fmt(o) if o else "-", "equal" if n == o else "DIFFERENT"))
    log("   every kernel of the three existing code objects has the parent's figures: %s" % ("yes" if ok else "NO"))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_area.txt"))
    ap.add_argument("--sections", default="resources,kernels,plain,e2e,bench")
    ap.add_argument("--parent-tree")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inputs")
    ap.add_argument("--child", choices=("kernels", "e2e"))
    ap.add_argument("--case", choices=AREA_CASES)
    ap.add_argument("--rule", default="linear", choices=("linear", "cubic"))
    ap.add_argument("--legs", default="all", choices=("all", "plain"))
    ap.add_argument("--tree")
    a = ap.parse_args()
    if a.child:
        {"kernels": child_kernels, "e2e": child_e2e}[a.child](a)
        raise SystemExit(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def log(text):
        print(text, flush=True)
        f.write(text + "\n")
        f.flush()

    with tempfile.TemporaryDirectory() as inputs:
        a.inputs = a.inputs or inputs
        for s in a.sections.split(","):
            {"resources": section_resources, "kernels": section_kernels, "plain": section_plain, "e2e": section_e2e, "bench": section_bench}[s](a, log)
