#!/usr/bin/env python3
"""Timing of LR_JPEG_OPTIMIZE: the encoder's launches with and without the bit, the bytes and the time of
Context.rectify_batch(jpeg=95) with and without jpeg_optimize, and calls without the bit against the parent commit's (a tool,
not a test).  Needs a GPU.

    python tools/jpeg_optimize_timing.py [--out profiles/jpeg_optimize.txt] [--batch 64] [--reps 5] [--repeats 3]
                                         [--parent TREE] [--sections kernels,e2e,unchanged,bench]

Inputs: jpeg_timing's -- `batch` colour frames drawn with a fixed seed from 3840x2160, 1920x1080, 1600x1200 and 1200x1600,
content from librectify_amd.synth -- and the first 3840x2160 frame of them on its own.

The parent process starts every GPU step as a process of its own under `timeout` and stops at the first that fails:

  * kernels: kernel time per launch, one `rocprofv3 --kernel-trace --stats` run per case ("4k", "list"): per repetition one
    lr_encode_jpeg_device call without the bit and one with it on every frame (quality 95, 4:2:0, extents of lr_jpeg_bound
    with the bit), the same frames, the same process.
  * e2e: the colour list from host arrays with the profiler off, rectify_batch(jpeg=95) and rectify_batch(jpeg=95,
    jpeg_optimize=True): a process per leg and round, alternating; a process warms its leg up once and times one call; the
    bytes that come back beside it.
  * unchanged (needs --parent TREE, a built checkout of the parent commit): the encoder's four launches on the list in a
    call without the bit, a rocprofv3 run per tree and round, alternating.
  * bench (needs --parent): `python bench.py --steps 20 --warmup 5` in the parent's tree and in this one, alternating.

Everything is appended to --out as it is measured.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from jpeg_timing import QUALITY, STEP_TIMEOUT, WARM, case_frames, import_package, spread  # noqa: E402
from ragged_batch_timing import SEED, SIZES, load_frames, make_bases, one_region  # noqa: E402
from rectify_batch_timing import dispatch_times  # noqa: E402

PLAIN = ("jpeg_transform_kernel", "jpeg_entropy_kernel", "jpeg_place_kernel")


def child_kernels(a):
    """who = this: per repetition a call without the bit, then one with it; who = parent (or --plain): without it alone"""
    import ctypes as C

    L = import_package(a.tree)
    ctx = L.Context(0)
    frames = case_frames(a)
    host, sources = one_region(frames)
    src = np.array(sources, np.int64)
    both = a.who == "this" and not a.plain
    caps = np.array([L.jpeg_bound(w, h, L.PIX_U8X3, 0, **({"optimize": True} if both else {})) for w, h, _, _ in sources], np.int64)
    offs = np.concatenate([[0], np.cumsum(caps)])
    extents = np.stack([offs[:-1], caps], axis=1)
    tables = [L.jpeg_table(src[:, :2], src[:, 2:], extents, QUALITY, 0)]
    if both:
        tables.append(L.jpeg_table(src[:, :2], src[:, 2:], extents, QUALITY, 0, optimize=True))
    d_src = ctx.device_upload(host)
    q = C.c_void_p()
    L._check(L.lib().lr_device_malloc(ctx._h, int(offs[-1]), C.byref(q)))
    sizes = []
    for _ in range(WARM + a.reps):
        sizes = [ctx.encode_jpeg_device(d_src, len(host), L.PIX_U8X3, t, q.value, int(offs[-1])) for t in tables]
    assert all((s <= caps.astype(np.uint64)).all() for s in sizes)
    print("RESULT case=%s frames=%d source_bytes=%d stream_bytes=%d optimised_stream_bytes=%d" % (
        a.case, len(frames), len(host), int(sizes[0].sum()), int(sizes[-1].sum()) if both else -1))
    for ptr in (d_src, q.value):
        ctx.device_free(ptr)
    ctx.close()


def child_e2e(a):
    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    frames = load_frames(a.inputs, a.batch, 1)
    kw = {"jpeg_optimize": True} if a.leg == "optimize" else {}
    res = ctx.rectify_batch(frames, jpeg=QUALITY, **kw)  # (warm-up)
    out_bytes = sum(len(r[2]) for r in res if r[2] is not None)
    del res
    t0 = time.perf_counter()
    ctx.rectify_batch(frames, jpeg=QUALITY, **kw)
    print("E2E leg=%s ms=%.1f out_bytes=%d" % (a.leg, (time.perf_counter() - t0) * 1e3, out_bytes))
    ctx.close()


def step(cmd, log, cwd=None):
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True, cwd=cwd)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def medians(tmp, name, per, reps, log):
    """the medians (us) of the `per` dispatches of the kernel in a repetition, in their order"""
    v = dispatch_times(tmp, name)
    if len(v) != (WARM + reps) * per:
        log("FAILED: %d dispatches of %s, expected %d" % (len(v), name, (WARM + reps) * per))
        raise SystemExit(1)
    us = np.array(v[WARM * per:], np.float64).reshape(reps, per) / 1e3
    return [(float(np.median(us[:, k])), float(us[:, k].min()), float(us[:, k].max())) for k in range(per)]


def parent(a):
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--reps", str(a.reps), "--repeats", str(a.repeats)]
    f = open(a.out, "a")

    def log(text):
        print(text)
        f.write(text + "\n")
        f.flush()

    def profiled(args, tmp):
        return step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "jo", "--output-format", "csv", "--"] + me + args, log)

    log("jpeg_optimize_timing: %d colour frames drawn (seed %d) from %s; quality %d, 4:2:0; %d timed kernel repetitions after %d untimed, %d rounds" % (
        a.batch, SEED, ", ".join("%dx%d" % s for s in SIZES), QUALITY, a.reps, WARM, a.repeats))
    sections = a.sections.split(",")
    with tempfile.TemporaryDirectory() as inputs:
        here = ["--inputs", inputs]
        sys.path.insert(0, ROOT)
        make_bases(inputs)
        if "kernels" in sections:
            log("\n== kernel time per launch (rocprofv3 --kernel-trace --stats, a run per case): a call without the bit and a call with it on every frame, alternating in one process ==")
            for case in ("4k", "list"):
                with tempfile.TemporaryDirectory() as tmp:
                    out = profiled(["--child", "kernels", "--case", case] + here, tmp)
                    log("  " + [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][7:])
                    t = medians(tmp, "jpeg_transform_kernel", 2, a.reps, log)
                    e = medians(tmp, "jpeg_entropy_kernel", 4, a.reps, log)
                    p = medians(tmp, "jpeg_place_kernel", 2, a.reps, log)
                    c = medians(tmp, "jpeg_count_kernel", 1, a.reps, log)
                    m = medians(tmp, "jpeg_tables_kernel", 1, a.reps, log)
                    rows = [("without: jpeg_transform_kernel", t[0]), ("without: jpeg_entropy_kernel (lengths)", e[0]), ("without: jpeg_place_kernel", p[0]),
                            ("without: jpeg_entropy_kernel (placement)", e[1]), None,
                            ("with:    jpeg_transform_kernel", t[1]), ("with:    jpeg_count_kernel (new)", c[0]), ("with:    jpeg_tables_kernel (new)", m[0]),
                            ("with:    jpeg_entropy_kernel (lengths, per-frame tables)", e[2]), ("with:    jpeg_place_kernel", p[1]),
                            ("with:    jpeg_entropy_kernel (placement, per-frame tables)", e[3])]
                    total = 0.0
                    for row in rows + [None]:
                        if row is None:
                            log("      %-58s        %9.1f us (sum of the medians)" % ("the call's launches", total))
                            total = 0.0
                            continue
                        log("      %-58s median %9.1f us  min %9.1f  max %9.1f" % ((row[0],) + row[1]))
                        total += row[1][0]
        if "e2e" in sections:
            log("\n== end to end, the colour list from host arrays, max_size=None (profiler off): a process per leg and round, alternating; a process warms up and times one call ==")
            ms, size = {"plain": [], "optimize": []}, {}
            for r in range(a.repeats):
                for leg in ("plain", "optimize"):
                    out = step(me + ["--child", "e2e", "--leg", leg] + here, log)
                    kv = dict(x.split("=") for x in [ln for ln in out.splitlines() if ln.startswith("E2E")][-1].split()[1:])
                    ms[leg].append(float(kv["ms"]))
                    size[leg] = int(kv["out_bytes"])
            for leg, what in (("plain", "rectify_batch(jpeg=%d)" % QUALITY), ("optimize", "rectify_batch(jpeg=%d, jpeg_optimize=True)" % QUALITY)):
                log("    %-44s %s ms; %d bytes come back" % (what, spread(ms[leg]), size[leg]))
            log("    bytes with / without: %.4f" % (size["optimize"] / size["plain"]))
        if a.parent and "unchanged" in sections:
            log("\n== a call without the bit, the list: the encoder's four launches in the parent's tree and in this one (a rocprofv3 run per tree and round, alternating) ==")
            sums = {"parent": [], "this": []}
            for r in range(a.repeats):
                for who, tree in (("parent", a.parent), ("this", ROOT)):
                    with tempfile.TemporaryDirectory() as tmp:
                        profiled(["--child", "kernels", "--case", "list", "--who", who, "--plain", "--tree", tree] + here, tmp)
                        parts = [medians(tmp, n, 2 if n == "jpeg_entropy_kernel" else 1, a.reps, log) for n in PLAIN]
                        sums[who].append(sum(x[0] for part in parts for x in part))
                        log("    %-6s round %d: transform %.1f, lengths %.1f, placement %.1f, places %.1f us" % (who, r, parts[0][0][0], parts[1][0][0], parts[1][1][0], parts[2][0][0]))
            for who in ("parent", "this"):
                log("    %-6s the four launches, us: %s" % (who, spread(sums[who])))
        if a.parent and "bench" in sections:
            log("\n== python bench.py --steps 20 --warmup 5, the parent's tree and this one alternating ==")
            res = {"parent": [], "this": []}
            for r in range(a.repeats):
                for who, tree in (("parent", a.parent), ("this", ROOT)):
                    out = step([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], log, cwd=tree)
                    res[who].append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]))
            keys = [k for k, v in res["this"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
            for k in keys:
                pv, tv = [x[k] for x in res["parent"] if k in x], [x[k] for x in res["this"]]
                if len(pv) == len(tv) and len(set(pv + tv)) > 1:
                    log("  %-34s parent %s" % (k, " ".join("%.4g" % x for x in pv)))
                    log("  %-34s this   %s   medians %.4g / %.4g" % ("", " ".join("%.4g" % x for x in tv), statistics.median(pv), statistics.median(tv)))
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_optimize.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--sections", default="kernels,e2e", help="which of kernels, e2e, unchanged, bench to run (the last two need --parent)")
    ap.add_argument("--child", choices=["kernels", "e2e"])
    ap.add_argument("--case", choices=["4k", "list"], default="4k")
    ap.add_argument("--who", choices=["parent", "this"], default="this")
    ap.add_argument("--plain", action="store_true", help="(kernels child) calls without the bit alone")
    ap.add_argument("--leg", choices=["plain", "optimize"], default="plain")
    ap.add_argument("--tree", help="(kernels child) the tree to import librectify_amd from")
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    a = ap.parse_args()
    if a.child == "kernels":
        child_kernels(a)
    elif a.child == "e2e":
        child_e2e(a)
    else:
        parent(a)
