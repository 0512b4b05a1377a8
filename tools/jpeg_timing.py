#!/usr/bin/env python3
"""Timing of the JPEG encoder: its launches beside the identity warp at the same size, and Context.rectify_batch(jpeg=95)
against the parent commit's rectify_batch, which brings raw pictures back (a tool, not a test).  Needs a GPU.

    python tools/jpeg_timing.py [--out profiles/jpeg.txt] [--batch 64] [--reps 5] [--repeats 3] [--parent TREE] [--sections kernels,e2e,bench]

Inputs: ragged_batch_timing's -- `batch` colour frames drawn with a fixed seed from 3840x2160, 1920x1080, 1600x1200 and
1200x1600, content from librectify_amd.synth -- and the first 3840x2160 frame of them on its own.

The parent process starts every GPU step as a process of its own under `timeout` and stops at the first that fails:

  * kernel time per launch, one `rocprofv3 --kernel-trace --stats` run per case ("4k": one 3840x2160 colour frame; "list":
    the mixed colour list): per repetition one identity warp of the u8x3 frames (the yardstick: it reads and writes every
    pixel once) and one lr_encode_jpeg_device call (quality 95, 4:2:0, extents of lr_jpeg_bound) on the same frames.
  * end to end from host arrays with the profiler off, the colour list with max_size=None and 1200: processes of the parent
    commit's tree (--parent TREE, a built checkout: rectify_batch, raw pictures) and of this tree (rectify_batch(jpeg=95),
    and rectify_batch raw) alternate, `repeats` rounds; a process warms its path up once and times one call.
  * section bench (not run by default): `python bench.py --steps 20 --warmup 5` in the parent's tree and in this one,
    alternating, `repeats` runs each.

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
from ragged_batch_timing import SEED, SIZES, load_frames, make_bases, one_region  # noqa: E402
from rectify_batch_timing import dispatch_times  # noqa: E402

STEP_TIMEOUT = 420
WARM = 2
QUALITY = 95


def import_package(tree):
    sys.path.insert(0, tree or ROOT)
    import librectify_amd as L

    return L


def case_frames(a):
    frames = load_frames(a.inputs, a.batch, 1)
    if a.case == "4k":
        frames = [next(f for f in frames if f.shape[:2] == (2160, 3840))]
    return frames


def child_kernels(a):
    import ctypes as C

    L = import_package(None)
    ctx = L.Context(0)
    frames = case_frames(a)
    host, sources = one_region(frames)
    src = np.array(sources, np.int64)
    wtable, wtotal = L.ragged_table(None, src[:, :2], src, 3)
    caps = np.array([L.jpeg_bound(w, h, L.PIX_U8X3, 0) for w, h, _, _ in sources], np.int64)
    offs = np.concatenate([[0], np.cumsum(caps)])
    jtable = L.jpeg_table(src[:, :2], src[:, 2:], np.stack([offs[:-1], caps], axis=1), QUALITY, 0)
    d_src = ctx.device_upload(host)
    p, q = C.c_void_p(), C.c_void_p()
    L._check(L.lib().lr_device_malloc(ctx._h, wtotal, C.byref(p)))
    L._check(L.lib().lr_device_malloc(ctx._h, int(offs[-1]), C.byref(q)))
    sizes = None
    for _ in range(WARM + a.reps):
        ctx.warp_perspective_ragged_device(d_src, len(host), L.PIX_U8X3, wtable, p.value, wtotal)
        ctx.synchronize()
        sizes = ctx.encode_jpeg_device(d_src, len(host), L.PIX_U8X3, jtable, q.value, int(offs[-1]))
    assert (sizes <= caps.astype(np.uint64)).all()
    print("RESULT case=%s frames=%d source_bytes=%d stream_bytes=%d extent_bytes=%d" % (a.case, len(frames), len(host), int(sizes.sum()), int(offs[-1])))
    for ptr in (d_src, p.value, q.value):
        ctx.device_free(ptr)
    ctx.close()


def child_e2e(a):
    """who = parent: rectify_batch (raw pictures) in the tree given; who = this: rectify_batch(jpeg=95), then rectify_batch"""
    L = import_package(a.tree)
    ctx = L.Context(0)
    ctx.set_seed(0)
    frames = load_frames(a.inputs, a.batch, 1)
    for max_size in (None, 1200):
        legs = {"raw": lambda: ctx.rectify_batch(frames, max_size=max_size)}
        if a.who == "this":
            legs = {"jpeg": lambda: ctx.rectify_batch(frames, max_size=max_size, jpeg=QUALITY), "raw": legs["raw"]}
        for name, fn in legs.items():
            res = fn()  # (warm-up)
            out_bytes = sum(len(r[2]) if isinstance(r[2], bytes) else r[2].nbytes for r in res if r[2] is not None)
            del res
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
            print("E2E who=%s leg=%s max_size=%s ms=%.1f out_bytes=%d" % (a.who, name, max_size, ms, out_bytes))
            sys.stdout.flush()
    ctx.close()


def step(cmd, log, cwd=None):
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True, cwd=cwd)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def spread(v):
    return "median %.1f  min %.1f  max %.1f  (spread %.1f %% of the median)  runs: %s" % (
        statistics.median(v), min(v), max(v), 100.0 * (max(v) - min(v)) / statistics.median(v), " ".join("%.1f" % x for x in v))


def parent(a):
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--reps", str(a.reps), "--repeats", str(a.repeats)]
    f = open(a.out, "a")

    def log(text):
        print(text)
        f.write(text + "\n")
        f.flush()

    log("jpeg_timing: %d colour frames drawn (seed %d) from %s; quality %d, 4:2:0; %d timed kernel repetitions after %d untimed, %d end-to-end rounds" % (
        a.batch, SEED, ", ".join("%dx%d" % s for s in SIZES), QUALITY, a.reps, WARM, a.repeats))
    with tempfile.TemporaryDirectory() as inputs:
        here = ["--inputs", inputs]
        sys.path.insert(0, ROOT)
        sections = a.sections.split(",")
        if "kernels" in sections or "e2e" in sections:
            make_bases(inputs)
        if "kernels" in sections:
          log("\n== kernel time per launch (rocprofv3 --kernel-trace --stats, a run per case); the u8x3 identity warp of the same frames beside it ==")
          for case in ("4k", "list"):
              with tempfile.TemporaryDirectory() as tmp:
                  out = step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "jp", "--output-format", "csv", "--"] + me + ["--child", "kernels", "--case", case] + here, log)
                  log("  " + [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][7:])
                  total = 0.0
                  for name in ("warp_ragged_kernel", "jpeg_transform_kernel", "jpeg_entropy_kernel", "jpeg_place_kernel"):
                      v = dispatch_times(tmp, name)
                      per = 2 if name == "jpeg_entropy_kernel" else 1  # (the lengths pass and the placement pass)
                      if len(v) != (WARM + a.reps) * per:
                          log("FAILED: %d dispatches of %s, expected %d" % (len(v), name, (WARM + a.reps) * per))
                          raise SystemExit(1)
                      us = np.array(v[WARM * per:], np.float64).reshape(a.reps, per) / 1e3
                      for k in range(per):
                          label = name + ("" if per == 1 else (" (lengths)" if k == 0 else " (placement)"))
                          log("      %-40s median %9.1f us  min %9.1f  max %9.1f" % (label, float(np.median(us[:, k])), us[:, k].min(), us[:, k].max()))
                          if name != "warp_ragged_kernel":
                              total += float(np.median(us[:, k]))
                  log("      %-40s        %9.1f us (sum of the medians)" % ("the encoder's four launches", total))
        if a.parent and "e2e" in sections:
            log("\n== end to end, the colour list from host arrays (profiler off): a process per tree and round, alternating; a process warms up and times one call ==")
            times = {}
            for r in range(a.repeats):
                for who, tree in (("parent", a.parent), ("this", "")):
                    out = step(me + ["--child", "e2e", "--who", who, "--tree", tree] + here, log)
                    for ln in out.splitlines():
                        if ln.startswith("E2E"):
                            kv = dict(x.split("=") for x in ln.split()[1:])
                            times.setdefault((kv["max_size"], kv["who"], kv["leg"]), []).append(float(kv["ms"]))
                            times[(kv["max_size"], kv["who"], kv["leg"], "bytes")] = int(kv["out_bytes"])
            for max_size in ("None", "1200"):
                log("  max_size=%s:" % max_size)
                for who, leg, what in (("parent", "raw", "the parent's rectify_batch (raw pictures)"), ("this", "raw", "this tree's rectify_batch (raw pictures)"),
                                       ("this", "jpeg", "this tree's rectify_batch(jpeg=%d)" % QUALITY)):
                    v = times[(max_size, who, leg)]
                    log("    %-44s %s ms; %.1f MB come back" % (what, spread(v), times[(max_size, who, leg, "bytes")] / 1e6))
                p, j = times[(max_size, "parent", "raw")], times[(max_size, "this", "jpeg")]
                log("    jpeg=%d against the parent: %.2f x (medians); the parent's own spread is %.1f %% of its median" % (
                    QUALITY, statistics.median(p) / statistics.median(j), 100.0 * (max(p) - min(p)) / statistics.median(p)))
        if a.parent and "bench" in sections:
            log("\n== python bench.py --steps 20 --warmup 5, the parent's tree and this one alternating ==")
            res = {"parent": [], "this": []}
            for r in range(a.repeats):
                for who, tree in (("parent", a.parent), ("this", ROOT)):
                    out = step([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], log, cwd=tree)
                    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
                    res[who].append(line)
            keys = [k for k, v in res["this"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
            for k in keys:
                pv, tv = [x[k] for x in res["parent"] if k in x], [x[k] for x in res["this"]]
                if len(pv) == len(tv) and len(set(pv + tv)) > 1:
                    log("  %-34s parent %s" % (k, " ".join("%.4g" % x for x in pv)))
                    log("  %-34s this   %s   medians %.4g / %.4g" % ("", " ".join("%.4g" % x for x in tv), statistics.median(pv), statistics.median(tv)))
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--sections", default="kernels,e2e", help="which of kernels, e2e, bench to run (e2e and bench need --parent)")
    ap.add_argument("--child", choices=["kernels", "e2e"])
    ap.add_argument("--case", choices=["4k", "list"], default="4k")
    ap.add_argument("--who", choices=["parent", "this"], default="this")
    ap.add_argument("--tree", help="(e2e child) the tree to import librectify_amd from")
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    a = ap.parse_args()
    if a.child == "kernels":
        child_kernels(a)
    elif a.child == "e2e":
        child_e2e(a)
    else:
        parent(a)
