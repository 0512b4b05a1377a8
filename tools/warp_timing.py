#!/usr/bin/env python3
"""Kernel time of lr_warp_perspective_device from rocprofv3 (--kernel-trace --stats), in a run of its own per case.

    python tools/warp_timing.py [--out profiles] [--reps 100]

Cases: a 3840x2160 u8x3 frame to a same-size output under a perspective map ("4k_u8x3"), and an 8192x8192 f32 frame
to a same-size output under the same kind of map ("8k_f32").  For each, the parent starts
`rocprofv3 --kernel-trace --stats -- python tools/warp_timing.py --child CASE` and writes <out>/warp_CASE.txt: the
kernel's average time over the timed launches (and min / max), and the effective rate counting the source frame's and
the output's bytes once.  Needs a GPU; there is no CPU path.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {  # name: (width, height, format, bytes per pixel)
    "4k_u8x3": (3840, 2160, 1, 3),
    "8k_f32": (8192, 8192, 2, 4),
}


def perspective(w, h):
    """a rectification-like destination -> source map that keeps most of the output inside the source"""
    return np.array([[1.0, 0.08, -0.012 * w], [0.02, 1.0, -0.014 * h], [1.5e-5 * 3840 / w, 2.0e-5 * 2160 / h, 1.0]])


def child(case, reps):
    import librectify_amd as L

    w, h, fmt, bpp = CASES[case]
    ctx = L.Context(0)
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, w * h * bpp, dtype=np.uint8)
    d_src = ctx.device_upload(src)
    d_dst = ctx.device_upload(np.zeros(w * h * bpp, np.uint8))
    M = perspective(w, h)
    for _ in range(5):  # warm-up
        ctx.warp_perspective_device(d_src, src.nbytes, 1, w, h, w * bpp, fmt, M, d_dst, src.nbytes, w, h, w * bpp)
    ctx.synchronize()
    for _ in range(reps):
        ctx.warp_perspective_device(d_src, src.nbytes, 1, w, h, w * bpp, fmt, M, d_dst, src.nbytes, w, h, w * bpp)
    ctx.synchronize()
    out = ctx.device_download(d_dst, (h, w * bpp), np.uint8)
    print("%s: %d launches, %.1f %% of the output non-zero" % (case, reps + 5, 100.0 * np.count_nonzero(out) / out.size))
    ctx.device_free(d_src)
    ctx.device_free(d_dst)
    ctx.close()


def parent(out_dir, reps):
    os.makedirs(out_dir, exist_ok=True)
    for case, (w, h, fmt, bpp) in CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "warp", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
                raise SystemExit("rocprofv3 run of %s failed with %d" % (case, r.returncode))
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise SystemExit("no kernel_stats.csv from rocprofv3 for %s" % case)
            row = None
            for s in stats:
                for rec in csv.DictReader(open(s)):
                    if "warp_perspective_kernel" in rec["Name"]:
                        row = rec
            with open(stats[0]) as f, open(os.path.join(out_dir, "warp_%s_kernel_stats.csv" % case), "w") as g:
                g.write(f.read())
            if row is None:
                raise SystemExit("the warp kernel is not in the stats of %s" % case)
        avg_us = float(row["AverageNs"]) / 1e3
        mb = 2.0 * w * h * bpp / 1e6  # source frame + output, once each
        text = "\n".join([
            "warp_perspective_kernel, case %s: %dx%d, %d bytes per pixel, same-size output, perspective map" % (case, w, h, bpp),
            "command: rocprofv3 --kernel-trace --stats -- python tools/warp_timing.py --child %s --reps %d" % (case, reps),
            "launches: %s" % row["Calls"],
            "kernel time: average %.2f us, min %.2f us, max %.2f us" % (avg_us, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3),
            "bytes counted (source + destination once): %.1f MB" % mb,
            "effective rate: %.0f GB/s (average), %.0f GB/s (min time)" % (mb * 1e3 / avg_us, mb * 1e3 / (float(row["MinNs"]) / 1e3)),
            "child output: " + r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "",
        ]) + "\n"
        with open(os.path.join(out_dir, "warp_%s.txt" % case), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--child", choices=sorted(CASES))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
    else:
        parent(a.out, a.reps)
