#!/usr/bin/env python3
"""Kernel time of the prepare step (lr_warp_perspective_device with LR_WARP_PREPARE) from rocprofv3 (--kernel-trace
--stats), in a run of its own per case, beside a device-to-device copy of the same source bytes in the same process; and
the wall time of Context.rectify(frame, max_size=1200) beside the same result without the device prepare step.

    python tools/prepare_timing.py [--out profiles] [--reps 100] [--runs 21]

Kernel cases: 3840x2160 u8x3, u8 and f32 to 1200x675, 8192x8192 u8 to 1200x1200.  For each, the parent starts
`rocprofv3 --kernel-trace --stats -- python tools/prepare_timing.py --child CASE` and writes <out>/prepare_CASE.txt: the
kernel's average time over the launches (and min / max), the bytes it has to move (source once + output once) and the
rate, and the copy's time by HIP events around the timed copies (and from the trace where the copy is a kernel there).
The copy moves 2 bytes per source byte, the prepare kernel about 1.1.
End to end (<out>/prepare_end_to_end.txt, no profiler): a 3840x2160 u8x3 frame, median of --runs alternated runs after
warm-up of (a) Context.rectify(frame, max_size=1200) and (b) the same lines, transform and picture the way the library
offered before: the prescale on the host (tests/numpy_prepare_ref.py, NumPy), the f32 frame uploaded, detection, endpoints
scaled back, transform, warp of the uploaded 8-bit frame.  Needs a GPU; there is no CPU path.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {  # name: (width, height, format, bytes per pixel, output width, output height)
    "4k_u8x3": (3840, 2160, 1, 3, 1200, 675),
    "4k_u8": (3840, 2160, 0, 1, 1200, 675),
    "4k_f32": (3840, 2160, 2, 4, 1200, 675),
    "8k_u8": (8192, 8192, 0, 1, 1200, 1200),
}


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    h.hipEventSynchronize.argtypes = [C.c_void_p]
    h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    return h


def child(case, reps):
    import librectify_amd as L

    w, h, fmt, bpp, ow, oh = CASES[case]
    ctx = L.Context(0)
    rng = np.random.default_rng(0)
    if fmt == 2:
        src = rng.random(w * h, dtype=np.float32)
    else:
        src = rng.integers(0, 256, w * h * bpp, dtype=np.uint8)
    d_src = ctx.device_upload(src)
    d_copy = ctx.device_upload(np.zeros(src.nbytes, np.uint8))
    d_dst = ctx.device_upload(np.zeros(ow * oh, np.float32))
    run = lambda: ctx.prepare_device(d_src, src.nbytes, 1, w, h, w * bpp, fmt, d_dst, ow * oh * 4, ow, oh, ow * 4)  # noqa: E731
    for _ in range(5):  # warm-up
        run()
    ctx.synchronize()
    for _ in range(reps):
        run()
    ctx.synchronize()
    out = ctx.device_download(d_dst, (oh, ow), np.float32)
    # the copy: same bytes, device to device, on the null stream, timed by events around all of them
    H = hip()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert H.hipEventCreate(C.byref(e)) == 0
    copy = lambda: H.hipMemcpyAsync(C.c_void_p(d_copy), C.c_void_p(d_src), src.nbytes, 3, None)  # noqa: E731 (3 = device to device)
    for _ in range(5):
        assert copy() == 0
    assert H.hipEventRecord(ev[0], None) == 0
    for _ in range(reps):
        assert copy() == 0
    assert H.hipEventRecord(ev[1], None) == 0 and H.hipEventSynchronize(ev[1]) == 0
    ms = C.c_float(0)
    assert H.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
    print("%s: %d launches, output mean %.6f, copy_us_by_events %.3f" % (case, reps + 5, float(out.mean()), ms.value * 1e3 / reps))
    for p in (d_src, d_copy, d_dst):
        ctx.device_free(p)
    ctx.close()


def kernel_cases(out_dir, reps):
    for case, (w, h, fmt, bpp, ow, oh) in CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "prepare", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
                raise SystemExit("rocprofv3 run of %s failed with %d" % (case, r.returncode))
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise SystemExit("no kernel_stats.csv from rocprofv3 for %s" % case)
            row, copy_row = None, None
            for s in stats:
                for rec in csv.DictReader(open(s)):
                    if "prepare_kernel" in rec["Name"]:
                        row = rec
                    elif "copy" in rec["Name"].lower() and int(rec["Calls"]) >= reps:
                        copy_row = rec
            with open(stats[0]) as f, open(os.path.join(out_dir, "prepare_%s_kernel_stats.csv" % case), "w") as g:
                g.write(f.read())
            if row is None:
                raise SystemExit("the prepare kernel is not in the stats of %s" % case)
        last = r.stdout.strip().splitlines()[-1]
        copy_us = float(last.rsplit("copy_us_by_events", 1)[1])
        avg_us, min_us = float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3
        src_mb, dst_mb = w * h * bpp / 1e6, ow * oh * 4 / 1e6
        lines = [
            "prepare_kernel, case %s: %dx%d, %d bytes per pixel, to %dx%d f32" % (case, w, h, bpp, ow, oh),
            "command: rocprofv3 --kernel-trace --stats -- python tools/prepare_timing.py --child %s --reps %d" % (case, reps),
            "launches: %s" % row["Calls"],
            "kernel time: average %.2f us, min %.2f us, max %.2f us" % (avg_us, min_us, float(row["MaxNs"]) / 1e3),
            "bytes counted (source once + destination once): %.1f + %.1f MB" % (src_mb, dst_mb),
            "effective rate: %.0f GB/s (average), %.0f GB/s (min time)" % ((src_mb + dst_mb) * 1e3 / avg_us, (src_mb + dst_mb) * 1e3 / min_us),
            "device-to-device hipMemcpyAsync of the source's %.1f MB, same process: %.2f us a copy by HIP events around %d copies "
            "= %.0f GB/s counting read + write" % (src_mb, copy_us, reps, 2 * src_mb * 1e3 / copy_us),
        ]
        if copy_row is not None:
            lines.append("the copy in the trace (%s): average %.2f us, min %.2f us over %s calls" % (
                copy_row["Name"][:60], float(copy_row["AverageNs"]) / 1e3, float(copy_row["MinNs"]) / 1e3, copy_row["Calls"]))
        lines.append("prepare kernel / copy: %.2f" % (avg_us / (float(copy_row["AverageNs"]) / 1e3 if copy_row is not None else copy_us)))
        lines.append("child output: " + last)
        text = "\n".join(lines) + "\n"
        with open(os.path.join(out_dir, "prepare_%s.txt" % case), "w") as f:
            f.write(text)
        print(text, flush=True)


def end_to_end(out_dir, runs):
    import librectify_amd as L
    from librectify_amd import synth

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy_prepare_ref as P

    w, h, max_size = 3840, 2160, 1200
    g = np.clip(synth.frame(w, h, 3) * 255.0, 0, 255).astype(np.uint8)
    rgb = np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))
    ctx = L.Context(0)
    ctx.set_seed(0)
    ow, oh, scale = L.prepared_size(w, h, max_size)
    cfg = L.RectificationConfig(hmin=2.0)

    def device_way():
        return ctx.rectify(rgb, max_size=max_size)

    def host_way(parts=None):
        t0 = time.perf_counter()
        small = P.prepare(rgb, ow, oh)
        t1 = time.perf_counter()
        lines = ctx.find_line_segment_groups(small, max(ow, oh) / 100.0)
        for k in ("x1", "y1", "x2", "y2"):
            lines[k] = lines[k] / scale
        t = L.compute_rectification_transform(lines, w, h, cfg)
        _, M, size = L.rectification_homography(t, 3.0)
        out = lines, t, ctx.warp_perspective(rgb, M, size)
        if parts is not None:
            parts.append((t1 - t0, time.perf_counter() - t1))
        return out

    a, b = device_way(), host_way()
    same = a[0].tobytes() == b[0].tobytes() and (a[1].as_array() == b[1].as_array()).all() and (a[2] == b[2]).all()
    for _ in range(2):
        device_way(), host_way()
    td, th, parts = [], [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        device_way()
        td.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        host_way(parts)
        th.append(time.perf_counter() - t0)
    ms = lambda v: 1e3 * float(np.median(v))  # noqa: E731
    text = "\n".join([
        "Context.rectify end to end, 3840x2160 u8x3 synthetic frame, max_size=1200 (%dx%d, scale %g), %d segments" % (ow, oh, float(scale), len(a[0])),
        "results of the two ways identical (lines, transform, picture): %s" % same,
        "alternated runs after 3 warm-up pairs: %d; wall time by time.perf_counter (every call ends in a download)" % runs,
        "device prepare (u8 frame up once, prepare + detect + warp on the device): median %.2f ms (min %.2f, max %.2f)" % (ms(td), 1e3 * min(td), 1e3 * max(td)),
        "host prescale (tests/numpy_prepare_ref.py in NumPy, f32 frame up, detect, u8 frame up, warp): median %.2f ms (min %.2f, max %.2f)" % (ms(th), 1e3 * min(th), 1e3 * max(th)),
        "  of which the NumPy prescale: median %.2f ms; everything after it: median %.2f ms" % (ms([p[0] for p in parts]), ms([p[1] for p in parts])),
    ]) + "\n"
    with open(os.path.join(out_dir, "prepare_end_to_end.txt"), "w") as f:
        f.write(text)
    print(text, flush=True)
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--child", choices=sorted(CASES))
    ap.add_argument("--only", choices=["kernels", "end_to_end"])
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
    else:
        os.makedirs(a.out, exist_ok=True)
        if a.only != "end_to_end":
            kernel_cases(a.out, a.reps)
        if a.only != "kernels":
            end_to_end(a.out, a.runs)
