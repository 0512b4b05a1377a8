#!/usr/bin/env python3
"""Timing of the packed warp and of Context.rectify_batch (a tool, not a test).  Needs a GPU; there is no CPU path.

    python tools/rectify_batch_timing.py [--out profiles/rectify_batch.txt] [--batch 64] [--reps 10] [--repeats 3]

Inputs: `batch` frames of 3840x2160 u8x3 and as many of 1920x1080: eight seeded synthetic frames (synth.frame), each
warped on the GPU by eight synthetic tilts, so that the rectified sizes differ from frame to frame.

The parent starts every GPU step as a process of its own under `timeout` and stops at the first that fails:

  * the inputs, in a process of their own that is not profiled: the frames and the table (maps, sizes, places) that
    rectify_batch_device finds for them go to files in a temporary folder, so that the profiled processes launch the
    kernels under test for the measurement alone.
  * the warp stage alone, one `rocprofv3 --kernel-trace --stats` run per way, on that table: (a) "packed", one
    LR_WARP_PACKED launch; (b) "uniform", one launch at the batch's largest size (the batched way there was before);
    (c) "single", one launch per frame.  Kernel time is taken per dispatch from the kernel trace: the warm-up
    repetitions are dropped, a repetition's time is the sum of its launches (one, or for (c) one per frame), and the
    median, minimum and maximum over the repetitions are reported.  The number of dispatches is checked against the
    number the child launched.  Bytes written are the destination's pixel rows.
  * end to end from host arrays with the profiler off: every shape and path is warmed first, then rectify_batch and the
    loop of rectify alternate, `repeats` rounds, with max_size=None and max_size=1200; and the batch's stages (upload,
    prepare + detector + host transform, packed warp, download) timed on their own.

Everything is appended to --out as it is measured.
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"4k": (3840, 2160), "1080p": (1920, 1080)}
STEP_TIMEOUT = 420  # seconds a GPU step may take
WARM = 2  # untimed repetitions before the timed ones in a warp child


def tilted_frames(ctx, L, n, w, h):
    """n u8x3 frames: eight synthetic frames under eight tilts each (a perspective warp on the GPU)"""
    from librectify_amd import synth

    base = []
    for i in range(min(n, 8)):
        g = np.clip(synth.frame(w, h, 500 + i) * 255.0, 0, 255).astype(np.uint8)
        base.append(np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1)))
    out = np.empty((n, h, w, 3), np.uint8)
    for k in range(n):
        t = k // len(base)  # the tilt
        px, py = (1.0e-5 + 2.2e-5 * (t % 4)) * 3840 / w, (0.5e-5 + 2.8e-5 * (t // 4 + t % 3)) * 2160 / h
        sh = 0.02 * t
        M = np.array([[1.0, sh, -0.5 * sh * h], [0.01 * t, 1.0, -0.005 * t * w], [px, py, 1.0 - 0.5 * (px * w + py * h)]])
        out[k] = ctx.warp_perspective(base[k % len(base)], M, (w, h))
    return out


def size_report(table, w, h):
    ow, oh = table[:, 9], table[:, 10]
    have = ow > 0
    px = (ow * oh)[have]
    fill = px.sum() / (have.sum() * ow.max() * oh.max())
    return ("output sizes of %d frames (%d without an image): width %d .. %d, height %d .. %d, pixels %.2f .. %.2f x the source's; "
            "sum(ow*oh) / (B * max ow * max oh) = %.3f" % (len(table), (~have).sum(), ow[have].min(), ow.max(), oh[have].min(), oh.max(),
                                                            px.min() / (w * h), px.max() / (w * h), fill))


def child_inputs(shape, batch, folder):
    """the frames and the table of their rectification, to files (the only place where set-up runs the warp kernels)"""
    import librectify_amd as L

    w, h = SHAPES[shape]
    ctx = L.Context(0)
    ctx.set_seed(0)
    frames = tilted_frames(ctx, L, batch, w, h)
    d_src = ctx.device_upload(frames)
    _, _, table, d_out, total = ctx.rectify_batch_device(d_src, batch, w, h, L.PIX_U8X3, max_size=1200)
    ctx.device_free(d_out)
    ctx.device_free(d_src)
    ctx.close()
    assert (table[:, 9] > 0).all(), "a frame without an image: the three ways would not warp the same frames"
    np.save(os.path.join(folder, "frames.npy"), frames)
    np.save(os.path.join(folder, "table.npy"), table)
    print(size_report(table, w, h) + "; packed output %.1f MB" % (total / 1e6))


def child_warp(shape, way, batch, reps, folder):
    import librectify_amd as L

    w, h = SHAPES[shape]
    ctx = L.Context(0)
    frames, table = np.load(os.path.join(folder, "frames.npy")), np.load(os.path.join(folder, "table.npy"))
    d_src = ctx.device_upload(frames)
    total = int((table[:, 11] + (table[:, 10] - 1) * table[:, 12] + table[:, 9] * 3).max())
    sizes = table[:, 9:11].astype(np.int64)
    mw, mh = int(sizes[:, 0].max()), int(sizes[:, 1].max())
    rows_bytes = int((sizes[:, 0] * sizes[:, 1]).sum()) * 3
    fb = w * h * 3
    import ctypes as C
    p = C.c_void_p()
    nbytes = {"packed": total, "uniform": batch * mw * mh * 3, "single": mw * mh * 3}[way]
    L._check(L.lib().lr_device_malloc(ctx._h, nbytes, C.byref(p)))
    d_dst = p.value
    Ms = np.ascontiguousarray(table[:, :9])

    def run():
        if way == "packed":
            ctx.warp_perspective_packed_device(d_src, fb, batch, w, h, w * 3, L.PIX_U8X3, table, d_dst, total)
        elif way == "uniform":
            ctx.warp_perspective_device(d_src, fb, batch, w, h, w * 3, L.PIX_U8X3, Ms, d_dst, mw * mh * 3, mw, mh, mw * 3)
        else:
            for b in range(batch):
                ow, oh = int(sizes[b, 0]), int(sizes[b, 1])
                ctx.warp_perspective_device(d_src + b * fb, fb, 1, w, h, w * 3, L.PIX_U8X3, Ms[b], d_dst, ow * oh * 3, ow, oh, ow * 3)

    for _ in range(WARM):
        run()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    written = {"packed": rows_bytes, "uniform": batch * mw * mh * 3, "single": rows_bytes}[way]
    print("RESULT way=%s launches_per_rep=%d warm_up_reps=%d timed_reps=%d bytes_written=%d destination_bytes=%d wall_ms_per_rep=%.3f" % (
        way, batch if way == "single" else 1, WARM, reps, written, nbytes if way != "single" else rows_bytes, wall))
    ctx.device_free(d_src)
    ctx.device_free(d_dst)
    ctx.close()


def child_e2e(shape, batch, repeats, folder):
    import librectify_amd as L

    w, h = SHAPES[shape]
    ctx = L.Context(0)
    ctx.set_seed(0)
    frames = np.load(os.path.join(folder, "frames.npy"))
    for max_size in (None, 1200):
        kw = dict(max_size=max_size)
        legs = {"rectify_batch": lambda: ctx.rectify_batch(frames, **kw), "loop of rectify": lambda: [ctx.rectify(f, **kw) for f in frames]}
        res = {k: fn() for k, fn in legs.items()}  # warm-up of both paths at this shape ...
        for b in range(batch):  # ... which also says that they agree
            a, c = res["rectify_batch"][b], res["loop of rectify"][b]
            assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[2], c[2]), "frame %d differs" % b
        del res
        times = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
        print("end to end, %d x %dx%d u8x3 from host arrays, max_size=%s, %d alternating rounds after a warm-up of both:" % (batch, w, h, max_size, repeats))
        for k, v in times.items():
            print("  %-16s median %9.1f ms  min %9.1f  max %9.1f   runs: %s" % (k, statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))
        print("  ratio loop / batch (medians): %.2f" % (statistics.median(times["loop of rectify"]) / statistics.median(times["rectify_batch"])))
        # the batch call's stages, each ended by a wait
        st = {k: [] for k in ("upload", "detector", "warp", "download")}
        for _ in range(repeats):
            t0 = time.perf_counter()
            d_src = ctx.device_upload(frames)
            t1 = time.perf_counter()
            _, _, table, d_out, total = ctx.rectify_batch_device(d_src, batch, w, h, L.PIX_U8X3, **kw)
            ctx.synchronize()
            t2 = time.perf_counter()
            ctx.warp_perspective_packed_device(d_src, w * h * 3, batch, w, h, w * 3, L.PIX_U8X3, table, d_out, total)
            ctx.synchronize()
            t3 = time.perf_counter()
            ctx.device_download(d_out, (total,), np.uint8)
            t4 = time.perf_counter()
            ctx.device_free(d_src)
            ctx.device_free(d_out)
            warp = (t3 - t2) * 1e3
            for k, v in zip(st, ((t1 - t0) * 1e3, (t2 - t1) * 1e3 - warp, warp, (t4 - t3) * 1e3)):
                st[k].append(v)
        med = {k: statistics.median(v) for k, v in st.items()}
        tot = sum(med.values())
        print("  stages of the batch call (medians; detector = prepare + detector batch + host transforms, the warp launch timed by repeating it): "
              + ", ".join("%s %.1f ms (%.0f %%)" % (k, v, 100 * v / tot) for k, v in med.items()))
        print("  " + size_report(table, w, h) + "; packed output %.1f MB" % (total / 1e6))
        sys.stdout.flush()
    ctx.close()


def step(cmd, log):
    """one GPU step: a process of its own under `timeout`; the run stops with the first that fails"""
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def dispatch_times(folder, name):
    """the durations (ns) of the dispatches of the kernel `name`, in start order, from rocprofv3's kernel trace"""
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            rd = csv.DictReader(fh)
            col = {k.lower(): k for k in rd.fieldnames or []}
            if not all(k in col for k in ("kernel_name", "start_timestamp", "end_timestamp")):
                raise SystemExit("unexpected columns in %s: %s" % (path, rd.fieldnames))
            for rec in rd:
                if name in rec[col["kernel_name"]]:
                    rows.append((int(rec[col["start_timestamp"]]), int(rec[col["end_timestamp"]])))
    rows.sort()
    return [e - s for s, e in rows]


def parent(out_path, batch, reps, repeats, shapes):
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(batch), "--reps", str(reps), "--repeats", str(repeats)]
    f = open(out_path, "a")

    def log(text):
        print(text)
        f.write(text + "\n")
        f.flush()

    log("rectify_batch_timing: batch %d, %d timed warp repetitions after %d untimed, %d end-to-end rounds" % (batch, reps, WARM, repeats))
    for shape in shapes:
        w, h = SHAPES[shape]
        with tempfile.TemporaryDirectory() as inputs:
            here = ["--shape", shape, "--inputs", inputs]
            log("\n== warp stage alone, %d x %dx%d u8x3 (kernel times per dispatch: rocprofv3 --kernel-trace --stats, a run per way) ==" % (batch, w, h))
            log("  " + step(me + ["--child", "inputs"] + here, log).strip().splitlines()[-1])
            for way in ("packed", "uniform", "single"):
                with tempfile.TemporaryDirectory() as tmp:
                    out = step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "rb", "--output-format", "csv", "--"] + me + ["--child", "warp", "--way", way] + here, log)
                    # (the packed warp is a launch of the table kernel, warp_ragged_kernel)
                    name = "warp_ragged_kernel" if way == "packed" else "warp_perspective_kernel"
                    other = "warp_perspective_kernel" if way == "packed" else "warp_ragged_kernel"
                    ns, stray = dispatch_times(tmp, name), dispatch_times(tmp, other)
                per = batch if way == "single" else 1
                if len(ns) != (WARM + reps) * per or stray:
                    log("FAILED: the %s run has %d dispatches of %s (expected %d) and %d of %s (expected 0)" % (way, len(ns), name, (WARM + reps) * per, len(stray), other))
                    raise SystemExit(1)
                timed = np.array(ns[WARM * per:], np.float64).reshape(reps, per)
                rep_us = timed.sum(axis=1) / 1e3  # a repetition: the sum of its launches
                res = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1]
                log("  %s: %s" % (way, res[7:]))
                log("      %s, %d dispatches in all, the %d timed repetitions of %d: kernel time per repetition median %.1f us, min %.1f us, max %.1f us"
                    "; a single dispatch %.1f .. %.1f us" % (name, len(ns), reps, per, float(np.median(rep_us)), rep_us.min(), rep_us.max(), timed.min() / 1e3, timed.max() / 1e3))
            log("\n== end to end, %s (profiler off) ==" % shape)
            log(step(me + ["--child", "e2e"] + here, log).rstrip())
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_batch.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="4k,1080p")
    ap.add_argument("--child", choices=["inputs", "warp", "e2e"])
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--way", choices=["packed", "uniform", "single"])
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    a = ap.parse_args()
    if a.child == "inputs":
        child_inputs(a.shape, a.batch, a.inputs)
    elif a.child == "warp":
        child_warp(a.shape, a.way, a.batch, a.reps, a.inputs)
    elif a.child == "e2e":
        child_e2e(a.shape, a.batch, a.repeats, a.inputs)
    else:
        parent(a.out, a.batch, a.reps, a.repeats, a.shapes.split(","))
