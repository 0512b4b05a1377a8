#!/usr/bin/env python3
"""Timing of the mixed-size batch: the ragged prepare and warp launches, the batch detector with a frame table and
Context.rectify_batch on a list of frames of different shapes (a tool, not a test).  Needs a GPU; there is no CPU path.

    python tools/ragged_batch_timing.py [--out profiles/ragged_batch.txt] [--batch 64] [--reps 5] [--repeats 3]
                                        [--parent TREE]

Inputs: `batch` frames drawn with a fixed seed from four sizes (3840x2160, 1920x1080, 1600x1200 and 1200x1600 portrait),
content from librectify_amd.synth (two frames per size, rolled by a few pixels from copy to copy), gray and colour.

The parent process starts every GPU step as a process of its own under `timeout` and stops at the first that fails:

  * the inputs: the base frames and, per colour mode, the tables (prepared sizes, maps, output sizes and places) that
    rectify_frames_device finds go to files in a temporary folder, so that the profiled processes launch the kernels
    under test for the measurement alone.
  * the two new launches against what they replace, one `rocprofv3 --kernel-trace --stats` run per way and colour mode:
    "ragged" is one LR_WARP_RAGGED | LR_WARP_PREPARE launch and one LR_WARP_RAGGED launch per repetition, "single" one
    LR_WARP_PREPARE launch and one warp launch per frame.  Kernel time is taken per dispatch from the kernel trace; the
    warm-up repetitions are dropped and a repetition's time is the sum of its launches.
  * the detector call with a frame table, frames in list order against decreasing pixel count, alternating (host clock
    around the call, which ends synchronised), with max_size=None (the 8-bit frames) and 1200 (the prepared ones).
  * end to end from host arrays with the profiler off, after a warm-up of every path: rectify_batch on the list and a
    loop of Context.rectify alternate, `repeats` rounds, with max_size=None and 1200.  With --parent TREE (a built
    checkout of the parent commit) the same loop also runs there, in processes of its own before and after.

Everything is appended to --out as it is measured.
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(3840, 2160), (1920, 1080), (1600, 1200), (1200, 1600)]
STEP_TIMEOUT = 300  # seconds a GPU step may take
WARM = 2  # untimed repetitions before the timed ones in a profiled child
SEED = 20261017


def import_package(tree):
    sys.path.insert(0, tree or ROOT)
    import librectify_amd as L

    return L


def make_bases(folder):
    from librectify_amd import synth

    bases = {}
    for s, (w, h) in enumerate(SIZES):
        for v in range(2):
            bases["s%d_%d" % (s, v)] = np.clip(synth.frame(w, h, 900 + 10 * s + v) * 255.0, 0, 255).astype(np.uint8)
    np.savez(os.path.join(folder, "bases.npz"), **bases)


def load_frames(folder, batch, colour):
    """the list of frames: sizes drawn with the fixed seed, copy k of a base frame rolled by (7k, 13k) pixels"""
    bases = np.load(os.path.join(folder, "bases.npz"))
    pick = np.random.default_rng(SEED).integers(0, len(SIZES), batch)
    frames = []
    for k, s in enumerate(pick):
        g = np.roll(bases["s%d_%d" % (s, k % 2)], (7 * k, 13 * k), (0, 1))
        frames.append(np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1)) if colour else np.ascontiguousarray(g))
    return frames


def one_region(frames):
    """all frames in one host buffer, as rectify_batch lays them out: (bytes, sources)"""
    bpp = 3 if frames[0].ndim == 3 else 1
    sources, end = [], 0
    for f in frames:
        start = (end + 3) // 4 * 4
        sources.append((f.shape[1], f.shape[0], start, f.shape[1] * bpp))
        end = start + f.nbytes
    host = np.zeros(end, np.uint8)
    for f, (_, _, start, _) in zip(frames, sources):
        host[start: start + f.nbytes] = f.reshape(-1)
    return host, sources


def child_inputs(a):
    L = import_package(None)
    make_bases(a.inputs)
    ctx = L.Context(0)
    ctx.set_seed(0)
    for colour in (0, 1):
        frames = load_frames(a.inputs, a.batch, colour)
        host, sources = one_region(frames)
        fmt, bpp = (L.PIX_U8X3, 3) if colour else (L.PIX_U8, 1)
        d = ctx.device_upload(host)
        _, _, table, d_out, total = ctx.rectify_frames_device(d, sources, fmt, max_size=1200)
        ctx.device_free(d_out)
        ctx.device_free(d)
        assert (table[:, 9] > 0).all(), "a frame without an image: the two ways would not warp the same frames"
        prepared = np.array([L.prepared_size(w, h, 1200)[:2] for w, h, _, _ in sources], np.int64)
        ptable, ptotal = L.ragged_table(None, prepared, np.array(sources, np.int64), bpp, out_bpp=4)
        np.savez(os.path.join(a.inputs, "tables%d.npz" % colour), warp=table, prepare=ptable)
        sizes = sorted({(w, h) for w, h, _, _ in sources})
        print("colour=%d: %d frames, %s; source region %.1f MB, prepared %.1f MB, rectified %.1f MB" % (
            colour, len(frames), ", ".join("%d of %dx%d" % (sum(1 for s in sources if s[:2] == z), z[0], z[1]) for z in sizes), len(host) / 1e6, ptotal / 1e6, total / 1e6))
    ctx.close()


def child_kernels(a):
    import ctypes as C

    L = import_package(None)
    ctx = L.Context(0)
    colour = a.colour
    frames = load_frames(a.inputs, a.batch, colour)
    host, sources = one_region(frames)
    fmt, bpp = (L.PIX_U8X3, 3) if colour else (L.PIX_U8, 1)
    t = np.load(os.path.join(a.inputs, "tables%d.npz" % colour))
    table, ptable = t["warp"], t["prepare"]
    total = int((table[:, 11] + (table[:, 10] - 1) * table[:, 12] + table[:, 9] * bpp).max())
    ptotal = int((ptable[:, 11] + (ptable[:, 10] - 1) * ptable[:, 12] + ptable[:, 9] * 4).max())
    d_src = ctx.device_upload(host)
    p, q = C.c_void_p(), C.c_void_p()
    L._check(L.lib().lr_device_malloc(ctx._h, total, C.byref(p)))
    L._check(L.lib().lr_device_malloc(ctx._h, ptotal, C.byref(q)))

    def run():
        if a.way == "ragged":
            ctx.prepare_ragged_device(d_src, len(host), fmt, ptable, q.value, ptotal)
            ctx.warp_perspective_ragged_device(d_src, len(host), fmt, table, p.value, total)
        else:
            for b, (w, h, off, row) in enumerate(sources):
                ow, oh, o, r = (int(v) for v in ptable[b, 9:13])
                ctx.prepare_device(d_src + off, 0, 1, w, h, row, fmt, q.value + o, 0, ow, oh, r)
            for b, (w, h, off, row) in enumerate(sources):
                ow, oh, o, r = (int(v) for v in table[b, 9:13])
                ctx.warp_perspective_device(d_src + off, 0, 1, w, h, row, fmt, table[b, :9].copy(), p.value + o, 0, ow, oh, r)

    for _ in range(WARM + a.reps):
        run()
        ctx.synchronize()
    print("RESULT way=%s colour=%d launches_per_rep_and_stage=%d source_bytes=%d prepared_bytes=%d warped_bytes=%d" % (
        a.way, colour, 1 if a.way == "ragged" else len(sources), len(host), int((ptable[:, 9] * ptable[:, 10]).sum()) * 4, int((table[:, 9] * table[:, 10]).sum()) * bpp))
    for ptr in (d_src, p.value, q.value):
        ctx.device_free(ptr)
    ctx.close()


def child_order(a):
    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    for colour in (0, 1):
        frames = load_frames(a.inputs, a.batch, colour)
        host, sources = one_region(frames)
        fmt, bpp = (L.PIX_U8X3, 3) if colour else (L.PIX_U8, 1)
        d_src = ctx.device_upload(host)
        rows = {None: [(d_src + off, w, h, row // bpp, max(w, h) / 100.0) for w, h, off, row in sources]}
        ptable = np.load(os.path.join(a.inputs, "tables%d.npz" % colour))["prepare"]
        ptotal = int((ptable[:, 11] + (ptable[:, 10] - 1) * ptable[:, 12] + ptable[:, 9] * 4).max())
        d_small = ctx.device_upload(np.zeros(ptotal, np.uint8))
        ctx.prepare_ragged_device(d_src, len(host), fmt, ptable, d_small, ptotal)
        ctx.synchronize()
        rows[1200] = [(d_small + int(r[11]), int(r[9]), int(r[10]), int(r[12]) // 4, max(r[9], r[10]) / 100.0) for r in ptable]
        for max_size, rr in rows.items():
            order = sorted(range(len(rr)), key=lambda b: -rr[b][1] * rr[b][2])
            legs = {"list order": rr, "decreasing pixel count": [rr[b] for b in order]}
            det_fmt = fmt if max_size is None else L.PIX_F32
            res = {k: ctx.find_line_segment_groups_frames_device(v, det_fmt, 0.0)[0] for k, v in legs.items()}  # (warm-up)
            assert all(res["list order"][b].tobytes() == res["decreasing pixel count"][i].tobytes() for i, b in enumerate(order)), "the order changed a result"
            times = {k: [] for k in legs}
            for _ in range(a.repeats * 2):
                for k, v in legs.items():
                    t0 = time.perf_counter()
                    ctx.find_line_segment_groups_frames_device(v, det_fmt, 0.0)
                    times[k].append((time.perf_counter() - t0) * 1e3)
            print("detector call with a frame table, %d frames, colour=%d, max_size=%s, %d alternating rounds after a warm-up:" % (len(rr), colour, max_size, a.repeats * 2))
            for k, v in times.items():
                print("  %-24s median %8.2f ms  min %8.2f  max %8.2f   runs: %s" % (k, statistics.median(v), min(v), max(v), " ".join("%.2f" % x for x in v)))
        ctx.device_free(d_src)
        ctx.device_free(d_small)
    ctx.close()


def child_e2e(a):
    """who = both: rectify_batch on the list and the loop of rectify alternate; who = loop: the loop alone (what a tree
    without the mixed-size batch can run)"""
    L = import_package(a.tree)
    ctx = L.Context(0)
    ctx.set_seed(0)
    for colour in (0, 1):
        frames = load_frames(a.inputs, a.batch, colour)
        for max_size in (None, 1200):
            kw = dict(max_size=max_size)
            legs = {"loop of rectify": lambda: [ctx.rectify(f, **kw) for f in frames]}
            if a.who == "both":
                legs["rectify_batch"] = lambda: ctx.rectify_batch(frames, **kw)
            res = {k: fn() for k, fn in legs.items()}  # warm-up of the paths at these shapes ...
            if a.who == "both":  # ... which also says that they agree
                for b, (x, y) in enumerate(zip(res["rectify_batch"], res["loop of rectify"])):
                    assert x[0].tobytes() == y[0].tobytes() and bytes(x[1]) == bytes(y[1]) and np.array_equal(x[2], y[2]), "frame %d differs" % b
            del res
            times = {k: [] for k in legs}
            for _ in range(a.repeats):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    fn()
                    times[k].append((time.perf_counter() - t0) * 1e3)
            print("end to end, %d mixed frames, colour=%d, max_size=%s, from host arrays, %d rounds after a warm-up (%s):" % (len(frames), colour, max_size, a.repeats, a.label))
            for k, v in times.items():
                print("  %-16s median %9.1f ms  min %9.1f  max %9.1f   per frame %.3f ms   runs: %s" % (k, statistics.median(v), min(v), max(v), statistics.median(v) / len(frames), " ".join("%.1f" % x for x in v)))
            if a.who == "both":
                print("  ratio loop / batch (medians, this tree): %.2f" % (statistics.median(times["loop of rectify"]) / statistics.median(times["rectify_batch"])))
            sys.stdout.flush()
    ctx.close()


def step(cmd, log):
    """one GPU step: a process of its own under `timeout`; the run stops with the first that fails"""
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def parent(a):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from rectify_batch_timing import dispatch_times

    me = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--reps", str(a.reps), "--repeats", str(a.repeats)]
    f = open(a.out, "a")

    def log(text):
        print(text)
        f.write(text + "\n")
        f.flush()

    log("ragged_batch_timing: %d frames drawn (seed %d) from %s; %d timed kernel repetitions after %d untimed, %d end-to-end rounds" % (
        a.batch, SEED, ", ".join("%dx%d" % s for s in SIZES), a.reps, WARM, a.repeats))
    with tempfile.TemporaryDirectory() as inputs:
        here = ["--inputs", inputs]
        log(step(me + ["--child", "inputs"] + here, log).rstrip())
        log("\n== the new launches against the single-frame launches they replace (kernel time per dispatch: rocprofv3 --kernel-trace --stats, a run per way) ==")
        for colour in (0, 1):
            for way in ("ragged", "single"):
                with tempfile.TemporaryDirectory() as tmp:
                    out = step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "rg", "--output-format", "csv", "--"] + me + ["--child", "kernels", "--way", way, "--colour", str(colour)] + here, log)
                    names = ("prepare_ragged_kernel", "warp_ragged_kernel") if way == "ragged" else ("prepare_kernel", "warp_perspective_kernel")
                    ns = [dispatch_times(tmp, n) for n in names]
                per = 1 if way == "ragged" else a.batch
                log("  " + [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][7:])
                for n, v in zip(names, ns):
                    if len(v) != (WARM + a.reps) * per:
                        log("FAILED: %d dispatches of %s, expected %d" % (len(v), n, (WARM + a.reps) * per))
                        raise SystemExit(1)
                    rep_us = np.array(v[WARM * per:], np.float64).reshape(a.reps, per).sum(axis=1) / 1e3
                    log("      %-24s %d launches a repetition: kernel time per repetition median %.1f us, min %.1f, max %.1f" % (n, per, float(np.median(rep_us)), rep_us.min(), rep_us.max()))
        log("\n== the detector call: frames in list order against decreasing pixel count (profiler off) ==")
        log(step(me + ["--child", "order"] + here, log).rstrip())
        log("\n== end to end (profiler off) ==")
        loop_parent = me + ["--child", "e2e", "--who", "loop", "--tree", a.parent or "", "--label", "the parent commit's tree"] + here
        if a.parent:
            log(step(loop_parent, log).rstrip())
        log(step(me + ["--child", "e2e", "--who", "both", "--label", "this tree"] + here, log).rstrip())
        if a.parent:
            log(step(loop_parent, log).rstrip())
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_batch.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", help="a built checkout of the parent commit: the loop of Context.rectify also runs there")
    ap.add_argument("--child", choices=["inputs", "kernels", "order", "e2e"])
    ap.add_argument("--way", choices=["ragged", "single"])
    ap.add_argument("--colour", type=int, default=0)
    ap.add_argument("--who", choices=["both", "loop"], default="both")
    ap.add_argument("--tree", help="(e2e child) the tree to import librectify_amd from")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    a = ap.parse_args()
    if a.child == "inputs":
        child_inputs(a)
    elif a.child == "kernels":
        child_kernels(a)
    elif a.child == "order":
        child_order(a)
    elif a.child == "e2e":
        child_e2e(a)
    else:
        parent(a)
