#!/usr/bin/env python3
"""Timing of LR_JPEG_ANY_SAMPLING in the JPEG decoder (a tool, not a test).  Needs a GPU and PIL.

    python tools/jpeg_decode_sampling_timing.py --parent-tree DIR [--out profiles/jpeg_decode_sampling.txt] [--batch 64] [--reps 5] [--runs 3]

DIR is a built checkout of the parent commit (python -m librectify_amd.build in it); without it the comparison with the
parent is left out.

Inputs: jpeg_decode_timing's -- `batch` colour frames drawn with a fixed seed from 3840x2160, 1920x1080, 1600x1200 and
1200x1600, content from librectify_amd.synth, at quality 95 without restart markers -- as PIL's 4:2:0 files, and the same
frames as 4:4:0 and 4:1:1 files from the writer of tools/make_jpeg_sampling_fixtures.py (16 processes).

  * without the bit: kernel time per stage of one lr_decode_jpeg_device call on the 4:2:0 files, the parent commit's library
    and this one's alternating, `runs` profiled processes each (`rocprofv3 --kernel-trace --stats`, a process of its own
    under `timeout` per run; each run's figure is the median of `reps` calls after 2 untimed).  The yardstick is the
    parent's own spread over its runs: this commit's median of runs must lie inside it.
  * with the bit on the same files: what the general instantiations cost on content the special ones could have taken
    (the library takes them only when a frame needs them, so here a 4:4:0 file of 16 x 16 is appended to the list).
  * the 4:4:0 and the 4:1:1 set with the bit, per stage; beside it PIL decoding each set on 16 threads.

Everything is appended to --out as it is measured.
"""
import argparse
import io
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ragged_batch_timing import SEED, SIZES, import_package, load_frames, make_bases  # noqa: E402
from rectify_batch_timing import dispatch_times  # noqa: E402

STEP_TIMEOUT = 300
WARM = 2
QUALITY = 95
THREADS = 16
ANY_SAMPLING = 0x20000
KERNELS = ("jd_sync_kernel", "jd_place_kernel", "jd_write_kernel", "jd_dc_kernel", "jd_transform_kernel", "jd_output_kernel")
SETS = {"420": None, "440": (0x12, 0x11, 0x11), "411": (0x41, 0x11, 0x11)}


def _written(args):
    import make_jpeg_sampling_fixtures as F

    frame, sampling = args
    return F.encode(frame, sampling, QUALITY)


def make_sets(folder, batch):
    """<set>.npz in the folder: the files one behind the other, their lengths, the pictures' sizes"""
    from PIL import Image

    sys.path.insert(0, ROOT)
    make_bases(folder)
    frames = load_frames(folder, batch, 1)

    def pil(f):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=QUALITY, subsampling=2)
        return buf.getvalue()

    tiny = _written((np.full((16, 16, 3), 128, np.uint8), SETS["440"]))
    for name, sampling in SETS.items():
        if sampling is None:
            with ThreadPoolExecutor(THREADS) as pool:
                files = list(pool.map(pil, frames))
        else:
            with ProcessPoolExecutor(THREADS) as pool:
                files = list(pool.map(_written, [(f, sampling) for f in frames]))
        sizes = [f.shape[1::-1] for f in frames]
        np.savez(os.path.join(folder, name + ".npz"), region=np.frombuffer(b"".join(files), np.uint8), lens=np.array([len(s) for s in files], np.int64),
                 sizes=np.array(sizes, np.int64))
        if name == "420":  # the same list with one small file that needs the general instantiations
            np.savez(os.path.join(folder, "420+.npz"), region=np.frombuffer(b"".join(files + [tiny]), np.uint8),
                     lens=np.array([len(s) for s in files + [tiny]], np.int64), sizes=np.array(sizes + [(16, 16)], np.int64))


def load_set(folder, name):
    z = np.load(os.path.join(folder, name + ".npz"))
    return z["region"], z["lens"], z["sizes"]


def child_kernels(a):
    import ctypes as C

    L = import_package(a.tree)
    ctx = L.Context(0)
    region, lens, sizes = load_set(a.inputs, a.set)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    places = np.concatenate([[0], np.cumsum((sizes[:, 0] * sizes[:, 1] * 3 + 3) // 4 * 4)]).astype(np.int64)
    table = L.jpeg_decode_table(np.stack([offs, lens], axis=1), np.stack([places[:-1], sizes[:, 0] * 3], axis=1), sizes)
    d_src = ctx.device_upload(region)
    d_dst = C.c_void_p()
    L._check(L.lib().lr_device_malloc(ctx._h, int(places[-1]), C.byref(d_dst)))
    fmt = L.PIX_U8X3 | (ANY_SAMPLING if a.bit else 0)
    for _ in range(WARM + a.reps):
        info = ctx.decode_jpeg_device(d_src, region, fmt, table, d_dst.value, int(places[-1]))
    assert not info[:, 5].any(), info[:, 5]
    print("RESULT frames=%d file_bytes=%d pixel_bytes=%d most_decodes_of_a_part=%d..%d" % (
        len(lens), len(region), int(places[-1]), int(info[:, 6].min()), int(info[:, 6].max())))
    ctx.device_free(d_src)
    ctx.device_free(d_dst.value)
    ctx.close()


def step(cmd, log):
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def profiled(a, log, inputs, tree, name, bit):
    """one profiled process: {kernel: median us of a call's launches of it, "all": their sum}, and the child's RESULT line"""
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", "kernels", "--inputs", inputs, "--set", name, "--bit", str(int(bit))]
    with tempfile.TemporaryDirectory() as tmp:
        out = step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "jd", "--output-format", "csv", "--"] + me + (["--tree", tree] if tree else []), log)
        got, calls = {}, WARM + a.reps
        for k in KERNELS:
            v = dispatch_times(tmp, k)
            if not v or len(v) % calls:
                log("FAILED: %d dispatches of %s in %d calls" % (len(v), k, calls))
                raise SystemExit(1)
            got[k] = float(np.median(np.array(v, np.float64).reshape(calls, len(v) // calls)[WARM:].sum(axis=1) / 1e3))
    got["all"] = sum(got[k] for k in KERNELS)
    return got, [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][7:]


def table(log, runs, label):
    for k in KERNELS + ("all",):
        v = [r[k] for r in runs]
        log("      %-22s %-20s median %9.1f us  min %9.1f  max %9.1f   runs: %s" % (
            "the decoder's launches" if k == "all" else k, label, statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))


def parent(a):
    f = open(a.out, "a")

    def log(text):
        print(text)
        f.write(text + "\n")
        f.flush()

    log("\njpeg_decode_sampling_timing: %d colour frames drawn (seed %d) from %s, quality %d, no DRI; per run the median of %d calls after %d untimed; %d runs where runs are compared" % (
        a.batch, SEED, ", ".join("%dx%d" % s for s in SIZES), QUALITY, a.reps, WARM, a.runs))
    with tempfile.TemporaryDirectory() as inputs:
        t0 = time.perf_counter()
        make_sets(inputs, a.batch)
        log("  (the three sets of files written in %.0f s)" % (time.perf_counter() - t0))
        log("\n== without the bit, PIL's 4:2:0 files: kernel time per lr_decode_jpeg_device call (rocprofv3 --kernel-trace --stats), alternating ==")
        old, new = [], []
        for _ in range(a.runs):
            if a.parent_tree:
                old.append(profiled(a, log, inputs, a.parent_tree, "420", False)[0])
            got, result = profiled(a, log, inputs, None, "420", False)
            new.append(got)
        log("  " + result)
        if old:
            table(log, old, "parent commit")
        table(log, new, "this commit")
        if old:
            for k in KERNELS + ("all",):
                lo, hi, mid = min(r[k] for r in old), max(r[k] for r in old), statistics.median(r[k] for r in new)
                where = "inside" if lo <= mid <= hi else ("ABOVE it, slower by %.2f %%" % (100.0 * (mid - hi) / hi) if mid > hi else "below it, faster by %.2f %%" % (100.0 * (lo - mid) / lo))
                log("      %-22s the parent's runs span %9.1f .. %9.1f us; this commit's median %9.1f us lies %s" % ("the decoder's launches" if k == "all" else k, lo, hi, mid, where))
        log("\n== with the bit, the same files and one 16 x 16 4:4:0 file that makes the call take the general instantiations ==")
        got, result = profiled(a, log, inputs, None, "420+", True)
        log("  " + result)
        table(log, [got], "this commit, the bit")
        for name in ("440", "411"):
            log("\n== with the bit, the same frames as 4:%s:%s files ==" % (name[1], name[2]))
            got, result = profiled(a, log, inputs, None, name, True)
            log("  " + result)
            table(log, [got], "this commit, the bit")
        log("\n== PIL decoding each set on %d threads (to RGB arrays) ==" % THREADS)
        from PIL import Image

        for name in ("420", "440", "411"):
            region, lens, _ = load_set(inputs, name)
            ends = np.cumsum(lens)
            files = [region[e - n:e].tobytes() for e, n in zip(ends, lens)]
            ms = []
            for _ in range(a.runs + 1):
                t0 = time.perf_counter()
                with ThreadPoolExecutor(THREADS) as pool:
                    list(pool.map(lambda s: np.asarray(Image.open(io.BytesIO(s)).convert("RGB")), files))
                ms.append((time.perf_counter() - t0) * 1e3)
            log("      4:%s:%s  %d files, %d bytes: median %.1f ms  min %.1f  max %.1f (after one warm-up)" % (
                name[1], name[2], len(files), len(region), statistics.median(ms[1:]), min(ms[1:]), max(ms[1:])))
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_sampling.txt"))
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child", choices=["kernels"])
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    ap.add_argument("--set", help="(children) the set of files")
    ap.add_argument("--bit", type=int, default=0, help="(children) 1: with LR_JPEG_ANY_SAMPLING")
    ap.add_argument("--tree", help="(children) the checkout whose library is loaded")
    a = ap.parse_args()
    if a.child == "kernels":
        child_kernels(a)
    else:
        parent(a)
