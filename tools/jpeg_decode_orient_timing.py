#!/usr/bin/env python3
"""Timing of the EXIF orientation in the JPEG decoder's output pass against what it replaces (a tool, not a test): kernel
time per launch of the decoder's chain, jpeg_decode_timing's inputs and method, this tree and the parent commit's in one
session.  Needs a GPU, PIL and a built checkout of the parent commit.

    python tools/jpeg_decode_orient_timing.py --parent ../parent_checkout [--out profiles/jpeg_decode_orient.txt]
                                              [--batch 64] [--reps 5] [--rounds 2]

Inputs: jpeg_decode_timing's -- `batch` colour frames drawn with a fixed seed from 3840x2160, 1920x1080, 1600x1200 and
1200x1600 as the files PIL writes of them at quality 95, 4:2:0, no restart markers; for the oriented leg the same files with
an Exif segment of orientation 6 behind SOI.  The files are written once and every leg reads the same bytes.

Every leg is one `rocprofv3 --kernel-trace --stats` run in a process of its own under `timeout`, WARM untimed and `reps`
timed lr_decode_jpeg_device calls on the list; a leg's figure is the median over its calls of the sum of the call's
launches.  The four legs run `rounds` times, one after the other, so that the file shows the spread between runs of one leg:

  (a) parent, as stored        the parent commit's library, entry [7] = 0
  (b) branch, as stored        this tree's library, entry [7] = 0
  (c) branch, oriented         this tree's library, the files of orientation 6, entry [7] = 1
  (d) parent, the workaround   the parent's decode of the same pictures plus one LR_WARP_RAGGED launch with the rotation's
                               map (destination to source: x' = y, y' = h - 1 - x) over them into a second buffer
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jpeg_decode_timing import KERNELS, QUALITY, STEP_TIMEOUT, WARM, pil_files  # noqa: E402
from ragged_batch_timing import SEED, SIZES, load_frames, make_bases  # noqa: E402
from rectify_batch_timing import dispatch_times  # noqa: E402

LEGS = [("a", "parent", "stored", "(a) parent, as stored"), ("b", "branch", "stored", "(b) branch, as stored"),
        ("c", "branch", "oriented", "(c) branch, oriented (6)"), ("d", "parent", "workaround", "(d) parent, decode + rotating warp")]
WARP = "warp_ragged_kernel"


def child(a):
    import ctypes as C

    sys.path.insert(0, a.tree)
    import librectify_amd as L

    assert os.path.abspath(os.path.dirname(os.path.dirname(L.__file__))) == os.path.abspath(a.tree)
    saved = np.load(os.path.join(a.inputs, "files.npz"))
    lens = saved["lens"].astype(np.int64)
    ends = np.cumsum(lens)
    files = [saved["data"][e - n:e].tobytes() for e, n in zip(ends, lens)]
    oriented = a.way == "oriented"
    if oriented:
        import numpy_jpeg_orient_ref as X

        files = [X.with_exif(s, 6) for s in files]
        lens = np.array([len(s) for s in files], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    region = np.frombuffer(b"".join(files), np.uint8)
    kw = dict(orient=True) if oriented else {}
    probe = L.jpeg_info(files, **kw)
    sizes = probe[:, :2].astype(np.int64)
    places = np.concatenate([[0], np.cumsum((sizes[:, 0] * sizes[:, 1] * 3 + 3) // 4 * 4)]).astype(np.int64)
    total = int(places[-1])
    table = L.jpeg_decode_table(np.stack([offs, lens], axis=1), np.stack([places[:-1], sizes[:, 0] * 3], axis=1), sizes, **kw)
    ctx = L.Context(0)
    d_src = ctx.device_upload(region)
    d_dst, d_turned = C.c_void_p(), C.c_void_p()
    L._check(L.lib().lr_device_malloc(ctx._h, total, C.byref(d_dst)))
    if a.way == "workaround":
        maps = np.array([[[0, 1, 0], [-1, 0, h - 1], [0, 0, 1]] for _, h in sizes.tolist()], np.float64)
        sources = np.stack([sizes[:, 0], sizes[:, 1], places[:-1], sizes[:, 0] * 3], axis=1)
        wtable, wtotal = L.ragged_table(maps, sizes[:, ::-1], sources, 3)
        L._check(L.lib().lr_device_malloc(ctx._h, wtotal, C.byref(d_turned)))
    for _ in range(WARM + a.reps):
        info = ctx.decode_jpeg_device(d_src, region, L.PIX_U8X3, table, d_dst.value, total)
        if a.way == "workaround":
            ctx.warp_perspective_ragged_device(d_dst.value, total, L.PIX_U8X3, wtable, d_turned.value, wtotal)
            ctx.synchronize()
    assert not info[:, 5].any() and (not oriented or (info[:, 7] == 6).all())
    print("RESULT frames=%d file_bytes=%d pixel_bytes=%d" % (len(files), len(region), total))
    for p in (d_src, d_dst.value, d_turned.value):
        if p:
            ctx.device_free(p)
    ctx.close()


def step(cmd, log):
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def parent(a):
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps)]
    f = open(a.out, "a")

    def log(text):
        print(text)
        f.write(text + "\n")
        f.flush()

    trees = {"parent": os.path.abspath(a.parent), "branch": ROOT}
    calls = WARM + a.reps
    log("jpeg_decode_orient_timing: %d colour frames drawn (seed %d) from %s, as PIL's files at quality %d, 4:2:0, no DRI; per leg and round "
        "one rocprofv3 --kernel-trace --stats run of %d timed lr_decode_jpeg_device calls after %d untimed; us per call" % (
            a.batch, SEED, ", ".join("%dx%d" % s for s in SIZES), QUALITY, a.reps, WARM))
    totals = {}
    with tempfile.TemporaryDirectory() as inputs:
        make_bases(inputs)
        files = pil_files(load_frames(inputs, a.batch, 1))
        np.savez(os.path.join(inputs, "files.npz"), data=np.frombuffer(b"".join(files), np.uint8), lens=np.array([len(s) for s in files], np.int64))
        for r in range(a.rounds):
            for key, tree, way, title in LEGS:
                with tempfile.TemporaryDirectory() as tmp:
                    out = step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "jd", "--output-format", "csv", "--"] + me +
                               ["--child", way, "--tree", trees[tree], "--inputs", inputs], log)
                    log("\n== round %d: %s: %s ==" % (r + 1, title, [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][7:]))
                    per_call = np.zeros(calls - WARM)
                    for name in KERNELS + ((WARP,) if way == "workaround" else ()):
                        v = dispatch_times(tmp, name)
                        if not v or len(v) % calls:
                            log("FAILED: %d dispatches of %s in %d calls" % (len(v), name, calls))
                            raise SystemExit(1)
                        us = np.array(v, np.float64).reshape(calls, len(v) // calls)[WARM:].sum(axis=1) / 1e3
                        per_call += us
                        if name in ("jd_output_kernel", WARP):
                            log("      %-24s median %9.1f us  min %9.1f  max %9.1f" % (name, float(np.median(us)), us.min(), us.max()))
                    log("      %-24s median %9.1f us  min %9.1f  max %9.1f" % ("all launches of a call", float(np.median(per_call)), per_call.min(), per_call.max()))
                    totals.setdefault(key, []).append((float(np.median(per_call)), float(per_call.min()), float(per_call.max())))
    log("\n== all launches of a call, us: the rounds' medians (and the least and most of any call) ==")
    for key, _, _, title in LEGS:
        v = totals[key]
        log("  %-38s %s   (%.1f .. %.1f)" % (title, "  ".join("%9.1f" % m for m, _, _ in v), min(x[1] for x in v), max(x[2] for x in v)))
    med = {k: statistics.median(m for m, _, _ in v) for k, v in totals.items()}
    log("  (b) - (a): %+.1f us;  (c) - (d): %+.1f us, (c) / (d) = %.3f" % (med["b"] - med["a"], med["c"] - med["d"], med["c"] / med["d"]))
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_orient.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", choices=["stored", "oriented", "workaround"])
    ap.add_argument("--tree", help="(children) the checkout whose package is measured")
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    a = ap.parse_args()
    if a.child:
        a.way = a.child
        child(a)
    elif not a.parent:
        ap.error("--parent is needed")
    else:
        parent(a)
