#!/usr/bin/env python3
"""Timing of LR_JPEG_SCALED in the JPEG decoder (a tool, not a test).  Needs a GPU and PIL.

    python tools/jpeg_decode_scale_timing.py --parent-tree DIR [--out profiles/jpeg_decode_scale.txt] [--batch 64] [--reps 5] [--runs 5]

DIR is a built checkout of the parent commit (python -m librectify_amd.build in it); without it the comparison with the
parent is left out.

Inputs: jpeg_decode_timing's -- `batch` colour frames drawn with a fixed seed from 3840x2160, 1920x1080, 1600x1200 and
1200x1600, content from librectify_amd.synth, at quality 95 without restart markers, as PIL's 4:2:0 files.

  * without the bit: kernel time per stage of one lr_decode_jpeg_device call, the parent commit's library and this one's
    alternating, `runs` profiled processes each (`rocprofv3 --kernel-trace --stats`, a process of its own under `timeout`
    per run; each run's figure is the median of `reps` calls after 2 untimed).  The yardstick is the parent's own spread over
    its runs: this commit's median of runs must lie inside it.
  * with the bit at N = 2, 4, 8: the same, one run each, per stage.
  * the product: rectify_batch(files, jpeg=95, decode_scale=2) against the two ways to a half-size result that need no bit --
    the full decode plus one scaling LR_WARP_RAGGED launch (time, and PSNR of both against the 2 x 2 box average of the full
    decode), and the full-size rectify_batch(files, jpeg=95) (time, and the bytes of HBM the pictures hold).  Wall-clock, in
    this process, the median of `reps` calls after 2 untimed.

Everything is appended to --out as it is measured.
"""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from jpeg_decode_sampling_timing import KERNELS, QUALITY, THREADS, WARM, step, table  # noqa: E402
from ragged_batch_timing import SEED, SIZES, import_package, load_frames, make_bases  # noqa: E402
from rectify_batch_timing import dispatch_times  # noqa: E402

SCALED = 0x80000
PSNR_FRAMES = 16


def make_files(folder, batch):
    from PIL import Image

    sys.path.insert(0, ROOT)
    make_bases(folder)
    frames = load_frames(folder, batch, 1)

    def pil(f):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=QUALITY, subsampling=2)
        return buf.getvalue()

    with ThreadPoolExecutor(THREADS) as pool:
        files = list(pool.map(pil, frames))
    np.savez(os.path.join(folder, "420.npz"), region=np.frombuffer(b"".join(files), np.uint8), lens=np.array([len(s) for s in files], np.int64),
             sizes=np.array([f.shape[1::-1] for f in frames], np.int64))


def load_files(folder):
    z = np.load(os.path.join(folder, "420.npz"))
    return z["region"], z["lens"], z["sizes"]


def decode_setup(L, ctx, region, lens, sizes, scale):
    """(format word, table, destination, its bytes, the places) of one decoder call at `scale` (0: without the bit)"""
    import ctypes as C

    n = max(scale, 1)
    sizes = -(-sizes // n)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    places = np.concatenate([[0], np.cumsum((sizes[:, 0] * sizes[:, 1] * 3 + 3) // 4 * 4)]).astype(np.int64)
    kw = {"scale": scale} if scale else {}
    tbl = L.jpeg_decode_table(np.stack([offs, lens], axis=1), np.stack([places[:-1], sizes[:, 0] * 3], axis=1), sizes, **kw)
    d_dst = C.c_void_p()
    L._check(L.lib().lr_device_malloc(ctx._h, int(places[-1]), C.byref(d_dst)))
    return L.PIX_U8X3 | (SCALED if scale else 0), tbl, d_dst.value, int(places[-1]), places, sizes


def child_kernels(a):
    L = import_package(a.tree)
    ctx = L.Context(0)
    region, lens, sizes = load_files(a.inputs)
    fmt, tbl, d_dst, total, _, _ = decode_setup(L, ctx, region, lens, sizes, a.scale)
    d_src = ctx.device_upload(region)
    for _ in range(WARM + a.reps):
        info = ctx.decode_jpeg_device(d_src, region, fmt, tbl, d_dst, total)
    assert not info[:, 5].any(), info[:, 5]
    print("RESULT frames=%d file_bytes=%d pixel_bytes=%d most_decodes_of_a_part=%d..%d" % (
        len(lens), len(region), total, int(info[:, 6].min()), int(info[:, 6].max())))
    ctx.device_free(d_src)
    ctx.device_free(d_dst)
    ctx.close()


def profiled(a, log, inputs, tree, scale):
    """one profiled process: {kernel: median us of a call's launches of it, "all": their sum}, and the child's RESULT line"""
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", "kernels", "--inputs", inputs, "--scale", str(scale)]
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
    print("  (a profiled run of %s, scale %d: %.1f us)" % ("the parent commit" if tree else "this commit", scale, got["all"]), flush=True)
    return got, [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][7:]


def timed(reps, call):
    ms = []
    for _ in range(WARM + reps):
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[WARM:]
    return out, "median %8.1f ms  min %8.1f  max %8.1f" % (statistics.median(ms), min(ms), max(ms))


def psnr(a, b):
    d = a.astype(np.int32) - b.astype(np.int32)
    return 10.0 * np.log10(255.0 ** 2 / max(float(np.mean(d * d)), 1e-12))


def box(p, n):
    h, w = p.shape[0] // n * n, p.shape[1] // n * n
    return ((p[:h, :w].astype(np.uint32).reshape(h // n, n, w // n, n, 3).sum(axis=(1, 3)) + n * n // 2) // (n * n)).astype(np.uint8)


def product(a, log, inputs):
    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    region, lens, sizes = load_files(inputs)
    ends = np.cumsum(lens)
    files = [region[e - n:e].tobytes() for e, n in zip(ends, lens)]
    d_src = ctx.device_upload(region)

    def pictures(d, places, szs, count):
        out = []
        for b in range(count):
            w, h = int(szs[b, 0]), int(szs[b, 1])
            flat = ctx.device_download(d + int(places[b]), (h * w * 3,), np.uint8)
            out.append(flat.reshape(h, w, 3))
        return out

    log("\n== half-size pictures in HBM: the decoder at N = 2 against the full decode plus one scaling LR_WARP_RAGGED launch (wall clock) ==")
    fmt1, tbl1, d_full, total1, places1, sizes1 = decode_setup(L, ctx, region, lens, sizes, 0)
    fmt2, tbl2, d_half, total2, places2, sizes2 = decode_setup(L, ctx, region, lens, sizes, 2)
    _, t = timed(a.reps, lambda: ctx.decode_jpeg_device(d_src, region, fmt2, tbl2, d_half, total2))
    log("      lr_decode_jpeg_device, LR_JPEG_SCALED, N = 2                 %s   pictures: %d bytes" % (t, total2))
    half = pictures(d_half, places2, sizes2, PSNR_FRAMES)
    sources = [(int(w), int(h), int(o), int(w) * 3) for (w, h), o in zip(sizes1, places1[:-1])]
    import ctypes as C

    for name, M in (("M = diag(2, 2, 1), the plain scaling map", [[2, 0, 0], [0, 2, 0], [0, 0, 1]]),
                    ("M = diag(2, 2, 1) + (0.5, 0.5), the centred scaling map", [[2, 0, 0.5], [0, 2, 0.5], [0, 0, 1]])):
        rt, wbytes = L.ragged_table(np.array([M] * len(files), np.float64), sizes2, sources, 3)
        d_warp = C.c_void_p()
        L._check(L.lib().lr_device_malloc(ctx._h, wbytes, C.byref(d_warp)))

        def way1():
            ctx.decode_jpeg_device(d_src, region, fmt1, tbl1, d_full, total1)
            ctx.warp_perspective_ragged_device(d_full, total1, L.PIX_U8X3, rt, d_warp.value, wbytes)
            return ctx.device_download(d_warp.value, (4,), np.uint8)  # (waits for the stream)

        _, t = timed(a.reps, way1)
        log("      full decode + LR_WARP_RAGGED, %-56s %s   pictures: %d + %d bytes" % (name, t, total1, wbytes))
        warped = [ctx.device_download(d_warp.value + int(rt[b, 11]), (int(sizes2[b, 1]), int(rt[b, 12])), np.uint8)[:, :int(sizes2[b, 0]) * 3].reshape(
            int(sizes2[b, 1]), int(sizes2[b, 0]), 3) for b in range(PSNR_FRAMES)]
        full = pictures(d_full, places1, sizes1, PSNR_FRAMES)
        ours, theirs = [], []
        for b in range(PSNR_FRAMES):
            want = box(full[b], 2)
            ours.append(psnr(half[b][:want.shape[0], :want.shape[1]], want))
            theirs.append(psnr(warped[b][:want.shape[0], :want.shape[1]], want))
        log("        PSNR against the 2 x 2 box average of the full decode, first %d frames: the decoder at N = 2 %.2f dB (worst %.2f); this warp %.2f dB (worst %.2f)" % (
            PSNR_FRAMES, statistics.mean(ours), min(ours), statistics.mean(theirs), min(theirs)))
        ctx.device_free(d_warp.value)
    for d in (d_src, d_full, d_half):
        ctx.device_free(d)

    log("\n== the product: rectify_batch(files, jpeg=95) on the %d files, wall clock, files in and files out ==" % len(files))
    for label, kw in (("full size", {}), ("decode_scale=2", {"decode_scale": 2}), ("decode_scale=4", {"decode_scale": 4})):
        res, t = timed(a.reps, lambda: ctx.rectify_batch(files, jpeg=95, **kw))
        outs = [r[2] for r in res if r[2] is not None]
        n = kw.get("decode_scale", 1)
        decoded = int((-(-sizes // n)).prod(axis=1).sum() * 3)
        rectified = int(L.jpeg_info(outs)[:, :2].astype(np.int64).prod(axis=1).sum() * 3)
        log("      %-16s %s   %d of %d rectified; HBM held by pictures: decoded %d + rectified %d = %d bytes; files out %d bytes; segments %d" % (
            label, t, len(outs), len(files), decoded, rectified, decoded + rectified, sum(len(o) for o in outs), sum(len(r[0]) for r in res)))
    ctx.close()


def parent(a):
    f = open(a.out, "a")

    def log(text):
        print(text, flush=True)
        f.write(text + "\n")
        f.flush()

    log("\njpeg_decode_scale_timing: %d colour frames drawn (seed %d) from %s, quality %d, no DRI, PIL's 4:2:0 files; per run the median of %d calls after %d untimed; %d runs where runs are compared" % (
        a.batch, SEED, ", ".join("%dx%d" % s for s in SIZES), QUALITY, a.reps, WARM, a.runs))
    with tempfile.TemporaryDirectory() as inputs:
        make_files(inputs, a.batch)
        log("\n== without the bit: kernel time per lr_decode_jpeg_device call (rocprofv3 --kernel-trace --stats), alternating ==")
        old, new = [], []
        for _ in range(a.runs):
            if a.parent_tree:
                old.append(profiled(a, log, inputs, a.parent_tree, 0)[0])
            got, result = profiled(a, log, inputs, None, 0)
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
        for n in (1, 2, 4, 8):
            log("\n== with the bit, every frame at N = %d%s ==" % (n, " (the kernels of a call without the bit)" if n == 1 else ""))
            got, result = profiled(a, log, inputs, None, n)
            log("  " + result)
            table(log, [got], "this commit, N = %d" % n)
        product(a, log, inputs)
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_scale.txt"))
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", choices=["kernels"])
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    ap.add_argument("--scale", type=int, default=0, help="(children) 0: without LR_JPEG_SCALED; 1, 2, 4, 8: with it, every frame at that scale")
    ap.add_argument("--tree", help="(children) the checkout whose library is loaded")
    a = ap.parse_args()
    if a.child == "kernels":
        child_kernels(a)
    else:
        parent(a)
