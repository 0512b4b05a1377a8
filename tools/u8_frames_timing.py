"""Timing of 8-bit against fp32 frames through the detector's entries (a tool, not a test).

One process: every shape is warmed in both formats first, then fp32 and 8-bit legs alternate, five repetitions each:

  single 4K call from pageable memory, single 4K call from page-locked memory, the 8192 x 8192 call,
  64 x 4K and 512 x 1080p through the batch call from pageable frames, 64 x 4K from resident frames,

and, as what the feature takes off the caller, the host-side conversion `astype(float32) / 256` of a 4K frame.
With --u8x3 the single calls and the resident batch are also timed for interleaved frames.

    python tools/u8_frames_timing.py [--reps 5] [--skip-8k] [--u8x3] > profiles/u8_frames.txt

--kernel-frames N: instead of the legs, N single resident frames of each format and nothing else -- the run to put
under `rocprofv3 --kernel-trace --stats` for the filter instantiations' kernel times.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import librectify_amd as L  # noqa: E402
from librectify_amd import synth  # noqa: E402


def quantise(img):
    return np.clip(np.floor(np.asarray(img, np.float64) * 256.0 + 0.5), 0, 255).astype(np.uint8)


def unit(u8):
    return np.ascontiguousarray(u8.astype(np.float32) * np.float32(1.0 / 256.0))


def frames_u8(n, w, h, seed):
    base = [quantise(synth.frame(w, h, seed + i)) for i in range(min(n, 4))]
    return np.ascontiguousarray(np.stack([np.roll(base[i % len(base)], 37 * (i // 4), axis=1) for i in range(n)]))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternate(legs, reps):
    """legs: {name: callable}; every leg once per round, `reps` rounds; returns {name: [ms]}"""
    for fn in legs.values():  # warm: workspace, staging, hints
        fn()
        fn()
    out = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            out[k].append(timed(fn))
    return out


def report(title, res, mpix):
    print(title)
    for k, v in res.items():
        med = statistics.median(v)
        print("  %-12s median %9.3f ms  min %9.3f  max %9.3f  %9.1f Mpix/s   runs: %s" % (
            k, med, min(v), max(v), mpix / med * 1e3, " ".join("%.3f" % x for x in v)))
    sys.stdout.flush()


def single_calls(ctx, u8, reps, rgb):
    h, w = u8.shape
    ml = max(w, h) / 100.0
    f32 = unit(u8)
    legs_src = {"fp32": f32, "u8": u8}
    if rgb:
        legs_src["u8x3"] = np.ascontiguousarray(np.stack([u8] * 3, axis=2))
    res = alternate({k: (lambda s=s: ctx.find_line_segment_groups(s, ml, num_threads=12, capacity=1 << 16)) for k, s in legs_src.items()}, reps)
    report("single %dx%d call, pageable frame" % (w, h), res, w * h / 1e6)
    pinned = {}
    try:
        for k, s in legs_src.items():
            pinned[k] = ctx.host_alloc(s.shape, s.dtype)
            pinned[k][...] = s
        res = alternate({k: (lambda s=s: ctx.find_line_segment_groups(s, ml, num_threads=12, capacity=1 << 16)) for k, s in pinned.items()}, reps)
        report("single %dx%d call, page-locked frame" % (w, h), res, w * h / 1e6)
    finally:
        for a in pinned.values():
            ctx.host_free(a)


def batch_host(ctx, u8, reps, title):
    B, h, w = u8.shape
    ml = max(w, h) / 100.0
    f32 = np.ascontiguousarray(np.stack([unit(f) for f in u8]))
    out = np.zeros((B, 4096), L.LINE_DTYPE)
    legs = {"fp32": lambda: ctx.find_line_segment_groups_batch_host(f32, ml, num_threads=12, out=out),
            "u8": lambda: ctx.find_line_segment_groups_batch_host(u8, ml, num_threads=12, out=out)}
    report(title, alternate(legs, reps), B * w * h / 1e6)


def batch_device(ctx, u8, reps, title, rgb):
    B, h, w = u8.shape
    ml = max(w, h) / 100.0
    out = np.zeros((B, 4096), L.LINE_DTYPE)
    bufs = {"fp32": (np.ascontiguousarray(np.stack([unit(f) for f in u8])), L.PIX_F32), "u8": (u8, L.PIX_U8)}
    if rgb:
        bufs["u8x3"] = (np.ascontiguousarray(np.stack([u8] * 3, axis=3)), L.PIX_U8X3)
    ptrs = {}
    try:
        for k, (a, fmt) in bufs.items():
            ptrs[k] = (ctx.device_upload(a), fmt)
        legs = {k: (lambda d=d, fmt=fmt: ctx.find_line_segment_groups_batch_device(d, w * h, B, w, h, ml, out=out, fmt=fmt)) for k, (d, fmt) in ptrs.items()}
        report(title, alternate(legs, reps), B * w * h / 1e6)
    finally:
        for d, _ in ptrs.values():
            ctx.device_free(d)


def kernel_frames(ctx, n):
    u8 = quantise(synth.frame(3840, 2160, 1))
    h, w = u8.shape
    for a, fmt in ((unit(u8), L.PIX_F32), (u8, L.PIX_U8), (np.ascontiguousarray(np.stack([u8] * 3, axis=2)), L.PIX_U8X3)):
        d = ctx.device_upload(a)
        try:
            for _ in range(n):
                ctx.find_line_segment_groups_device(d, w, h, 38.4, fmt=fmt)
        finally:
            ctx.device_free(d)
    print("%d frames 3840x2160 of each format through lr_find_line_segment_groups_device" % n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-8k", action="store_true")
    ap.add_argument("--u8x3", action="store_true")
    ap.add_argument("--kernel-frames", type=int, default=0)
    args = ap.parse_args()
    ctx = L.Context(0)
    ctx.set_seed(0)
    if args.kernel_frames:
        kernel_frames(ctx, args.kernel_frames)
        return
    u8_4k = frames_u8(64, 3840, 2160, 1)
    conv = [timed(lambda: u8_4k[0].astype(np.float32) / np.float32(256.0)) for _ in range(args.reps + 2)][2:]
    print("host conversion of one 3840x2160 frame, astype(float32) / 256, one core: median %.3f ms (%s)" % (
        statistics.median(conv), " ".join("%.3f" % x for x in conv)))
    single_calls(ctx, u8_4k[0], args.reps, args.u8x3)
    batch_host(ctx, u8_4k, args.reps, "64 x 3840x2160 through the batch call, pageable frames")
    batch_device(ctx, u8_4k, args.reps, "64 x 3840x2160 through the batch call, resident frames", args.u8x3)
    del u8_4k
    batch_host(ctx, frames_u8(512, 1920, 1080, 1000), args.reps, "512 x 1920x1080 through the batch call, pageable frames")
    ctx.trim()
    if not args.skip_8k:
        big = np.ascontiguousarray(np.tile(quantise(synth.frame(2048, 2048, 7)), (4, 4)))
        c2 = L.Context(0)
        c2.set_seed(0)
        single_calls(c2, big, args.reps, False)
        c2.close()
    ctx.close()


if __name__ == "__main__":
    main()
