#!/usr/bin/env python3
"""Timing of the lines picture (lr_draw_lines_device) against the u8x3 warp on an identity map at the same output size
(a tool, not a test).  Needs a GPU; there is no CPU path.

    python tools/overlay_timing.py [--out profiles/overlay.txt] [--reps 5]

Legs: `4k` the 3840x2160 bench frame (synth seed 1) with its own segments; `8k` the 8192x8192 tiled frame of
BASELINE.json configs[4] (synth seed 7, 6000 bars in 512-px blocks; through the host entry with min_length 20: some 24 000
segments); `batch` 64 frames of
1920x1080 (seeds 1000.., rolled copies of four) through one call, as draw_lines_batch makes it.

The parent process starts every GPU step as a process of its own under `timeout` and stops at the first that fails:
  * `inputs`: the frames and their segments (the detector), written to a temporary folder;
  * per leg one `rocprofv3 --kernel-trace --stats` run of `kernels`: after a warm-up, `reps` times each of
      draw        the gray frame and all segments into u8x3 (1 byte read + 3 written per pixel),
      background  the same call with every count 0: the kernel's copy alone,
      in place    the segments drawn upon the finished picture: the culling and the per-pixel tests without the
                  background's traffic (only covered pixels are written),
      dots        draw with every segment shrunk to its midpoint: the same number of records in nearly the same bins and
                  tiles -- the bins' lists, the box tests, the compaction into LDS and the barriers stay -- while the
                  per-pixel tests shrink to an 11 x 11 box a record.  The cull-only variant, as near as the library's
                  interface allows without a switch in the kernel: draw - dots is the per-pixel work of the strokes,
                  dots - background what the culling and the list handling cost,
      no bins     (the 8192x8192 leg) draw with the coarse level out of the way: segments that paint nothing are put in
                  front, five pixels outside each edge of the frame and as long as it, until the frame has more than
                  8 bin entries a record and the host keeps one list of all, which every tile then walks in full.  The
                  picture is compared with draw's, byte for byte.  The padding's records survive only in the tiles on the
                  frame's edges,
      warp        warp_perspective_kernel<u8x3> on the identity map (3 bytes read + 3 written per pixel): the yardstick.
    Kernel time per dispatch comes from the kernel trace.  The culling's box tests (tiles x entries of their bin's list)
    and the records that survive them are counted on the host from the same bins the library makes.
  * per leg `calls`, profiler off: the host clock around call + synchronize for draw and warp, alternating (the
    library keeps its stream to itself, so no event of the tool's can be recorded on it).
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
STEP_TIMEOUT = 420
WARM = 2
HBM_TBS = 8.0
LEGS = ("4k", "8k", "batch")


def import_package():
    sys.path.insert(0, ROOT)
    import librectify_amd as L

    return L


def u8(frame):
    return np.clip(frame * 255.0, 0, 255).astype(np.uint8)


def child_inputs(a):
    L = import_package()
    from librectify_amd import synth

    ctx = L.Context(0)
    ctx.set_seed(0)
    sets = {"4k": [(u8(synth.frame(3840, 2160, 1)), 38.4)], "8k": [(u8(synth.frame(8192, 8192, 7, bars=6000, tile=512)), 20.0)]}
    bases = [u8(synth.frame(1920, 1080, 1000 + i)) for i in range(4)]
    sets["batch"] = [(np.ascontiguousarray(np.roll(bases[k % 4], (7 * k, 13 * k), (0, 1))), 19.2) for k in range(64)]
    for leg, frames in sets.items():
        lines = [ctx.find_line_segment_groups(f.astype(np.float32) / 256.0, ml, capacity=65536).copy() for f, ml in frames]
        np.savez(os.path.join(a.inputs, leg + ".npz"), n=len(frames), **{"f%d" % i: f for i, (f, _) in enumerate(frames)},
                 **{"l%d" % i: l for i, l in enumerate(lines)})
        print("%s: %d frame(s) of %dx%d, %d segments in all (groups %s)" % (
            leg, len(frames), frames[0][0].shape[1], frames[0][0].shape[0], sum(len(l) for l in lines),
            sorted(set(np.concatenate(lines)["group_id"].tolist()))))
    ctx.close()


def load(a, L):
    z = np.load(os.path.join(a.inputs, a.leg + ".npz"))
    n = int(z["n"])
    frames, lines = [z["f%d" % i] for i in range(n)], [z["l%d" % i].astype(L.LINE_DTYPE) for i in range(n)]
    h, w = frames[0].shape
    sizes = [(w, h)] * n
    table = L.draw_table(sizes, [(i * w * h, w) for i in range(n)], [(i * w * h * 3, w * 3) for i in range(n)],
                         list(zip(np.cumsum([0] + [len(l) for l in lines[:-1]]).tolist(), [len(l) for l in lines])))
    return frames, np.concatenate(lines), table, w, h, n


def cull_counts(lines_per_frame, w, h):
    """box tests and survivors of the kernel's culling, from the host's bins (kernels_overlay.hip: 256-px bins, boxes grown by
    5, a frame with more than 8 entries a record keeps one list) -- recomputed here with NumPy"""
    tests = survivors = entries_all = 0
    for ls in lines_per_frame:
        x = np.stack([np.trunc(ls["x1"].astype(np.float64)), np.trunc(ls["x2"].astype(np.float64))])
        y = np.stack([np.trunc(ls["y1"].astype(np.float64)), np.trunc(ls["y2"].astype(np.float64))])
        lo_x, hi_x = np.maximum(x.min(0) - 5, 0), np.minimum(x.max(0) + 5, w - 1)
        lo_y, hi_y = np.maximum(y.min(0) - 5, 0), np.minimum(y.max(0) + 5, h - 1)
        ok = (lo_x <= hi_x) & (lo_y <= hi_y)
        nb = lambda lo, hi, s: (hi // s - lo // s + 1)[ok]  # noqa: E731
        entries = float((nb(lo_x, hi_x, 256) * nb(lo_y, hi_y, 256)).sum())
        tiles = -(-w // 64) * -(-h // 16)
        tests += entries * 64 if entries <= 8 * len(ls) else float(len(ls)) * tiles
        entries_all += entries
        survivors += float((nb(lo_x, hi_x, 64) * nb(lo_y, hi_y, 16)).sum())
    return tests, survivors, entries_all


def edge_padding(L, lines, w, h):
    """segments just outside the four edges that paint nothing (the stroke ends a pixel short of the frame, the discs lie
    beyond its corners) but whose grown boxes cross a whole row or column of bins: enough of them to take the frame over
    the host's limit of 8 bin entries a record"""
    _, _, entries = cull_counts([lines], w, h)
    per = -(-max(w, h) // 256)
    k = int(max(0.0, 8 * len(lines) - entries) / (min(-(-w // 256), -(-h // 256)) - 8)) + 16
    pad = np.zeros(k, L.LINE_DTYPE)
    edges = [(-20.0, -5.0, w + 20.0, -5.0), (-20.0, h + 4.0, w + 20.0, h + 4.0), (-5.0, -20.0, -5.0, h + 20.0), (w + 4.0, -20.0, w + 4.0, h + 20.0)]
    for i in range(k):
        pad[i] = edges[i % 4] + (1.0, 0.0, i % 12)
    assert per > 8, "the padding needs a frame of more than eight bins a side"
    return pad


def child_kernels(a):
    import ctypes as C

    L = import_package()
    ctx = L.Context(0)
    frames, lines, table, w, h, n = load(a, L)
    gray_bytes, rgb_bytes = n * w * h, n * w * h * 3
    d_gray = ctx.device_upload(np.concatenate([f.reshape(-1) for f in frames]))
    bufs = [C.c_void_p() for _ in range(2)]
    for b in bufs:
        L._check(L.lib().lr_device_malloc(ctx._h, rgb_bytes, C.byref(b)))
    d_rgb, d_out = bufs[0].value, bufs[1].value
    empty = table.copy()
    empty[:, 6:] = 0
    in_place = table.copy()
    in_place[:, 2:4] = 0
    eye = np.tile(np.eye(3).reshape(-1), n)
    dots = lines.copy()
    dots["x1"] = dots["x2"] = np.trunc((lines["x1"] + lines["x2"]) / 2)
    dots["y1"] = dots["y2"] = np.trunc((lines["y1"] + lines["y2"]) / 2)
    order = ["draw", "background", "in place", "dots"]
    if a.leg == "8k":
        padded = np.concatenate([edge_padding(L, lines, w, h), lines])
        unbinned = table.copy()
        unbinned[:, 7] = len(padded)
        order.append("no bins")
    runs = {
        "draw": lambda: ctx.draw_lines_device(d_gray, gray_bytes, L.PIX_U8, lines, table, d_rgb, rgb_bytes),
        "background": lambda: ctx.draw_lines_device(d_gray, gray_bytes, L.PIX_U8, lines, empty, d_out, rgb_bytes),
        "in place": lambda: ctx.draw_lines_device(None, 0, L.PIX_U8X3, lines, in_place, d_rgb, rgb_bytes),
        "dots": lambda: ctx.draw_lines_device(d_gray, gray_bytes, L.PIX_U8, dots, table, d_out, rgb_bytes),
        "no bins": lambda: ctx.draw_lines_device(d_gray, gray_bytes, L.PIX_U8, padded, unbinned, d_out, rgb_bytes),
        "warp": lambda: ctx.warp_perspective_device(d_rgb, w * h * 3, n, w, h, w * 3, L.PIX_U8X3, eye, d_out, w * h * 3, w, h, w * 3),
    }
    if a.mode == "kernels":
        extra = ""
        for name in order + ["warp"]:
            if name == "in place":  # (before it draws upon the picture)
                picture = ctx.device_download(d_rgb, (rgb_bytes,), np.uint8) if a.leg == "8k" else None
            for _ in range(WARM + a.reps):
                runs[name]()
                ctx.synchronize()
            if name == "no bins":
                t2, s2, e2 = cull_counts([padded], w, h)
                assert e2 > 8 * len(padded) and t2 == float(len(padded)) * -(-w // 64) * -(-h // 16), "the padded frame is still binned"
                assert np.array_equal(ctx.device_download(d_out, (rgb_bytes,), np.uint8), picture), "the padding changed the picture"
                extra = " nobins_records=%d nobins_box_tests=%.3e nobins_survivors=%.3e" % (len(padded), t2, s2)
        tests, survivors, entries = cull_counts(np.split(lines, np.cumsum(table[:, 7].astype(int))[:-1]), w, h)
        print("RESULT leg=%s frames=%d size=%dx%d segments=%d bin_entries=%d box_tests=%.3e survivors=%.3e runs=%s%s" % (
            a.leg, n, w, h, len(lines), entries, tests, survivors, ",".join(x.replace(" ", "_") for x in order), extra))
    else:
        for name in ("draw", "warp"):
            runs[name]()
        ctx.synchronize()
        times = {"draw": [], "warp": []}
        for _ in range(a.reps * 2):
            for name in times:
                t0 = time.perf_counter()
                runs[name]()
                ctx.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
        for name, v in times.items():
            print("  %s call + synchronize, host clock, %d alternating rounds after a warm-up: median %.1f us  min %.1f  max %.1f" % (
                name, len(v), statistics.median(v), min(v), max(v)))
    for p in (d_gray, d_rgb, d_out):
        ctx.device_free(p)
    ctx.close()


def step(cmd, log):
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def parent(a):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from rectify_batch_timing import dispatch_times

    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps)]
    f = open(a.out, "a")

    def log(text):
        print(text)
        f.write(text + "\n")
        f.flush()

    log("overlay_timing: %d timed repetitions after %d untimed; kernel time per dispatch from rocprofv3 --kernel-trace --stats, a run per leg" % (a.reps, WARM))
    with tempfile.TemporaryDirectory() as inputs:
        here = ["--inputs", inputs]
        log(step(me + ["--child", "inputs"] + here, log).rstrip())
        for leg in LEGS:
            with tempfile.TemporaryDirectory() as tmp:
                out = step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "ov", "--output-format", "csv", "--"] + me +
                           ["--child", "kernels", "--leg", leg] + here, log)
                ov, wp = dispatch_times(tmp, "overlay_kernel"), dispatch_times(tmp, "warp_perspective_kernel")
            res = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][7:]
            log("\n== " + res + " ==")
            fields = dict(kv.split("=") for kv in res.split())
            per = WARM + a.reps
            names = [x.replace("_", " ") for x in fields["runs"].split(",")]
            if len(ov) != len(names) * per or len(wp) != per:
                log("FAILED: %d overlay and %d warp dispatches, expected %d and %d" % (len(ov), len(wp), len(names) * per, per))
                raise SystemExit(1)
            timed = {name: ov[k * per + WARM:(k + 1) * per] for k, name in enumerate(names)}
            timed["warp"] = wp[WARM:]
            med = {name: float(np.median(v)) / 1e3 for name, v in timed.items()}
            w, h = (int(v) for v in fields["size"].split("x"))
            px = int(fields["frames"]) * w * h
            for name, v in timed.items():
                bpp = {"draw": 4, "background": 4, "warp": 6}.get(name, 0)
                rate = "  %.2f TB/s = %.2f of the %.0f TB/s roof" % (px * bpp / med[name] / 1e6, px * bpp / med[name] / 1e6 / HBM_TBS, HBM_TBS) if bpp else ""
                log("  %-11s kernel median %9.1f us  min %9.1f  max %9.1f%s" % (name, med[name], min(v) / 1e3, max(v) / 1e3, rate))
            log("  ratio draw / warp: %.2f" % (med["draw"] / med["warp"]))
            log("  the copy alone (background) %.1f us; in place on the finished picture (no copy, covered pixels written) %.1f us" % (med["background"], med["in place"]))
            log("  split by the dots variant: culling and list handling (dots - background) %.1f us; per-pixel tests of the strokes (draw - dots) %.1f us" % (
                med["dots"] - med["background"], med["draw"] - med["dots"]))
            log("  culling: %s box tests (tiles x entries of their bin's list), %s records survive into the LDS lists" % (fields["box_tests"], fields["survivors"]))
            if "no bins" in med:
                log("  without the coarse level (one list of %s records for every tile: %s box tests, %s survivors; same picture): %.1f us = %.2f of the warp, %.1f x draw" % (
                    fields["nobins_records"], fields["nobins_box_tests"], fields["nobins_survivors"], med["no bins"], med["no bins"] / med["warp"], med["no bins"] / med["draw"]))
            log(step(me + ["--child", "calls", "--leg", leg] + here, log).rstrip())
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", choices=["inputs", "kernels", "calls"])
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--inputs")
    a = ap.parse_args()
    a.mode = a.child
    if a.child == "inputs":
        child_inputs(a)
    elif a.child in ("kernels", "calls"):
        child_kernels(a)
    else:
        parent(a)
