#!/usr/bin/env python3
"""Timing of the JPEG decoder: its launches per stage, and from files to files Context.rectify_batch(files, jpeg=95) against
the route the parent commit offers to the same products -- PIL decoding the files on 16 host threads, then
rectify_batch(arrays, jpeg=95) (a tool, not a test).  Needs a GPU and PIL, except for --sections cpu.

    python tools/jpeg_decode_timing.py [--out profiles/jpeg_decode.txt] [--batch 64] [--reps 5] [--repeats 3] [--sections cpu,kernels,e2e]

Inputs: jpeg_timing's -- `batch` colour frames drawn with a fixed seed from 3840x2160, 1920x1080, 1600x1200 and 1200x1600,
content from librectify_amd.synth -- as the files PIL writes of them at quality 95, 4:2:0, no restart markers (what a camera
writes: the hard case for the entropy decoder).

  * cpu (no GPU): the restatement (tests/numpy_jpeg_decode_ref.py) against PIL's decode on the fixture files and
    tests/golden/doc_image.jpg, the maximum difference and the PSNR per layout: the figures tests/test_jpeg_decode_cpu.py
    asserts with its margins.
  * kernels: kernel time per launch of one lr_decode_jpeg_device call on the list, one `rocprofv3 --kernel-trace --stats`
    run in a process of its own under `timeout`; the bytes uploaded against the pixels'; the entropy stage's rounds.
  * e2e: with the profiler off, in one process, the two routes alternating, `repeats` rounds after one warm-up each, with
    max_size=None and 1200.

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
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ragged_batch_timing import SEED, SIZES, load_frames, make_bases  # noqa: E402
from rectify_batch_timing import dispatch_times  # noqa: E402

STEP_TIMEOUT = 420
WARM = 2
QUALITY = 95
THREADS = 16
KERNELS = ("jd_sync_kernel", "jd_place_kernel", "jd_write_kernel", "jd_dc_kernel", "jd_transform_kernel", "jd_output_kernel")


def pil_files(frames):
    from PIL import Image

    def one(f):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=QUALITY, subsampling=2)
        return buf.getvalue()

    with ThreadPoolExecutor(THREADS) as pool:
        return list(pool.map(one, frames))


def pil_decode(files):
    from PIL import Image

    with ThreadPoolExecutor(THREADS) as pool:
        return list(pool.map(lambda s: np.asarray(Image.open(io.BytesIO(s)).convert("RGB")), files))


def section_cpu(log):
    from PIL import Image

    import numpy_jpeg_decode_ref as D
    import numpy_jpeg_ref as R

    kat = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode_kat.npz"))
    cases = [(str(n), kat["stream_" + str(n)].tobytes()) for n in kat["names"]]
    with open(os.path.join(ROOT, "tests", "golden", "doc_image.jpg"), "rb") as f:
        cases.append(("doc_image", f.read()))
    log("\n== the restatement against PIL %s's decode (no GPU): maximum difference, PSNR ==" % Image.__version__)
    worst = {}
    for name, s in cases:
        pil = np.asarray(Image.open(io.BytesIO(s)))
        info = D.probe(s)
        _, ours = D.decode(s, "u8x3" if pil.ndim == 3 else "u8")
        d, p = int(np.abs(ours.astype(int) - pil.astype(int)).max()), R.psnr(ours, pil)
        key = "one component" if pil.ndim == 2 else {0: "4:2:0", 1: "4:4:4", 2: "4:2:2"}[info.layout]
        worst[key] = (max(worst.get(key, (0, 99))[0], d), min(worst.get(key, (0, 99))[1], p))
        log("  %-20s %-13s max %d  PSNR %.2f dB" % (name, key, d, p))
    for key, (d, p) in sorted(worst.items()):
        log("  %-13s: maximum %d, lowest PSNR %.2f dB" % (key, d, p))


def child_kernels(a):
    import ctypes as C

    import librectify_amd as L

    ctx = L.Context(0)
    files = pil_files(load_frames(a.inputs, a.batch, 1))
    lens = np.array([len(s) for s in files], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    region = np.frombuffer(b"".join(files), np.uint8)
    sizes = L.jpeg_info(files)[:, :2].astype(np.int64)
    places = np.concatenate([[0], np.cumsum((sizes[:, 0] * sizes[:, 1] * 3 + 3) // 4 * 4)]).astype(np.int64)
    table = L.jpeg_decode_table(np.stack([offs, lens], axis=1), np.stack([places[:-1], sizes[:, 0] * 3], axis=1), sizes)
    d_src = ctx.device_upload(region)
    d_dst = C.c_void_p()
    L._check(L.lib().lr_device_malloc(ctx._h, int(places[-1]), C.byref(d_dst)))
    for _ in range(WARM + a.reps):
        info = ctx.decode_jpeg_device(d_src, region, L.PIX_U8X3, table, d_dst.value, int(places[-1]))
    assert not info[:, 5].any()
    print("RESULT frames=%d file_bytes=%d pixel_bytes=%d most_decodes_of_a_part=%d..%d" % (
        len(files), len(region), int(places[-1]), int(info[:, 6].min()), int(info[:, 6].max())))
    ctx.device_free(d_src)
    ctx.device_free(d_dst.value)
    ctx.close()


def child_e2e(a):
    import librectify_amd as L

    ctx = L.Context(0)
    ctx.set_seed(0)
    files = pil_files(load_frames(a.inputs, a.batch, 1))
    for max_size in (None, 1200):
        legs = {"host": lambda: ctx.rectify_batch(pil_decode(files), max_size=max_size, jpeg=QUALITY),
                "device": lambda: ctx.rectify_batch(files, max_size=max_size, jpeg=QUALITY)}
        same = [x[2] == y[2] for x, y in zip(legs["host"](), legs["device"]())]  # (warm-up of both)
        print("NOTE max_size=%s: %d of %d products are the same bytes by both routes (PIL's decode is not ours)" % (max_size, sum(same), len(same)))
        for r in range(a.repeats):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                print("E2E leg=%s max_size=%s ms=%.1f" % (name, max_size, (time.perf_counter() - t0) * 1e3))
                sys.stdout.flush()
        t0 = time.perf_counter()
        pil_decode(files)
        print("E2E leg=pil max_size=%s ms=%.1f" % (max_size, (time.perf_counter() - t0) * 1e3))
    ctx.close()


def step(cmd, log):
    r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        raise SystemExit(1)
    return r.stdout


def spread(v):
    return "median %.1f  min %.1f  max %.1f  runs: %s" % (statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v))


def parent(a):
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--reps", str(a.reps), "--repeats", str(a.repeats)]
    f = open(a.out, "a")

    def log(text):
        print(text)
        f.write(text + "\n")
        f.flush()

    sections = a.sections.split(",")
    if "cpu" in sections:
        section_cpu(log)
    if "kernels" in sections or "e2e" in sections:
        log("\njpeg_decode_timing: %d colour frames drawn (seed %d) from %s, as PIL's files at quality %d, 4:2:0, no DRI; %d timed repetitions after %d untimed, %d end-to-end rounds" % (
            a.batch, SEED, ", ".join("%dx%d" % s for s in SIZES), QUALITY, a.reps, WARM, a.repeats))
        with tempfile.TemporaryDirectory() as inputs:
            here = ["--inputs", inputs]
            make_bases(inputs)
            if "kernels" in sections:
                log("\n== kernel time per lr_decode_jpeg_device call on the list (rocprofv3 --kernel-trace --stats) ==")
                with tempfile.TemporaryDirectory() as tmp:
                    out = step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "jd", "--output-format", "csv", "--"] + me + ["--child", "kernels"] + here, log)
                    log("  " + [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][7:])
                    total = 0.0
                    for name in KERNELS:
                        v = dispatch_times(tmp, name)
                        calls = WARM + a.reps
                        if not v or len(v) % calls:
                            log("FAILED: %d dispatches of %s in %d calls" % (len(v), name, calls))
                            raise SystemExit(1)
                        per = len(v) // calls
                        us = np.array(v, np.float64).reshape(calls, per)[WARM:].sum(axis=1) / 1e3
                        log("      %-24s %d launch%s a call  median %9.1f us  min %9.1f  max %9.1f" % (name, per, "" if per == 1 else "es", float(np.median(us)), us.min(), us.max()))
                        total += float(np.median(us))
                    log("      %-24s                    %9.1f us (sum of the medians)" % ("the decoder's launches", total))
            if "e2e" in sections:
                log("\n== end to end, files to files (profiler off): PIL on %d threads + rectify_batch(arrays, jpeg=%d) against rectify_batch(files, jpeg=%d), alternating ==" % (THREADS, QUALITY, QUALITY))
                out = step(me + ["--child", "e2e"] + here, log)
                times = {}
                for ln in out.splitlines():
                    if ln.startswith("NOTE"):
                        log("  " + ln[5:])
                    if ln.startswith("E2E"):
                        kv = dict(x.split("=") for x in ln.split()[1:])
                        times.setdefault((kv["max_size"], kv["leg"]), []).append(float(kv["ms"]))
                for max_size in ("None", "1200"):
                    log("  max_size=%s:" % max_size)
                    log("    %-52s %s ms" % ("PIL decode + rectify_batch(arrays, jpeg=%d)" % QUALITY, spread(times[(max_size, "host")])))
                    log("    %-52s %s ms" % ("  of which PIL's decode alone (one more run)", spread(times[(max_size, "pil")])))
                    log("    %-52s %s ms" % ("rectify_batch(files, jpeg=%d)" % QUALITY, spread(times[(max_size, "device")])))
                    log("    files against host decode: %.2f x (medians)" % (statistics.median(times[(max_size, "host")]) / statistics.median(times[(max_size, "device")])))
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sections", default="cpu,kernels,e2e")
    ap.add_argument("--child", choices=["kernels", "e2e"])
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    a = ap.parse_args()
    if a.child == "kernels":
        child_kernels(a)
    elif a.child == "e2e":
        child_e2e(a)
    else:
        parent(a)
