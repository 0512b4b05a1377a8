#!/usr/bin/env python3
"""What LR_WARP_LENS_MODEL costs: the launch with seventeen-entry lenses against the same launch with the nine-entry lens,
which runs the parent's kernels; and that no kernel that existed before was touched.

    python tools/warp_lens_models_timing.py [--out profiles/warp_lens_models.txt] [--sections resources,kernels,e2e,bench]
                                            [--parent-tree DIR] [--reps 15] [--inner 10] [--repeats 5]

Sections (each appends to --out):
  resources  no GPU: the five warp translation units compiled with -Rpass-analysis=kernel-resource-usage: VGPRs, SGPRs,
             scratch, LDS and occupancy of the eighteen instantiations of kernels_warp_lens_model.hip, none of which may use
             scratch, and of every kernel of the four units that existed before, from this tree and from --parent-tree (a
             checkout of the parent commit), which must be equal; exits 1 otherwise.
  kernels    time per launch by host clock around --inner enqueued launches and a synchronise, --reps windows a leg after three
             of warm-up, the legs alternating window by window in one process: the nine-entry barrel lens (LR_WARP_LENS alone),
             model 0 with all twelve coefficients, and the fisheye.  Cases: the 3840x2160 u8x3 frame of
             tools/warp_cubic_timing.py under its perspective map, bilinear and bicubic; the 3840x2160 u8 frame; the 64 mixed
             colour frames of tools/ragged_batch_timing.py in one ragged launch.  Medians and the ratios to the first leg.
  e2e        rectify_batch(64 files, jpeg=95, lens=) with a nine-entry Lens per file (the parent's lens= figure) and with a
             fisheye per file, by host clock around the synchronous call, alternating.
  bench      bench.py --gpus 1 --steps 20 --warmup 5 from the parent's tree (--parent-tree, with its library built) and from this
             one, alternating, --repeats runs each (nothing bench.py times was touched).
Every GPU step is a child process under a time limit; the first that fails ends the run.  Needs a GPU except `resources`.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ragged_batch_timing import load_frames, make_bases, one_region  # noqa: E402
from warp_cubic_timing import CASES, CUBIC, import_package, section_bench, step  # noqa: E402
from warp_timing import perspective  # noqa: E402

LENS, MODEL = 0x100000, 0x800000
WARM = 3
OLD_UNITS = ("kernels_warp.hip", "kernels_warp_border.hip", "kernels_warp_lens.hip", "kernels_warp_area.hip")
NEW_UNIT = "kernels_warp_lens_model.hip"
KERNEL = re.compile(r"(warp_\w+_kernel)<([^>]*)>")
RUNS = (("4k_u8x3", "linear"), ("4k_u8x3", "cubic"), ("4k_u8", "linear"), ("ragged64", "linear"))
LEGS = ("nine", "rational12", "fisheye")


def lens_rows(leg, w, h):
    """a phone's wide camera, roughly: 0.8 of the longer side as focal length, the centre in the middle; (entries, bits)"""
    f, cx, cy = 0.8 * max(w, h), (w - 1) / 2.0, (h - 1) / 2.0
    if leg == "nine":
        return (f, f, cx, cy, -0.2, 0.05, 0.0, 0.0, 0.0), LENS
    if leg == "rational12":
        return (f, f, cx, cy, -0.2, 0.05, 0.001, -0.0005, 0.01, 0.02, 0.003, 0.0004, 0.0005, -0.0001, 0.0003, 0.0001, 0.0), LENS | MODEL
    return (f, f, cx, cy, 0.05, -0.01, 0.005, -0.001) + (0.0,) * 8 + (1.0,), LENS | MODEL


def child_kernels(a):
    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    rule = CUBIC if a.rule == "cubic" else 0
    launches = {}
    if a.case == "ragged64":
        make_bases(a.inputs)
        host, sources = one_region(load_frames(a.inputs, 64, 1))
        d_src = ctx.device_upload(host)
        _, _, table, d_dst, total = ctx.rectify_frames_device(d_src, sources, L.PIX_U8X3, max_size=1200)
        assert (table[:, 9] > 0).all()
        for leg in LEGS:
            rows = np.array([lens_rows(leg, w, h)[0] for w, h, _, _ in sources])
            bits = lens_rows(leg, 1, 1)[1]
            launches[leg] = (lambda t, b: lambda: ctx.warp_perspective_ragged_device(d_src, len(host), L.PIX_U8X3 | rule | b, t, d_dst, total))(np.concatenate([table, rows], axis=1), bits)
    else:
        w, h, fmt, bpp = CASES[a.case]
        src = np.random.default_rng(0).integers(0, 256, w * h * bpp, dtype=np.uint8)
        d_src = ctx.device_upload(src)
        d_dst = ctx.device_upload(np.zeros(w * h * bpp, np.uint8))
        M = perspective(w, h).reshape(9)
        for leg in LEGS:
            row, bits = lens_rows(leg, w, h)
            launches[leg] = (lambda m, b: lambda: ctx.warp_perspective_device(d_src, src.nbytes, 1, w, h, w * bpp, fmt | rule | b, m, d_dst, src.nbytes, w, h, w * bpp))(np.concatenate([M, row]), bits)
    for window in range(WARM + a.reps):
        for leg in LEGS:
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.inner):
                launches[leg]()
            ctx.synchronize()
            if window >= WARM:
                print("LEG %s %.2f" % (leg, (time.perf_counter() - t0) * 1e6 / a.inner))
    ctx.device_free(d_src)
    ctx.device_free(d_dst)
    ctx.close()


def section_kernels(a, log):
    log("\n== kernels: time per launch in us, host clock around %d enqueued launches and a synchronise; %d windows a leg after %d of warm-up, legs alternating in one process ==" % (a.inner, a.reps, WARM))
    log("   (nine: LR_WARP_LENS alone, the parent's kernels; rational12 and fisheye: LR_WARP_LENS_MODEL; median (min - max); ratio = median / nine's)")
    for case, rule in RUNS:
        out = step([sys.executable, os.path.abspath(__file__), "--child", "kernels", "--case", case, "--rule", rule, "--reps", str(a.reps),
                    "--inner", str(a.inner), "--inputs", a.inputs], log)
        med = {}
        text = "  %-9s %-6s" % (case, rule)
        for leg in LEGS:
            v = [float(x.split()[2]) for x in out.splitlines() if x.startswith("LEG " + leg + " ")]
            med[leg] = statistics.median(v)
            text += "  %s %8.1f (%.1f - %.1f)" % (leg, med[leg], min(v), max(v))
        log(text + "   ratios %.2f %.2f" % (med["rational12"] / med["nine"], med["fisheye"] / med["nine"]))


def child_e2e(a):
    from jpeg_decode_timing import pil_files

    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    make_bases(a.inputs)
    frames = load_frames(a.inputs, 64, 1)
    files = pil_files(frames)
    legs = (("nine", [L.Lens(*lens_rows("nine", f.shape[1], f.shape[0])[0]) for f in frames]),
            ("fisheye", [L.LensModel(*lens_rows("fisheye", f.shape[1], f.shape[0])[0]) for f in frames]))
    for k, v in legs:  # (warm-up of both)
        ctx.rectify_batch(files, jpeg=95, lens=v)
    for r in range(a.repeats):
        for k, v in legs:
            t0 = time.perf_counter()
            ctx.rectify_batch(files, jpeg=95, lens=v)
            print("E2E %s %.1f" % (k, (time.perf_counter() - t0) * 1e3))
    ctx.close()


def section_e2e(a, log):
    log("\n== e2e: rectify_batch(64 files, jpeg=95, lens=) with a nine-entry Lens per file and with a fisheye per file, host clock around the call, alternating ==")
    out = step([sys.executable, os.path.abspath(__file__), "--child", "e2e", "--repeats", str(a.repeats), "--inputs", a.inputs], log)
    med = {}
    for k in ("nine", "fisheye"):
        v = [float(x.split()[2]) for x in out.splitlines() if x.startswith("E2E " + k)]
        med[k] = statistics.median(v)
        log("  %-7s median %7.1f ms  min %7.1f  max %7.1f  runs: %s" % (k, med[k], min(v), max(v), " ".join("%.1f" % x for x in v)))
    log("  ratio fisheye / nine %.3f" % (med["fisheye"] / med["nine"]))


def resources(tree, units):
    """{unit: {kernel: (VGPRs, SGPRs, scratch, LDS, occupancy)}} of a tree's warp translation units"""
    sys.path.insert(0, ROOT)
    from librectify_amd import build

    out = {}
    for unit in units:
        src = os.path.join(tree, "librectify_amd", "csrc", unit)
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o", os.path.join(tmp, "w.o")],
                               capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-3000:])
        kernels, name = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                k = KERNEL.search(subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout)
                name = "%s<%s>" % (k.group(1), re.sub(r"\(lr_pixel_format\)|\(bool\)", "", k.group(2))) if k else None
                if name:
                    kernels[name] = {}
            elif name:
                kernels[name][m.group(1).split()[0]] = int(m.group(2))
        out[unit] = {k: (d["VGPRs"], d["TotalSGPRs"], d["ScratchSize"], d["LDS"], d["Occupancy"]) for k, d in kernels.items()}
    return out


def section_resources(a, log):
    if not a.parent_tree:
        raise SystemExit("--sections resources needs --parent-tree")
    log("\n== resources: -Rpass-analysis=kernel-resource-usage for gfx950: VGPRs / SGPRs / scratch bytes a lane / LDS bytes / waves a SIMD ==")
    new, old = resources(ROOT, OLD_UNITS + (NEW_UNIT,)), resources(a.parent_tree, OLD_UNITS)
    fmt = lambda r: "%3d / %3d / %d / %d / %d" % r  # noqa: E731
    log("  %s (new): warp_ragged_lens_model_kernel<format, cubic, border>, warp_ragged_area_lens_model_kernel<format, cubic>:" % NEW_UNIT)
    for name, r in sorted(new[NEW_UNIT].items()):
        log("    %-52s %s" % (name, fmt(r)))
    ok = len(new[NEW_UNIT]) == 18 and all(r[2] == 0 for r in new[NEW_UNIT].values())
    log("   eighteen instantiations, none with scratch: %s" % ("yes" if ok else "NO"))
    for unit in OLD_UNITS:
        log("  %s, this tree and the parent's:" % unit)
        for name in sorted(set(new[unit]) | set(old[unit])):
            n, o = new[unit].get(name), old[unit].get(name)
            ok = ok and n == o
            log("    %-52s %-28s parent %-28s %s" % (name, fmt(n) if n else "-", fmt(o) if o else "-", "equal" if n == o else "DIFFERENT"))
    log("   every kernel of the four existing code objects has the parent's figures: %s" % ("yes" if ok else "NO"))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_lens_models.txt"))
    ap.add_argument("--sections", default="resources,kernels,e2e")
    ap.add_argument("--parent-tree")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inputs")
    ap.add_argument("--child", choices=("kernels", "e2e"))
    ap.add_argument("--case", choices=sorted({c for c, _ in RUNS}))
    ap.add_argument("--rule", default="linear", choices=("linear", "cubic"))
    a = ap.parse_args()
    if a.child:
        {"kernels": child_kernels, "e2e": child_e2e}[a.child](a)
        raise SystemExit(0)
    f = open(a.out, "a")

    def log(text):
        print(text, flush=True)
        f.write(text + "\n")
        f.flush()

    with tempfile.TemporaryDirectory() as inputs:
        a.inputs = a.inputs or inputs
        for s in a.sections.split(","):
            {"resources": section_resources, "kernels": section_kernels, "e2e": section_e2e, "bench": section_bench}[s](a, log)
