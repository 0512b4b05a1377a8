#!/usr/bin/env python3
"""What LR_WARP_LENS costs: the lens launch against the same launch without the bit, against the two launches it replaces,
and end to end; and that nothing else was touched.

    python tools/warp_lens_timing.py [--out profiles/warp_lens.txt] [--sections resources,kernels,two,e2e,bench,demo]
                                     [--parent-tree DIR] [--reps 20] [--repeats 3]

Sections (each appends to --out):
  resources  no GPU: the three warp translation units compiled with -Rpass-analysis=kernel-resource-usage: VGPRs, SGPRs,
             scratch, LDS and occupancy of the twelve warp_ragged_lens_kernel instantiations, none of which may use scratch,
             and of every kernel of kernels_warp.hip and kernels_warp_border.hip from this tree and from --parent-tree (a
             checkout of the parent commit), which must be equal; exits 1 otherwise.
  kernels    kernel time from `rocprofv3 --kernel-trace --stats`, a run of its own per case and sampling rule, the program
             after `--`: in one process the launch without the bit and the launch with a barrel lens on every frame,
             alternating.  Cases: the 3840x2160 u8x3 and u8 frames of tools/warp_cubic_timing.py under its perspective map, and
             the 64 mixed colour frames of tools/ragged_batch_timing.py in one ragged launch.
  two        the two launches that one lens launch replaces, in a run of the same kind: the lens launch with the identity
             map (the undistorted frames) and the plain warp of its result; their sum beside the single launch's time.
  e2e        rectify_batch(64 files, jpeg=95) with and without lens=, by host clock around the synchronous call, alternating.
  bench      bench.py --gpus 1 --steps 20 --warmup 5 from the parent's tree and from this one, alternating, --repeats runs
             each (nothing bench.py times was touched).
  demo       not a test: the golden photograph distorted on the CPU with the barrel lens, run through rectify without and with
             lens=, beside the undistorted original: segments, their mean length and the two vanishing directions of each.
Every GPU step is a child process under a time limit; the first that fails ends the run.  Needs a GPU except `resources`.
"""
import argparse
import csv
import glob
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
from warp_cubic_timing import CASES, CUBIC, WARM, import_package, section_bench, step  # noqa: E402
from warp_timing import perspective  # noqa: E402

LENS = 0x100000
LENS_CASES = ("4k_u8x3", "4k_u8", "ragged64")
UNITS = ("kernels_warp.hip", "kernels_warp_border.hip", "kernels_warp_lens.hip")
KERNEL = re.compile(r"(warp_perspective_kernel|warp_ragged_kernel|warp_ragged_border_kernel|warp_ragged_lens_kernel)<([^>]*)>")


def barrel(w, h):
    """a phone's wide camera, roughly: 0.8 of the longer side as focal length, the centre in the middle"""
    f = 0.8 * max(w, h)
    return (f, f, (w - 1) / 2.0, (h - 1) / 2.0, -0.2, 0.05, 0.0, 0.0, 0.0)


def child_kernels(a):
    """legs plain / lens alternating (--mode one) or identity lens launch / plain warp of its result alternating (--mode two)"""
    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    rule = CUBIC if a.rule == "cubic" else 0
    if a.case == "ragged64":
        make_bases(a.inputs)
        host, sources = one_region(load_frames(a.inputs, 64, 1))
        d_src = ctx.device_upload(host)
        _, _, table, d_dst, total = ctx.rectify_frames_device(d_src, sources, L.PIX_U8X3, max_size=1200)
        assert (table[:, 9] > 0).all()
        lenses = np.array([barrel(w, h) for w, h, _, _ in sources])
        with_lens = np.concatenate([table, lenses], axis=1)
        ideal = np.zeros((len(sources), 27))
        ideal[:, :9] = np.eye(3).reshape(9)
        ideal[:, 9:13] = ideal[:, 13:17] = np.array(sources, np.float64)
        ideal[:, 18:] = lenses
        d_ideal = ctx.device_upload(np.zeros(len(host), np.uint8))
        fmt = L.PIX_U8X3
        plain = lambda src: ctx.warp_perspective_ragged_device(src, len(host), fmt | rule, table, d_dst, total)  # noqa: E731
        lens = lambda: ctx.warp_perspective_ragged_device(d_src, len(host), fmt | rule | LENS, with_lens, d_dst, total)  # noqa: E731
        undistort = lambda: ctx.warp_perspective_ragged_device(d_src, len(host), fmt | LENS, ideal, d_ideal, len(host))  # noqa: E731
    else:
        w, h, fmt, bpp = CASES[a.case]
        src = np.random.default_rng(0).integers(0, 256, w * h * bpp, dtype=np.uint8)
        d_src = ctx.device_upload(src)
        d_dst = ctx.device_upload(np.zeros(w * h * bpp, np.uint8))
        d_ideal = ctx.device_upload(np.zeros(w * h * bpp, np.uint8))
        M = perspective(w, h).reshape(9)
        row = np.concatenate([M, barrel(w, h)])
        eye = np.concatenate([np.eye(3).reshape(9), barrel(w, h)])
        one = lambda s, d, word, m: ctx.warp_perspective_device(s, src.nbytes, 1, w, h, w * bpp, word, m, d, src.nbytes, w, h, w * bpp)  # noqa: E731
        plain = lambda s: one(s, d_dst, fmt | rule, M)  # noqa: E731
        lens = lambda: one(d_src, d_dst, fmt | rule | LENS, row)  # noqa: E731
        undistort = lambda: one(d_src, d_ideal, fmt | LENS, eye)  # noqa: E731
    for _ in range(WARM + a.reps):
        if a.mode == "one":
            plain(d_src)
            ctx.synchronize()
            lens()
        else:
            undistort()
            ctx.synchronize()
            plain(d_ideal)
        ctx.synchronize()
    print("RESULT case=%s launches_per_leg=%d" % (a.case, WARM + a.reps))
    for p in (d_src, d_dst, d_ideal):
        ctx.device_free(p)
    ctx.close()


def profiled(a, case, rule, mode, log):
    """{kernel name: (average, min, max in us, calls)} of the warp kernels of one rocprofv3 run"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "warp", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "kernels", "--case", case, "--rule", rule, "--mode", mode,
               "--reps", str(a.reps), "--inputs", a.inputs]
        step(cmd, log)
        res = {}
        for s in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for rec in csv.DictReader(open(s)):
                m = KERNEL.search(rec["Name"])
                if m:
                    res[m.group(1)] = res.get(m.group(1), []) + [(float(rec["AverageNs"]) / 1e3, float(rec["MinNs"]) / 1e3, float(rec["MaxNs"]) / 1e3, int(rec["Calls"]))]
    return res


def plain_name(case):
    return "warp_ragged_kernel" if case == "ragged64" else "warp_perspective_kernel"


def most_called(rows):
    """(ragged64's run also holds rectify_frames_device's own bilinear launch: with the cubic rule an instantiation of one call)"""
    return max(rows, key=lambda r: r[3])


def section_kernels(a, log):
    log("\n== kernels: the launch with a barrel lens on every frame against the same launch without the bit, alternating in one process; one rocprofv3 --kernel-trace --stats run per case and rule ==")
    log("   (%d launches a leg, the first %d of them warm-up, all counted; average us (min - max); ratio = lens / without)" % (WARM + a.reps, WARM))
    a.single = {}
    for case in LENS_CASES:
        for rule in ("linear", "cubic"):
            res = profiled(a, case, rule, "one", log)
            p, l = most_called(res[plain_name(case)]), most_called(res["warp_ragged_lens_kernel"])
            a.single[case, rule] = l[0]
            log("  %-9s %-6s without %8.1f (%.1f - %.1f)   lens %8.1f (%.1f - %.1f)   ratio %.2f" % (case, rule, p[0], p[1], p[2], l[0], l[1], l[2], l[0] / p[0]))


def section_two(a, log):
    log("\n== two: the two launches one lens launch replaces: the identity-map lens launch (bilinear), then the plain warp of its result; a run of the same kind ==")
    for case in LENS_CASES:
        for rule in ("linear", "cubic"):
            res = profiled(a, case, rule, "two", log)
            u, p = most_called(res["warp_ragged_lens_kernel"]), most_called(res[plain_name(case)])
            single = getattr(a, "single", {}).get((case, rule))
            log("  %-9s %-6s undistort %8.1f + warp %8.1f = %8.1f us%s" % (case, rule, u[0], p[0], u[0] + p[0],
                "" if single is None else "   one lens launch %8.1f us: %.2f of the two" % (single, single / (u[0] + p[0]))))


def child_e2e(a):
    from jpeg_decode_timing import pil_files

    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    make_bases(a.inputs)
    frames = load_frames(a.inputs, 64, 1)
    files = pil_files(frames)
    lenses = [L.Lens(*barrel(f.shape[1], f.shape[0])) for f in frames]
    legs = (("without", None), ("lens", lenses))
    out = {k: ctx.rectify_batch(files, jpeg=95, lens=v) for k, v in legs}  # (warm-up of both)
    print("NOTE %d files, %.1f MB; products %.1f MB (without), %.1f MB (lens)" % (
        len(files), sum(map(len, files)) / 1e6, sum(len(x[2]) for x in out["without"] if x[2]) / 1e6, sum(len(x[2]) for x in out["lens"] if x[2]) / 1e6))
    for r in range(a.repeats):
        for k, v in legs:
            t0 = time.perf_counter()
            ctx.rectify_batch(files, jpeg=95, lens=v)
            print("E2E %s %.1f" % (k, (time.perf_counter() - t0) * 1e3))
    ctx.close()


def section_e2e(a, log):
    log("\n== e2e: rectify_batch(64 files, jpeg=95) without and with lens= (a barrel lens per file), host clock around the call, alternating ==")
    out = step([sys.executable, os.path.abspath(__file__), "--child", "e2e", "--repeats", str(a.repeats), "--inputs", a.inputs], log)
    for line in out.splitlines():
        if line.startswith("NOTE"):
            log("  " + line[5:])
    for k in ("without", "lens"):
        v = [float(x.split()[2]) for x in out.splitlines() if x.startswith("E2E " + k)]
        log("  %-7s median %7.1f ms  min %7.1f  max %7.1f  runs: %s" % (k, statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))


def distort_on_the_cpu(img, lens):
    """the photograph a camera with this lens would have stored: for every stored pixel the ideal point that the lens shows
    there (a fixed-point iteration on the displacement), sampled bilinearly from the ideal picture `img`"""
    import librectify_amd as L

    h, w = img.shape
    p = np.stack(np.meshgrid(np.arange(float(w)), np.arange(float(h))), axis=-1)
    q = p.copy()
    for _ in range(60):
        q = p - (L.lens_distort(lens, q) - q)
    assert np.abs(L.lens_distort(lens, q) - p).max() < 1e-6
    x0, y0 = np.floor(q[..., 0]).astype(np.int64), np.floor(q[..., 1]).astype(np.int64)
    ax, ay = q[..., 0] - x0, q[..., 1] - y0
    pad = np.pad(img.astype(np.float64), 1)  # (zero outside, as the warp)
    tap = lambda dx, dy: pad[np.clip(y0 + dy + 1, 0, h + 1), np.clip(x0 + dx + 1, 0, w + 1)]  # noqa: E731
    out = (tap(0, 0) * (1 - ax) + tap(1, 0) * ax) * (1 - ay) + (tap(0, 1) * (1 - ax) + tap(1, 1) * ax) * ay
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def child_demo(a):
    L = import_package(None)
    ctx = L.Context(0)
    ctx.set_seed(0)
    img = np.load(os.path.join(ROOT, "tests", "golden", "doc_image_gray.npy"))
    lens = L.Lens(*barrel(img.shape[1], img.shape[0]))
    stored = distort_on_the_cpu(img, lens)
    for name, frame, kw in (("original", img, {}), ("distorted", stored, {}), ("distorted, lens=", stored, {"lens": lens})):
        lines, t, _ = ctx.rectify(frame, **kw)
        length = np.hypot(lines["x2"] - lines["x1"], lines["y2"] - lines["y1"])
        vps = []
        for vp in (t.horizontal_vp, t.vertical_vp):  # (homogeneous: the direction from the picture's centre)
            dx, dy = vp.x - vp.z * img.shape[1] / 2.0, vp.y - vp.z * img.shape[0] / 2.0
            vps.append(np.degrees(np.arctan2(dy, dx)) % 180.0)
        print("DEMO %-18s %4d segments, mean length %6.1f px, vanishing directions %6.2f and %6.2f degrees" % (name, len(lines), length.mean(), vps[0], vps[1]))
    ctx.close()


def section_demo(a, log):
    log("\n== demo (no test): the golden photograph, the same distorted on the CPU with the barrel lens (k1 -0.2, k2 0.05, f = 0.8 of the longer side), and that through rectify(lens=) ==")
    out = step([sys.executable, os.path.abspath(__file__), "--child", "demo"], log)
    for line in out.splitlines():
        if line.startswith("DEMO"):
            log("  " + line[5:])


def resources(tree):
    """{unit: {kernel: (VGPRs, SGPRs, scratch, LDS, occupancy)}} of a tree's warp translation units"""
    sys.path.insert(0, ROOT)
    from librectify_amd import build

    out = {}
    for unit in UNITS:
        src = os.path.join(tree, "librectify_amd", "csrc", unit)
        if not os.path.exists(src):
            continue
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
    new, old = resources(ROOT), resources(a.parent_tree)
    fmt = lambda r: "%3d / %3d / %d / %d / %d" % r  # noqa: E731
    log("  kernels_warp_lens.hip, warp_ragged_lens_kernel<format, cubic, border> (new):")
    for name, r in sorted(new["kernels_warp_lens.hip"].items()):
        log("    %-44s %s" % (name, fmt(r)))
    ok = len(new["kernels_warp_lens.hip"]) == 12 and all(r[2] == 0 for r in new["kernels_warp_lens.hip"].values())
    log("   twelve instantiations, none with scratch: %s" % ("yes" if ok else "NO"))
    for unit in UNITS[:2]:
        log("  %s, this tree and the parent's:" % unit)
        for name in sorted(set(new[unit]) | set(old[unit])):
            n, o = new[unit].get(name), old[unit].get(name)
            ok = ok and n == o
            log("    %-44s %-26s parent %-26s %s" % (name, fmt(n) if n else "-", fmt(o) if o else "-", "equal" if n == o else "DIFFERENT"))
    log("   every kernel of the two existing code objects has the parent's figures: %s" % ("yes" if ok else "NO"))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_lens.txt"))
    ap.add_argument("--sections", default="resources,kernels,two,e2e,bench,demo")
    ap.add_argument("--parent-tree")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inputs")
    ap.add_argument("--child", choices=("kernels", "e2e", "demo"))
    ap.add_argument("--case", choices=LENS_CASES)
    ap.add_argument("--rule", default="linear", choices=("linear", "cubic"))
    ap.add_argument("--mode", default="one", choices=("one", "two"))
    a = ap.parse_args()
    if a.child:
        {"kernels": child_kernels, "e2e": child_e2e, "demo": child_demo}[a.child](a)
        raise SystemExit(0)
    f = open(a.out, "a")

    def log(text):
        print(text, flush=True)
        f.write(text + "\n")
        f.flush()

    with tempfile.TemporaryDirectory() as inputs:
        a.inputs = a.inputs or inputs
        for s in a.sections.split(","):
            {"resources": section_resources, "kernels": section_kernels, "two": section_two, "e2e": section_e2e, "bench": section_bench,
             "demo": section_demo}[s](a, log)
