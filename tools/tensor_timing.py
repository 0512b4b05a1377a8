#!/usr/bin/env python3
"""Timing of lr_pack_tensor_device: its launch beside the identity LR_WARP_RAGGED launch over the same pictures and beside
torch's own expression on the same device data, and Context.rectify_batch(files, jpeg=95, tensor=spec) against the parent
commit's rectify_batch followed by the same packing with NumPy on the host and an upload (a tool, not a test).  Needs a GPU
and torch.

    python tools/tensor_timing.py [--out profiles/tensor.txt] [--batch 64] [--reps 5] [--repeats 3] [--parent TREE] [--sections kernels,calls,e2e]

Inputs: ragged_batch_timing's -- `batch` colour frames drawn with a fixed seed from 3840x2160, 1920x1080, 1600x1200 and
1200x1600, content from librectify_amd.synth.  Case "list": every frame subsampled to the size fit_box gives it in 640 x 640
(what the area warp hands the pack), packed into batch x 3 x 640 x 640 f16.  Case "4k-f32-nchw" and "4k-f16-nhwc": the first
3840x2160 frame as it is, into one slot of its own size.

The parent process starts every GPU step as a process of its own under `timeout` and stops at the first that fails:

  * kernels: one `rocprofv3 --kernel-trace --stats` run per case; per repetition one identity warp of the u8x3 pictures (the
    project's yardstick for one pass over these bytes) and one lr_pack_tensor_device call.  Bytes moved = the pictures' bytes
    read + the named slots' bytes written; their rate over the kernel time is set against the HBM roof.
  * calls (profiler off): per case the whole lr_pack_tensor_device call (host table, upload, launch, wait) and torch's own
    expression on the same device data (permute, to, sub_, div_, F.pad, into the same batch tensor), each between device
    synchronisations, alternating.
  * e2e (profiler off, needs --parent TREE, a built checkout of the parent commit): the files of the list; the parent's
    rectify_batch(files, jpeg=95, out_max_size=640), the parent's rectify_batch(files, out_max_size=640) followed by the
    NumPy packing on the host and one upload of the tensor, and this tree's rectify_batch(files, jpeg=95, tensor=spec,
    tensor_out=a torch tensor); a process per tree and round, alternating; a process warms its path up once and times one call.

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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ragged_batch_timing import SEED, SIZES, load_frames, make_bases, one_region  # noqa: E402
from rectify_batch_timing import dispatch_times  # noqa: E402

STEP_TIMEOUT = 420
WARM = 2
BOX = 640
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12  # bytes/s: the spec, and what a float4 copy reaches (MI355X)
CASES = ("list", "4k-f32-nchw", "4k-f16-nhwc")


def import_package(tree):
    sys.path.insert(0, tree or ROOT)
    import librectify_amd as L

    return L


def bounded_size(w, h):
    """shrink_homography's size rule for the bound fit_box((w, h), (BOX, BOX)), restated (the parent's tree has no fit_box)"""
    longer = max(w, h)
    N = min(longer, ((BOX + 1) * longer - 1) // w, ((BOX + 1) * longer - 1) // h)
    return (w, h) if longer <= N else (max(1, w * N // longer), max(1, h * N // longer))


def case_pictures(a, L):
    """(pictures, spec) of a case"""
    frames = load_frames(a.inputs, a.batch, 1)
    if a.case == "list":
        pics = []
        for f in frames:
            w, h = bounded_size(f.shape[1], f.shape[0])
            pics.append(np.ascontiguousarray(f[(np.arange(h) * f.shape[0]) // h][:, (np.arange(w) * f.shape[1]) // w]))
        return pics, L.TensorSpec((BOX, BOX), "f16", "nchw", mean=MEAN, std=STD)
    big = next(f for f in frames if f.shape[:2] == (2160, 3840))
    dtype, layout = a.case.split("-")[1:]
    return [big], L.TensorSpec((2160, 3840), dtype, layout, mean=MEAN, std=STD)


def resident(ctx, L, pics, spec):
    """the pictures in HBM with the two calls' tables: (d_src, src_bytes, sources, pack table, warp table, warp bytes)"""
    host, sources = one_region(pics)
    src = np.array(sources, np.int64)
    ttable = L.tensor_table(src[:, :2], src[:, 2:], np.arange(len(pics)), spec)
    wtable, wtotal = L.ragged_table(None, src[:, :2], src, 3)
    return ctx.device_upload(host), len(host), sources, ttable, wtable, wtotal


def child_kernels(a):
    import ctypes as C

    L = import_package(None)
    ctx = L.Context(0)
    pics, spec = case_pictures(a, L)
    d_src, src_bytes, sources, ttable, wtable, wtotal = resident(ctx, L, pics, spec)
    shape = spec.shape(len(pics), L.PIX_U8X3)
    total = int(np.prod(shape, dtype=np.int64)) * np.dtype(spec.np_dtype).itemsize
    p, q = C.c_void_p(), C.c_void_p()
    L._check(L.lib().lr_device_malloc(ctx._h, wtotal, C.byref(p)))
    L._check(L.lib().lr_device_malloc(ctx._h, total, C.byref(q)))
    for _ in range(WARM + a.reps):
        ctx.warp_perspective_ragged_device(d_src, src_bytes, L.PIX_U8X3, wtable, p.value, wtotal)
        ctx.synchronize()
        ctx.pack_tensor_device(d_src, src_bytes, L.PIX_U8X3, ttable, spec, len(pics), q.value, total)
    read = sum(w * h * 3 for w, h, _, _ in sources)
    print("RESULT case=%s pictures=%d picture_bytes=%d tensor_bytes=%d" % (a.case, len(pics), read, total))
    for ptr in (d_src, p.value, q.value):
        ctx.device_free(ptr)
    ctx.close()


def torch_expression(torch, F, d_pics, out, mean, std, spec):
    """torchvision's ToTensor + Normalize + a centred pad, written with torch's own operators on device data"""
    H, W = spec.size
    for b, t in enumerate(d_pics):
        x = t.permute(2, 0, 1).to(torch.float32)
        x.div_(255.0).sub_(mean).div_(std)
        x = x.to(out.dtype)
        h, w = x.shape[1:]
        left, top = (W - w) // 2, (H - h) // 2
        x = F.pad(x, (left, W - w - left, top, H - h - top))
        out[b].copy_(x.permute(1, 2, 0) if spec.layout == "nhwc" else x)


def child_calls(a):
    import torch
    import torch.nn.functional as F

    L = import_package(None)
    ctx = L.Context(0)
    dev = torch.device("cuda", 0)
    pics, spec = case_pictures(a, L)
    d_src, src_bytes, sources, ttable, _, _ = resident(ctx, L, pics, spec)
    tdtype = {"f32": torch.float32, "f16": torch.float16}[spec.dtype]
    out = torch.empty(spec.shape(len(pics), L.PIX_U8X3), dtype=tdtype, device=dev)
    ref = torch.empty_like(out)
    d_pics = [torch.from_numpy(p).to(dev) for p in pics]
    mean, std = (torch.tensor(v, dtype=torch.float32, device=dev).view(3, 1, 1) for v in (MEAN, STD))
    ours, theirs = [], []
    for r in range(WARM + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.pack_tensor_device(d_src, src_bytes, L.PIX_U8X3, ttable, spec, len(pics), out.data_ptr(), out.numel() * out.element_size())
        t1 = time.perf_counter()
        torch_expression(torch, F, d_pics, ref, mean, std, spec)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r >= WARM:
            ours.append((t1 - t0) * 1e6)
            theirs.append((t2 - t1) * 1e6)
    diff = (out.float() - ref.float()).abs().max().item()  # (torch rounds (v / 255 - mean) / std in float32: not the same bits)
    print("CALLS case=%s ours_us=%s torch_us=%s max_abs_diff=%.3g" % (a.case, ",".join("%.1f" % v for v in ours), ",".join("%.1f" % v for v in theirs), diff))
    ctx.device_free(d_src)
    ctx.close()


def host_pack(pics, spec_size, scale, bias):
    """the same packing with NumPy on the host: the rule of tests/numpy_tensor_ref.py, centred, pad level 0, f16 NCHW"""
    H, W = spec_size
    out = np.empty((len(pics), 3, H, W), np.float16)
    out[:] = (0.0 * scale + bias).astype(np.float32).astype(np.float16).reshape(1, 3, 1, 1)
    for b, p in enumerate(pics):
        if p is None:
            continue
        h, w = p.shape[:2]
        left, top = (W - w) // 2, (H - h) // 2
        out[b, :, top:top + h, left:left + w] = (p.astype(np.float64) * scale + bias).astype(np.float32).astype(np.float16).transpose(2, 0, 1)
    return out


def child_e2e(a):
    if a.who == "this":
        import torch  # (before the library is loaded, as bench.py imports it: after it torch finds no device)
    L = import_package(a.tree)
    ctx = L.Context(0)
    ctx.set_seed(0)
    files = ctx.encode_jpeg_batch(load_frames(a.inputs, a.batch, 1), 95)
    scale, bias = 1.0 / (255.0 * np.array(STD)), -np.array(MEAN) / np.array(STD)
    if a.who == "parent":
        def with_host_pack():
            res = ctx.rectify_batch(files, out_max_size=BOX)
            t = host_pack([r[2] for r in res], (BOX, BOX), scale, bias)
            d = ctx.device_upload(t)
            ctx.synchronize()
            ctx.device_free(d)

        legs = {"jpeg": lambda: ctx.rectify_batch(files, jpeg=95, out_max_size=BOX), "raw+numpy+upload": with_host_pack}
    else:
        spec = L.TensorSpec((BOX, BOX), "f16", "nchw", mean=MEAN, std=STD)
        out = torch.empty((len(files), 3, BOX, BOX), dtype=torch.float16, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        legs = {"jpeg+tensor": lambda: ctx.rectify_batch(files, jpeg=95, tensor=spec, tensor_out=out),
                "jpeg": lambda: ctx.rectify_batch(files, jpeg=95, out_max_size=BOX)}
    for name, fn in legs.items():
        fn()  # (warm-up)
        t0 = time.perf_counter()
        fn()
        print("E2E who=%s leg=%s ms=%.1f" % (a.who, name, (time.perf_counter() - t0) * 1e3))
        sys.stdout.flush()
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

    log("tensor_timing: %d colour frames drawn (seed %d) from %s; %d timed repetitions after %d untimed, %d end-to-end rounds" % (
        a.batch, SEED, ", ".join("%dx%d" % s for s in SIZES), a.reps, WARM, a.repeats))
    sections = a.sections.split(",")
    with tempfile.TemporaryDirectory() as inputs:
        here = ["--inputs", inputs]
        sys.path.insert(0, ROOT)
        make_bases(inputs)
        if "kernels" in sections:
            log("\n== kernel time per launch (rocprofv3 --kernel-trace --stats, a run per case); the u8x3 identity warp of the same pictures beside it ==")
            for case in CASES:
                with tempfile.TemporaryDirectory() as tmp:
                    out = step(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "tp", "--output-format", "csv", "--"] + me + ["--child", "kernels", "--case", case] + here, log)
                    res = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1]
                    log("  " + res[7:])
                    kv = dict(x.split("=") for x in res.split()[1:])
                    for name, moved in (("warp_ragged_kernel", 2 * int(kv["picture_bytes"])), ("tensor_pack_kernel", int(kv["picture_bytes"]) + int(kv["tensor_bytes"]))):
                        v = dispatch_times(tmp, name)
                        if len(v) != WARM + a.reps:
                            log("FAILED: %d dispatches of %s, expected %d" % (len(v), name, WARM + a.reps))
                            raise SystemExit(1)
                        us = np.array(v[WARM:], np.float64) / 1e3
                        rate = moved / (float(np.median(us)) * 1e-6)
                        log("      %-22s median %9.1f us  min %9.1f  max %9.1f   %6.1f MB moved, %5.2f TB/s: %4.1f %% of the 8.0 TB/s roof (%4.1f %% of a copy's 6.29)" % (
                            name, float(np.median(us)), us.min(), us.max(), moved / 1e6, rate / 1e12, 100 * rate / HBM_PEAK, 100 * rate / HBM_COPY))
        if "calls" in sections:
            log("\n== whole calls between device synchronisations (profiler off): lr_pack_tensor_device, and torch's permute / to / div_ / sub_ / div_ / F.pad on the same device data ==")
            for case in CASES:
                out = step(me + ["--child", "calls", "--case", case] + here, log)
                kv = dict(x.split("=") for x in [ln for ln in out.splitlines() if ln.startswith("CALLS")][-1].split()[1:])
                log("  case=%s (largest difference between the two tensors: %s)" % (case, kv["max_abs_diff"]))
                log("      lr_pack_tensor_device  %s us" % spread([float(x) for x in kv["ours_us"].split(",")]))
                log("      torch                  %s us" % spread([float(x) for x in kv["torch_us"].split(",")]))
        if a.parent and "e2e" in sections:
            log("\n== end to end from %d JPEG files (profiler off): a process per tree and round, alternating; a process warms up and times one call ==" % a.batch)
            times = {}
            for r in range(a.repeats):
                for who, tree in (("parent", a.parent), ("this", "")):
                    out = step(me + ["--child", "e2e", "--who", who, "--tree", tree] + here, log)
                    for ln in out.splitlines():
                        if ln.startswith("E2E"):
                            kv = dict(x.split("=") for x in ln.split()[1:])
                            times.setdefault((kv["who"], kv["leg"]), []).append(float(kv["ms"]))
            for who, leg, what in (("parent", "jpeg", "the parent's rectify_batch(jpeg=95, out_max_size=640): files only"),
                                   ("parent", "raw+numpy+upload", "the parent's rectify_batch(out_max_size=640) + NumPy pack + upload"),
                                   ("this", "jpeg", "this tree's rectify_batch(jpeg=95, out_max_size=640): files only"),
                                   ("this", "jpeg+tensor", "this tree's rectify_batch(jpeg=95, tensor=spec, tensor_out=)")):
                log("    %-68s %s ms" % (what, spread(times[(who, leg)])))
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--sections", default="kernels,calls,e2e", help="which of kernels, calls, e2e to run (e2e needs --parent)")
    ap.add_argument("--child", choices=["kernels", "calls", "e2e"])
    ap.add_argument("--case", choices=CASES, default="list")
    ap.add_argument("--who", choices=["parent", "this"], default="this")
    ap.add_argument("--tree", help="(e2e child) the tree to import librectify_amd from")
    ap.add_argument("--inputs", help="(children) the folder of the inputs' files")
    a = ap.parse_args()
    if a.child == "kernels":
        child_kernels(a)
    elif a.child == "calls":
        child_calls(a)
    elif a.child == "e2e":
        child_e2e(a)
    else:
        parent(a)
