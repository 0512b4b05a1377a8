"""The perspective warp on the GPU (lr_warp_perspective_device) against its float64 / int64 second source
(tests/numpy_warp_ref.py), bit for bit: three pixel formats, padded and odd strides, maps that reach every corner of the
canonical arithmetic, batches, offsets beyond 4 GiB; the golden picture through the library path; the batch detector
feeding one batched warp; Context.rectify; the recipe's --warp; bad arguments."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.set_seed(0)
    yield c
    c.close()


BPP = {0: 1, 1: 3, 2: 4}
DTYPE = {0: np.uint8, 1: np.uint8, 2: np.float32}


def frame(fmt, w, h, seed):
    rng = np.random.default_rng(seed)
    if fmt == 2:
        return (rng.random((h, w), dtype=np.float32) * np.float32(4.0) - np.float32(1.0)).astype(np.float32)
    return rng.integers(0, 256, (h, w, 3) if fmt == 1 else (h, w), dtype=np.uint8)


def maps(w, h, ow, oh):
    """name -> destination-to-source map for a w x h source and an ow x oh output"""
    c, s = math.cos(0.3), math.sin(0.3)
    cx, cy = w / 2.0, h / 2.0
    rot = np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1.0]])
    return {
        "identity": np.eye(3),
        "shift": np.array([[1.0, 0, -3], [0, 1, 2], [0, 0, 1]]),
        "scale_up": np.array([[0.37, 0, 0.2], [0, 0.41, -0.1], [0, 0, 1]]),
        "scale_down": np.array([[2.3, 0, 0], [0, 1.7, 0.5], [0, 0, 1]]),
        "rotation": rot,
        "perspective": np.array([[1.2, 0.3, -0.1 * w], [-0.05, 1.0, 0.05 * h], [0.6 / max(ow, 1), 0.4 / max(oh, 1), 1.0]]),
        # W0 = x / ow + 1.7 y / oh - 1.3 changes sign inside the output
        "horizon": np.array([[0.9, 0.1, 0.0], [0.05, 1.1, 0.0], [1.0 / ow, 1.7 / oh, -1.3]]),
        # W0 = y - oh // 2 is exactly 0 on one row
        "w0_zero_row": np.array([[1.0, 0, 0.25], [0, 1, 0], [0, 1.0, -float(oh // 2)]]),
        # 32 / W0 overflows: 0 * inf (NaN) at x = 0, INT_MAX beyond
        "tiny_w0_nan": np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1e-320]]),
        "tiny_w0_overflow": np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1e-300]]),
    }


def run_warp(L, ctx, src, fmt, M, ow, oh, src_pad, dst_pad, src_off=0, dst_off=0):
    """Warps one frame through padded rows, at a byte offset from the allocation; returns the output and checks that no
    byte outside the output's rows was written."""
    bpp = BPP[fmt]
    h, w = src.shape[:2]
    srow, drow = w * bpp + src_pad, ow * bpp + dst_pad
    sbuf = np.full(src_off + h * srow, 0x5A, np.uint8)
    sbuf[src_off:].reshape(h, srow)[:, : w * bpp] = np.ascontiguousarray(src).reshape(h, -1).view(np.uint8)
    dbuf = np.full(dst_off + oh * drow, 0xAB, np.uint8)
    d_src, d_dst = ctx.device_upload(sbuf), ctx.device_upload(dbuf)
    try:
        ctx.warp_perspective_device(d_src + src_off, h * srow, 1, w, h, srow, fmt, M, d_dst + dst_off, oh * drow, ow, oh, drow)
        got = ctx.device_download(d_dst, dbuf.shape, np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    assert (got[:dst_off] == 0xAB).all()
    rows = got[dst_off:].reshape(oh, drow)
    assert (rows[:, ow * bpp:] == 0xAB).all(), "bytes beyond a row's pixels were written"
    out = np.ascontiguousarray(rows[:, : ow * bpp]).view(DTYPE[fmt])
    return out.reshape((oh, ow, 3) if fmt == 1 else (oh, ow))


def assert_same(got, exp):
    if got.dtype == np.float32:
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
    else:
        np.testing.assert_array_equal(got, exp)


SMALL = [(1, 1), (5, 5), (63, 17), (257, 131)]


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("w,h", SMALL)
def test_bit_exact_small_shapes_every_map(L, ctx, fmt, w, h):
    src = frame(fmt, w, h, 11 + w)
    ow, oh = w + w // 3 + 1, h + h // 5 + 1
    pads = (3, 5, 1, 1) if fmt != 2 else (4, 12, 4, 8)  # odd / padded strides; f32 stays 4-byte aligned
    for k, (name, M) in enumerate(maps(w, h, ow, oh).items()):
        sp, dp = pads[k % 2], pads[(k + 1) % 2]
        off = (k % 3) * pads[2]
        got = run_warp(L, ctx, src, fmt, M, ow, oh, sp, dp, src_off=off, dst_off=pads[3] * (k % 2))
        assert_same(got, R.warp(src, M, ow, oh)), name
        if name == "identity":
            assert_same(got[:h, :w], src)


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_bit_exact_large_frames(L, ctx, fmt, w, h):
    src = frame(fmt, w, h, 5)
    m = maps(w, h, w, h)
    for name in ("identity", "perspective", "horizon", "rotation"):
        pad = 4 if fmt == 2 else 3
        got = run_warp(L, ctx, src, fmt, m[name], w, h, pad, pad + (4 if fmt == 2 else 2))
        assert_same(got, R.warp(src, m[name], w, h))
        if name == "identity":
            assert_same(got, src)


# outputs of one tile (1 x 1), exactly one tile (64 x 16) and one pixel over in each direction (65 x 17: four tiles, a partial
# lane at the right edge); at most twelve tiles in a launch, so some XCDs' runs are short or empty
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("ow,oh,batch", [(1, 1, 1), (64, 16, 1), (65, 17, 1), (65, 17, 3)])
def test_outputs_of_a_few_tiles(L, ctx, fmt, ow, oh, batch):
    w, h = 70, 20
    bpp = BPP[fmt]
    frames = [frame(fmt, w, h, 40 + b) for b in range(batch)]
    m = maps(w, h, ow, oh)
    Ms = np.stack([m[name] for name in ("rotation", "identity", "perspective")[:batch]])
    srow, drow = w * bpp + (4 if fmt == 2 else 1), ow * bpp + (4 if fmt == 2 else 3)
    simg, dimg = h * srow + (4 if fmt == 2 else 7), oh * drow + (12 if fmt == 2 else 5)
    sbuf = np.zeros(batch * simg, np.uint8)
    for b, f in enumerate(frames):
        sbuf[b * simg: b * simg + h * srow].reshape(h, srow)[:, : w * bpp] = f.reshape(h, -1).view(np.uint8)
    d_src = ctx.device_upload(sbuf)
    d_dst = ctx.device_upload(np.full(batch * dimg, 0xAB, np.uint8))
    try:
        ctx.warp_perspective_device(d_src, simg, batch, w, h, srow, fmt, Ms, d_dst, dimg, ow, oh, drow)
        got = ctx.device_download(d_dst, (batch * dimg,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    for b in range(batch):
        rows = got[b * dimg: b * dimg + oh * drow].reshape(oh, drow)
        assert (rows[:, ow * bpp:] == 0xAB).all() and (got[b * dimg + oh * drow: (b + 1) * dimg] == 0xAB).all()
        out = np.ascontiguousarray(rows[:, : ow * bpp]).view(DTYPE[fmt]).reshape((oh, ow, 3) if fmt == 1 else (oh, ow))
        assert_same(out, R.warp(frames[b], Ms[b], ow, oh))


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_batch_of_seven_frames_with_their_own_maps(L, ctx, fmt):
    w, h, ow, oh = 257, 131, 200, 150
    bpp = BPP[fmt]
    frames = [frame(fmt, w, h, 100 + b) for b in range(7)]
    base = list(maps(w, h, ow, oh).values())
    Ms = np.stack([base[(3 * b + 1) % len(base)] @ np.array([[1, 0, b], [0, 1, -b], [0, 0, 1.0]]) for b in range(7)])
    srow, drow = w * bpp + (4 if fmt == 2 else 1), ow * bpp + (4 if fmt == 2 else 3)
    simg, dimg = h * srow + (4 if fmt == 2 else 7), oh * drow + (12 if fmt == 2 else 5)  # unaligned image strides
    sbuf = np.zeros(7 * simg, np.uint8)
    for b, f in enumerate(frames):
        sbuf[b * simg: b * simg + h * srow].reshape(h, srow)[:, : w * bpp] = f.reshape(h, -1).view(np.uint8)
    d_src = ctx.device_upload(sbuf)
    d_dst = ctx.device_upload(np.full(7 * dimg, 0xAB, np.uint8))
    try:
        ctx.warp_perspective_device(d_src, simg, 7, w, h, srow, fmt, Ms, d_dst, dimg, ow, oh, drow)
        got = ctx.device_download(d_dst, (7 * dimg,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    for b in range(7):
        rows = got[b * dimg: b * dimg + oh * drow].reshape(oh, drow)
        assert (rows[:, ow * bpp:] == 0xAB).all() and (got[b * dimg + oh * drow: (b + 1) * dimg] == 0xAB).all()
        out = np.ascontiguousarray(rows[:, : ow * bpp]).view(DTYPE[fmt]).reshape((oh, ow, 3) if fmt == 1 else (oh, ow))
        assert_same(out, R.warp(frames[b], Ms[b], ow, oh))


def golden_transform(L):
    rows = [[float(v) for v in line.split(",")] for line in open(os.path.join(G, "doc_warp_tform.csv"))]
    t = L.ImageTransform()
    t.width, t.height = 1000, 563
    t.top_left, t.top_right, t.bottom_left, t.bottom_right = [L.Point(r[0], r[1], 0.0) for r in rows[:4]]
    return t


def test_golden_picture_through_the_library(L, ctx):
    _, M, (w, h) = L.rectification_homography(golden_transform(L), 3.0)
    src = np.load(os.path.join(G, "doc_image_gray.npy"))
    gold = np.load(os.path.join(G, "doc_warp_gray.npz"))["gray"]
    got = ctx.warp_perspective(src, M, (w, h))
    assert got.shape == gold.shape == (594, 1132)
    d = np.abs(got.astype(np.int32) - gold.astype(np.int32))
    assert d.mean() <= 1.0 and np.percentile(d, 99) <= 5, (d.mean(), np.percentile(d, 99))
    np.testing.assert_array_equal(got, R.warp(src, M, w, h))


def test_destination_beyond_4_gib(L, ctx):
    """u8x3 rows 2 000 003 bytes apart: the last rows start past 4 GiB."""
    src = frame(1, 300, 200, 9)
    ow, oh, drow = 2000, 2200, 2_000_003
    span = (oh - 1) * drow + ow * 3
    assert span > 2**32 + 10**8
    M = np.array([[0.15, 0.01, 0.0], [0.0, 1.0, -(oh - 160.0)], [0.0, 0.0, 1.0]])
    p = C.c_void_p()
    assert L.lib().lr_device_malloc(ctx._h, span, C.byref(p)) == 0, L.lib().lr_last_error()
    d_dst = p.value
    d_src = ctx.device_upload(src)
    try:
        ctx.warp_perspective_device(d_src, src.nbytes, 1, 300, 200, 900, 1, M, d_dst, span, ow, oh, drow)
        first = oh - 40
        blk = ctx.device_download(d_dst + first * drow, ((oh - first - 1) * drow + ow * 3,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    assert first * drow > 2**32
    got = np.stack([blk[i * drow: i * drow + ow * 3] for i in range(oh - first)]).reshape(oh - first, ow, 3)
    exp = R.warp(src, M, ow, oh, rows=np.arange(first, oh))
    assert exp.any()
    np.testing.assert_array_equal(got, exp)


def test_source_row_stride_beyond_2_gib(L, ctx):
    """Three u8 source rows 2^31 + 77 bytes apart; only those rows are uploaded."""
    w, h, srow = 500, 3, 2**31 + 77
    src = frame(0, w, h, 21)
    span = (h - 1) * srow + w
    p = C.c_void_p()
    assert L.lib().lr_device_malloc(ctx._h, span, C.byref(p)) == 0, L.lib().lr_last_error()
    d_src = p.value
    ow, oh = 400, 300
    d_dst = ctx.device_upload(np.zeros(ow * oh, np.uint8))
    M = np.array([[1.2, 0.05, 0.0], [0.0, 0.0095, 0.0], [0.0, 0.0, 1.0]])
    try:
        for r in range(h):
            row = np.ascontiguousarray(src[r])
            assert L.lib().lr_memcpy_h2d(ctx._h, C.c_void_p(d_src + r * srow), row.ctypes.data_as(C.c_void_p), w) == 0
        ctx.warp_perspective_device(d_src, span, 1, w, h, srow, 0, M, d_dst, ow * oh, ow, oh, ow)
        got = ctx.device_download(d_dst, (oh, ow), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    exp = R.warp(src, M, ow, oh)
    assert exp[oh // 2:].any()
    np.testing.assert_array_equal(got, exp)


def test_batch_detector_then_one_batched_warp(L, ctx):
    from librectify_amd import synth

    w, h, B = 640, 480, 3
    frames = np.stack([synth.frame(w, h, 40 + b) for b in range(B)]).astype(np.float32)
    d = ctx.device_upload(frames)
    cfg = L.RectificationConfig(hmin=2.0)
    try:
        _, n, tf = ctx.find_line_segment_groups_batch_device(d, w * h, B, w, h, max(w, h) / 100.0, cfg=cfg)
        assert (n > 10).all()
        hom = [L.rectification_homography(tf[b], 3.0) for b in range(B)]
        ow, oh = max(x[2][0] for x in hom), max(x[2][1] for x in hom)
        Ms = np.stack([x[1] for x in hom])
        d_out = ctx.device_upload(np.zeros(B * ow * oh, np.float32))
        try:
            ctx.warp_perspective_device(d, w * h * 4, B, w, h, w * 4, 2, Ms, d_out, ow * oh * 4, ow, oh, ow * 4)
            got = ctx.device_download(d_out, (B, oh, ow), np.float32)
        finally:
            ctx.device_free(d_out)
    finally:
        ctx.device_free(d)
    for b in range(B):
        single = ctx.warp_perspective(frames[b], Ms[b], (ow, oh))
        assert_same(got[b], single)
        assert_same(single, R.warp(frames[b], Ms[b], ow, oh))


def synthetic_rgb(w, h, seed):
    from librectify_amd import synth

    g = np.clip(synth.frame(w, h, seed) * 255.0, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))


def test_context_rectify_on_synthetic_rgb(L, ctx):
    for w, h, seed in ((480, 360, 3), (777, 401, 4)):
        rgb = synthetic_rgb(w, h, seed)
        lines, t, warped = ctx.rectify(rgb)
        c = rgb.astype(np.int32)
        luma = ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.float32) / np.float32(256)
        ref = ctx.find_line_segment_groups(luma, max(w, h) / 100.0)
        assert len(lines) == len(ref) > 10 and lines.tobytes() == ref.tobytes()
        T = L.compute_rectification_transform(ref, w, h, L.RectificationConfig(hmin=2.0))
        np.testing.assert_array_equal(t.as_array(), T.as_array())
        _, M, size = L.rectification_homography(T, 3.0)
        assert warped.shape == (size[1], size[0], 3)
        np.testing.assert_array_equal(warped, ctx.warp_perspective(rgb, M, size))
        np.testing.assert_array_equal(warped, R.warp(rgb, M, *size))


def read_pnm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    ch = 3 if parts[0] == b"P6" else 1
    a = np.frombuffer(parts[3], np.uint8)
    return a.reshape((h, w, 3) if ch == 3 else (h, w))


def test_recipe_warp_writes_what_the_library_computes(L, ctx, tmp_path):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (gray.shape[1], gray.shape[0]) + gray.tobytes())
    r = subprocess.run([exe, pgm, str(tmp_path / "doc"), "--warp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, _, want = ctx.rectify(gray)
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "doc_warp.pgm")), want)

    rgb = synthetic_rgb(480, 360, 7)
    ppm = str(tmp_path / "syn.ppm")
    with open(ppm, "wb") as f:
        f.write(b"P6\n480 360\n255\n" + rgb.tobytes())
    r = subprocess.run([exe, ppm, str(tmp_path / "syn"), "--warp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, t, want = ctx.rectify(rgb)
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "syn_warp.ppm")), want)


def test_bad_arguments_fail_cleanly_and_leave_the_context_usable(L, ctx):
    lib = L.lib()
    src = frame(1, 64, 48, 2)
    d_src = ctx.device_upload(src)
    d_dst = ctx.device_upload(np.zeros(64 * 48 * 4, np.uint8))
    M = np.eye(3).reshape(-1).copy()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nan = M.copy()
    nan[4] = np.nan
    inf = M.copy()
    inf[8] = np.inf
    good = dict(src=d_src, sib=64 * 48 * 3, batch=1, w=64, h=48, srow=64 * 3, fmt=1, M=P(M), dst=d_dst, dib=64 * 48 * 3, ow=64, oh=48, drow=64 * 3)
    bad = [
        dict(src=0), dict(dst=0), dict(M=None), dict(batch=0), dict(batch=-3), dict(w=0), dict(h=-1), dict(ow=0), dict(oh=0),
        dict(srow=64 * 3 - 1), dict(drow=10), dict(fmt=3), dict(fmt=-1), dict(M=P(nan)), dict(M=P(inf)),
        dict(fmt=2, srow=64 * 4 + 2, drow=64 * 4, sib=48 * 64 * 4 + 2),  # f32 stride not 4-byte aligned
        dict(fmt=2, src=d_src + 2, srow=64 * 4, drow=64 * 4),  # f32 pointer not 4-byte aligned
        dict(fmt=2, dst=d_dst + 1, srow=64 * 4, drow=64 * 4),  # f32 destination not 4-byte aligned
        dict(batch=2, sib=100),  # image stride shorter than a frame
    ]
    try:
        for k, change in enumerate(bad):
            a = dict(good)
            a.update(change)
            rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(a["src"]), a["sib"], a["batch"], a["w"], a["h"], a["srow"], a["fmt"], a["M"],
                                                C.c_void_p(a["dst"]), a["dib"], a["ow"], a["oh"], a["drow"])
            assert rc != 0, (k, change)
            assert lib.lr_last_error().decode().startswith("lr_warp_perspective_device"), (k, lib.lr_last_error())
            # and the next call on the same context is still right
            ctx.warp_perspective_device(d_src, 64 * 48 * 3, 1, 64, 48, 64 * 3, 1, M, d_dst, 64 * 48 * 3, 64, 48, 64 * 3)
            assert_same(ctx.device_download(d_dst, (48, 64, 3), np.uint8), src)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
