"""LR_WARP_CUBIC on the GPU against its NumPy second source (tests/numpy_warp_cubic_ref.py), bit for bit: three pixel
formats, sources smaller than the 4 x 4 support, padded and odd strides, every map of the bilinear warp's test, a few tiles
and many, the packed and the ragged launch; the same calls without the bit against the bilinear source; what is refused;
the Python paths (rectify, rectify_batch, jpeg=) and the recipe's --cubic."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_cubic_ref as RC
import numpy_warp_ref as R
from test_gpu_rectify_warp import BPP, DTYPE, assert_same, frame, maps, read_pnm, synthetic_rgb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CUBIC = 0x8000
SENTINEL = 0xAB


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


def ref(src, M, ow, oh, opts):
    return RC.warp(src, M, ow, oh) if opts & CUBIC else R.warp(src, M, ow, oh)


def content(fmt, w, h, seed):
    """random pixels; 8-bit frames of some size carry a patch of 0 / 255 squares of two pixels, so both clamps fire"""
    a = frame(fmt, w, h, seed)
    if fmt != 2 and w >= 5 and h >= 5:
        ph, pw = min(h, 24), min(w, 40)
        b = (((np.arange(ph)[:, None] // 2 + np.arange(pw)[None, :] // 2) & 1) * 255).astype(np.uint8)
        a[:ph, :pw] = b[..., None] if fmt == 1 else b
    return a


def run_warp(ctx, src, fmt, opts, M, ow, oh, src_pad, dst_pad, src_off=0, dst_off=0):
    """One frame through padded rows at a byte offset from the allocation (test_gpu_rectify_warp.run_warp with option bits);
    checks that no byte outside the output's pixels was written."""
    bpp = BPP[fmt]
    h, w = src.shape[:2]
    srow, drow = w * bpp + src_pad, ow * bpp + dst_pad
    sbuf = np.full(src_off + h * srow, 0x5A, np.uint8)
    sbuf[src_off:].reshape(h, srow)[:, : w * bpp] = np.ascontiguousarray(src).reshape(h, -1).view(np.uint8)
    dbuf = np.full(dst_off + oh * drow, SENTINEL, np.uint8)
    d_src, d_dst = ctx.device_upload(sbuf), ctx.device_upload(dbuf)
    try:
        ctx.warp_perspective_device(d_src + src_off, h * srow, 1, w, h, srow, fmt | opts, M, d_dst + dst_off, oh * drow, ow, oh, drow)
        got = ctx.device_download(d_dst, dbuf.shape, np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    assert (got[:dst_off] == SENTINEL).all()
    rows = got[dst_off:].reshape(oh, drow)
    assert (rows[:, ow * bpp:] == SENTINEL).all(), "bytes beyond a row's pixels were written"
    out = np.ascontiguousarray(rows[:, : ow * bpp]).view(DTYPE[fmt])
    return out.reshape((oh, ow, 3) if fmt == 1 else (oh, ow))


# 1 x 1 and 2 x 3 are smaller than the support, so every tap is fetched on its own; in the larger ones the one-load path and
# the tap-by-tap path meet inside a row, at odd addresses (the offsets and strides below)
SMALL = [(1, 1), (2, 3), (5, 5), (63, 17), (257, 131)]


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("w,h", SMALL)
def test_bit_exact_small_shapes_every_map(ctx, fmt, w, h):
    src = content(fmt, w, h, 11 + w)
    ow, oh = w + w // 3 + 1, h + h // 5 + 1
    pads = (3, 5, 1, 1) if fmt != 2 else (4, 12, 4, 8)  # odd / padded strides; f32 stays 4-byte aligned
    for k, (name, M) in enumerate(maps(w, h, ow, oh).items()):
        sp, dp = pads[k % 2], pads[(k + 1) % 2]
        off = (k % 3) * pads[2]
        for opts in (CUBIC, 0):  # (without the bit the call is the bilinear warp it was)
            got = run_warp(ctx, src, fmt, opts, M, ow, oh, sp, dp, src_off=off, dst_off=pads[3] * (k % 2))
            assert_same(got, ref(src, M, ow, oh, opts)), (name, opts)
            if name == "identity":
                assert_same(got[:h, :w], src)
                assert not got[h:].any() and not got[:, w:].any()


@pytest.mark.parametrize("fmt", [0, 1])
def test_a_checkerboard_fires_both_clamps(ctx, fmt):
    w, h, ow, oh = 40, 24, 97, 61
    src = content(fmt, w, h, 1)
    m = maps(w, h, ow, oh)
    for name in ("scale_up", "rotation"):
        stats = {}
        exp = RC.warp(src, m[name], ow, oh, stats=stats)
        low = RC.warp_f64(src, m[name], ow, oh)
        assert stats["max_abs_s"] > 255 << 22 and (exp == 255).any() and ((exp == 0) & (low == 0.0)).any()
        assert_same(run_warp(ctx, src, fmt, CUBIC, m[name], ow, oh, 3, 1, src_off=1, dst_off=3), exp)


# outputs of one pixel, exactly one tile and one pixel over in each direction (four tiles, a partial lane at the right edge)
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("ow,oh,batch", [(1, 1, 1), (64, 16, 1), (65, 17, 1), (65, 17, 3)])
def test_outputs_of_a_few_tiles(ctx, fmt, ow, oh, batch):
    w, h = 70, 20
    bpp = BPP[fmt]
    frames = [content(fmt, w, h, 40 + b) for b in range(batch)]
    m = maps(w, h, ow, oh)
    Ms = np.stack([m[name] for name in ("rotation", "identity", "perspective")[:batch]])
    srow, drow = w * bpp + (4 if fmt == 2 else 1), ow * bpp + (4 if fmt == 2 else 3)
    simg, dimg = h * srow + (4 if fmt == 2 else 7), oh * drow + (12 if fmt == 2 else 5)
    sbuf = np.zeros(batch * simg, np.uint8)
    for b, f in enumerate(frames):
        sbuf[b * simg: b * simg + h * srow].reshape(h, srow)[:, : w * bpp] = f.reshape(h, -1).view(np.uint8)
    d_src = ctx.device_upload(sbuf)
    d_dst = ctx.device_upload(np.full(batch * dimg, SENTINEL, np.uint8))
    try:
        for opts in (CUBIC, 0):
            ctx.warp_perspective_device(d_src, simg, batch, w, h, srow, fmt | opts, Ms, d_dst, dimg, ow, oh, drow)
            got = ctx.device_download(d_dst, (batch * dimg,), np.uint8)
            for b in range(batch):
                rows = got[b * dimg: b * dimg + oh * drow].reshape(oh, drow)
                assert (rows[:, ow * bpp:] == SENTINEL).all() and (got[b * dimg + oh * drow: (b + 1) * dimg] == SENTINEL).all()
                out = np.ascontiguousarray(rows[:, : ow * bpp]).view(DTYPE[fmt]).reshape((oh, ow, 3) if fmt == 1 else (oh, ow))
                assert_same(out, ref(frames[b], Ms[b], ow, oh, opts))
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_one_frame_of_many_tiles(ctx, fmt):
    """513 x 259: 9 x 17 tiles, some nineteen to each XCD's run"""
    w, h = 513, 259
    src = content(fmt, w, h, 5)
    m = maps(w, h, w, h)
    pad = 4 if fmt == 2 else 3
    for name in ("identity", "perspective", "rotation"):
        got = run_warp(ctx, src, fmt, CUBIC, m[name], w, h, pad, pad + (4 if fmt == 2 else 2), src_off=pad)
        assert_same(got, RC.warp(src, m[name], w, h))
        if name == "identity":
            assert_same(got, src)


def six_frames(fmt, same_source):
    """six frames' sources, maps and output sizes: a 1 x 1 source and a 1 x 1 output among them"""
    src_sizes = [(70, 20)] * 6 if same_source else [(70, 20), (1, 1), (33, 47), (5, 5), (129, 31), (70, 20)]
    out_sizes = [(65, 17), (3, 2), (1, 1), (64, 16), (130, 33), (31, 50)]
    names = ("rotation", "identity", "perspective", "scale_up", "shift", "horizon")
    frames = [content(fmt, w, h, 70 + b) for b, (w, h) in enumerate(src_sizes)]
    Ms = [maps(w, h, ow, oh)[n] for (w, h), (ow, oh), n in zip(src_sizes, out_sizes, names)]
    return frames, Ms, out_sizes


def destination_table(out_sizes, bpp, cols):
    """outputs in an order of their own, with gaps between them and padded rows"""
    step = 4 if bpp == 4 else 1
    table = np.zeros((len(out_sizes), cols), np.float64)
    cursor = 8
    for b in (3, 0, 5, 1, 4, 2):
        ow, oh = out_sizes[b]
        row = ow * bpp + (3, 0, 5)[b % 3] * step
        table[b, 9:13] = (ow, oh, cursor, row)
        cursor += (oh - 1) * row + ow * bpp + (2, 7, 0)[b % 3] * step
    return table, cursor + 12


def check_region(L, ctx, got, table, frames, Ms, fmt, opts):
    """every frame is the reference's and the single-frame call's; nothing else in the region was written"""
    bpp = BPP[fmt]
    written = np.zeros(got.shape, bool)
    for b, f in enumerate(frames):
        ow, oh, off, row = (int(v) for v in table[b, 9:13])
        rows = np.lib.stride_tricks.as_strided(got[off:], (oh, ow * bpp), (row, 1))
        np.lib.stride_tricks.as_strided(written[off:], (oh, ow * bpp), (row, 1))[:] = True
        out = np.ascontiguousarray(rows).view(DTYPE[fmt]).reshape((oh, ow, 3) if fmt == 1 else (oh, ow))
        assert_same(out, ref(f, Ms[b], ow, oh, opts)), b
        assert_same(out, ctx.warp_perspective(f, Ms[b], (ow, oh), interp="cubic" if opts & CUBIC else "linear")), b
    assert (got[~written] == SENTINEL).all(), "bytes outside the frames' pixels were written"


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_packed_launch_of_six_frames(L, ctx, fmt):
    bpp = BPP[fmt]
    frames, Ms, out_sizes = six_frames(fmt, True)
    w, h = 70, 20
    srow = w * bpp + (4 if fmt == 2 else 1)
    simg = h * srow + (4 if fmt == 2 else 7)
    sbuf = np.full(6 * simg, 0x5A, np.uint8)
    for b, f in enumerate(frames):
        sbuf[b * simg: b * simg + h * srow].reshape(h, srow)[:, : w * bpp] = f.reshape(h, -1).view(np.uint8)
    table, region = destination_table(out_sizes, bpp, 13)
    table[:, :9] = np.stack(Ms).reshape(6, 9)
    d_src = ctx.device_upload(sbuf)
    try:
        for opts in (CUBIC, 0):
            d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
            try:
                ctx.warp_perspective_packed_device(d_src, simg, 6, w, h, srow, fmt | opts, table, d_dst, region)
                got = ctx.device_download(d_dst, (region,), np.uint8)
            finally:
                ctx.device_free(d_dst)
            check_region(L, ctx, got, table, frames, Ms, fmt, opts)
    finally:
        ctx.device_free(d_src)


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ragged_launch_of_six_frames(L, ctx, fmt):
    bpp = BPP[fmt]
    step = 4 if bpp == 4 else 1
    frames, Ms, out_sizes = six_frames(fmt, False)
    frames[5] = frames[0]  # (a shared source: frames 0 and 5 read the same bytes)
    table, region = destination_table(out_sizes, bpp, 18)
    table[:, :9] = np.stack(Ms).reshape(6, 9)
    cursor, places = 3 * step, []
    for b, f in enumerate(frames[:5]):
        h, w = f.shape[:2]
        row = w * bpp + (1, 3, 0)[b % 3] * step
        places.append((w, h, cursor, row))
        cursor += (h - 1) * row + w * bpp + (5, 0, 2)[b % 3] * step
    places.append(places[0])
    sbuf = np.full(cursor, 0x5A, np.uint8)  # (the last source ends with the region: nothing lies behind its last pixel)
    for f, (w, h, off, row) in zip(frames[:5], places):
        np.lib.stride_tricks.as_strided(sbuf[off:], (h, w * bpp), (row, 1))[:] = f.reshape(h, -1).view(np.uint8)
    table[:, 13:17] = places
    d_src = ctx.device_upload(sbuf)
    try:
        for opts in (CUBIC, 0):
            d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
            try:
                ctx.warp_perspective_ragged_device(d_src, len(sbuf), fmt | opts, table, d_dst, region)
                got = ctx.device_download(d_dst, (region,), np.uint8)
            finally:
                ctx.device_free(d_dst)
            check_region(L, ctx, got, table, frames, Ms, fmt, opts)
    finally:
        ctx.device_free(d_src)


def test_refusals_leave_the_destination_and_the_context_as_they_were(L, ctx):
    lib = L.lib()
    w, h = 64, 48
    src = frame(1, w, h, 2)
    n = w * h * 3
    d_src = ctx.device_upload(src)
    d_dst = ctx.device_upload(np.full(n, SENTINEL, np.uint8))
    M = np.eye(3).reshape(-1).copy()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    packed = np.concatenate([M, [w, h, 0, w * 3]])
    ragged = np.concatenate([M, [w, h, 0, w * 3, w, h, 0, w * 3, 0]])
    ragged17 = ragged.copy()
    ragged17[17] = 1.0
    args = L.JpegArgs()  # (never read: the combination is refused first)
    plain = dict(sib=n, w=w, h=h, srow=w * 3, M=P(M), ow=w, oh=h, drow=w * 3)
    table = dict(sib=n, w=w, h=h, srow=0, ow=w, oh=h, drow=0)
    behind = dict(sib=n, w=0, h=0, srow=0, M=C.cast(C.byref(args), C.c_void_p), ow=0, oh=0, drow=0)
    cases = [
        ("LR_WARP_PREPARE", dict(plain, fmt=1 | L.WARP_PREPARE | CUBIC, M=None)),
        ("LR_WARP_PREPARE", dict(table, fmt=1 | L.WARP_RAGGED | L.WARP_PREPARE | CUBIC, M=P(ragged))),
        ("LR_WARP_LINES", dict(behind, fmt=1 | L.WARP_LINES | CUBIC)),
        ("LR_WARP_JPEG", dict(behind, fmt=1 | L.WARP_JPEG | CUBIC)),
        ("LR_WARP_JPEG_DECODE", dict(behind, fmt=1 | L.WARP_JPEG_DECODE | CUBIC)),
        ("unknown option", dict(plain, fmt=1 | CUBIC | 0x400)),
        ("unknown option", dict(table, fmt=1 | L.WARP_PACKED | CUBIC | 0x10000, M=P(packed), srow=w * 3)),
        ("LR_WARP_PACKED", dict(table, fmt=1 | L.WARP_PACKED | L.WARP_RAGGED | CUBIC, M=P(ragged))),
        ("[17]", dict(table, fmt=1 | L.WARP_RAGGED | CUBIC, M=P(ragged17))),
        ("unknown pixel format", dict(plain, fmt=3 | CUBIC)),
    ]
    try:
        for k, (word, a) in enumerate(cases):
            rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), a["sib"], 1, a["w"], a["h"], a["srow"], a["fmt"], a["M"],
                                                C.c_void_p(d_dst), n, a["ow"], a["oh"], a["drow"])
            err = lib.lr_last_error().decode()
            assert rc != 0, (k, word)
            assert err.startswith("lr_warp_perspective_device") and word in err, (k, word, err)
            if "LR_WARP_" in word and word != "LR_WARP_PACKED":
                assert "LR_WARP_CUBIC" in err, err  # (the message names the combination)
            assert (ctx.device_download(d_dst, (n,), np.uint8) == SENTINEL).all(), (k, word)
        # and the next calls on the same context are right, in all three spellings
        for opts, tbl in ((CUBIC, M), (CUBIC | L.WARP_PACKED, packed), (CUBIC | L.WARP_RAGGED, ragged)):
            srow = 0 if opts & L.WARP_RAGGED else w * 3  # (the ragged table holds the sources' strides, the others the call)
            assert lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), n, 1, w, h, srow, 1 | opts, P(tbl),
                                                  C.c_void_p(d_dst), n, w, h, w * 3 if opts == CUBIC else 0) == 0, lib.lr_last_error()
            assert_same(ctx.device_download(d_dst, (h, w, 3), np.uint8), src)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def gray_of(rgb):
    c = rgb.astype(np.int32)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


@pytest.fixture(scope="module")
def pictures():
    """colour frames of mixed shapes, and their gray versions"""
    rgb = [synthetic_rgb(w, h, seed) for w, h, seed in ((480, 360, 3), (333, 250, 4), (401, 277, 5))]
    return {"colour": rgb, "gray": [gray_of(f) for f in rgb]}


def test_rectify_with_cubic_changes_the_picture_alone(L, ctx, pictures):
    for img in (pictures["colour"][0], pictures["gray"][1]):
        lines, t, warped = ctx.rectify(img, interp="cubic")
        lines0, t0, warped0 = ctx.rectify(img)
        assert lines.tobytes() == lines0.tobytes()
        np.testing.assert_array_equal(t.as_array(), t0.as_array())
        _, M, size = L.rectification_homography(t, 3.0)
        assert warped.shape == warped0.shape == (size[1], size[0]) + img.shape[2:]
        np.testing.assert_array_equal(warped, RC.warp(img, M, *size))
        np.testing.assert_array_equal(warped0, R.warp(img, M, *size))
        assert (warped != warped0).any()
        # the prescaled path ends in the same launch
        _, t2, warped2 = ctx.rectify(img, max_size=400, interp="cubic")
        _, M2, size2 = L.rectification_homography(t2, 3.0)
        np.testing.assert_array_equal(warped2, RC.warp(img, M2, *size2))


@pytest.mark.parametrize("kind", ["gray", "colour"])
def test_rectify_batch_with_cubic_is_a_loop_of_rectify(L, ctx, pictures, kind):
    frames = pictures[kind]
    single = [ctx.rectify(f, interp="cubic") for f in frames]
    assert all(s[2] is not None for s in single)
    batch = ctx.rectify_batch(frames, interp="cubic")  # (mixed shapes: the ragged launch)
    same = ctx.rectify_batch(np.stack([frames[0], frames[0][::-1].copy()]), interp="cubic")  # (one shape: the packed launch)
    same_single = [ctx.rectify(frames[0], interp="cubic"), ctx.rectify(frames[0][::-1].copy(), interp="cubic")]
    for (l, t, img), (l1, t1, img1) in list(zip(batch, single)) + list(zip(same, same_single)):
        assert l.tobytes() == l1.tobytes()
        np.testing.assert_array_equal(t.as_array(), t1.as_array())
        np.testing.assert_array_equal(img, img1)
    streams = ctx.rectify_batch(frames, jpeg=90, interp="cubic")
    for (l, t, stream), (l1, t1, img1) in zip(streams, single):
        assert l.tobytes() == l1.tobytes()
        assert stream == ctx.encode_jpeg(img1, 90)
    assert ctx.rectify(frames[0], jpeg=90, interp="cubic")[2] == streams[0][2]


def test_recipe_warp_cubic_writes_what_the_library_computes(L, ctx, tmp_path):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (gray.shape[1], gray.shape[0]) + gray.tobytes())
    r = subprocess.run([exe, pgm, str(tmp_path / "none"), "--cubic"], capture_output=True, text=True)
    assert r.returncode == 2 and "--cubic" in r.stderr and not os.path.exists(str(tmp_path / "none_lines.csv"))
    r = subprocess.run([exe, pgm, str(tmp_path / "doc"), "--warp", "--cubic"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, _, want = ctx.rectify(gray, interp="cubic")
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "doc_warp.pgm")), want)
    assert (want != ctx.rectify(gray)[2]).any()

    rgb = synthetic_rgb(480, 360, 7)
    ppm = str(tmp_path / "syn.ppm")
    with open(ppm, "wb") as f:
        f.write(b"P6\n480 360\n255\n" + rgb.tobytes())
    r = subprocess.run([exe, ppm, str(tmp_path / "syn"), "--warp", "--cubic"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "syn_warp.ppm")), ctx.rectify(rgb, interp="cubic")[2])
