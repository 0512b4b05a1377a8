"""The prepare step on the GPU (lr_warp_perspective_device with LR_WARP_PREPARE) against its NumPy second source
(tests/numpy_prepare_ref.py), compared as raw uint32: three source formats over scales from 1 to above 64, tiny sizes and
sizes off the tile, padded and odd strides, batches, source offsets beyond 4 GiB; the doc image through
Context.rectify(max_size=...); the detector on a device-prepared frame; the unchanged default; bad arguments; the recipe's
--device-prepare."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_prepare_ref as P

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


def frame(fmt, w, h, seed):
    rng = np.random.default_rng(seed)
    if fmt == 2:
        return (rng.random((h, w), dtype=np.float32) * np.float32(4.0) - np.float32(1.0)).astype(np.float32)
    return rng.integers(0, 256, (h, w, 3) if fmt == 1 else (h, w), dtype=np.uint8)


def assert_same_bits(got, exp):
    assert got.dtype == exp.dtype == np.float32 and got.shape == exp.shape
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))


def run_prepare(ctx, src, fmt, ow, oh, src_pad=0, dst_pad=0, src_off=0, dst_off=0):
    """Prepares one frame through padded rows, at byte offsets from the allocations; returns the f32 output and checks
    that no byte outside the output's pixels was written."""
    bpp = BPP[fmt]
    h, w = src.shape[:2]
    srow, drow = w * bpp + src_pad, ow * 4 + dst_pad
    sbuf = np.full(src_off + h * srow, 0x5A, np.uint8)
    sbuf[src_off:].reshape(h, srow)[:, : w * bpp] = np.ascontiguousarray(src).reshape(h, -1).view(np.uint8)
    dbuf = np.full(dst_off + oh * drow + 64, 0xAB, np.uint8)
    d_src, d_dst = ctx.device_upload(sbuf), ctx.device_upload(dbuf)
    try:
        ctx.prepare_device(d_src + src_off, h * srow, 1, w, h, srow, fmt, d_dst + dst_off, oh * drow, ow, oh, drow)
        got = ctx.device_download(d_dst, dbuf.shape, np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    assert (got[:dst_off] == 0xAB).all() and (got[dst_off + oh * drow:] == 0xAB).all()
    rows = got[dst_off: dst_off + oh * drow].reshape(oh, drow)
    assert (rows[:, ow * 4:] == 0xAB).all(), "bytes beyond a row's pixels were written"
    return np.ascontiguousarray(rows[:, : ow * 4]).view(np.float32).reshape(oh, ow)


SIZES = [  # source width, height -> output width, height
    (67, 45, 67, 45),       # identity
    (130, 66, 65, 33),      # scale 2, one pixel past a tile
    (195, 99, 65, 33),      # scale 3
    (320, 160, 100, 50),    # 3.2
    (270, 108, 250, 100),   # 1.08
    (683, 410, 100, 60),    # 6.83
    (650, 130, 10, 2),      # 65
    (5000, 20, 70, 3),      # 71.4 across: a tile's footprint takes several column chunks
    (40, 700, 5, 3),        # 233 down: many row chunks
    (37, 23, 1, 1),         # output 1 x 1
    (1, 1, 1, 1), (2, 1, 1, 1), (3, 2, 2, 1), (4, 2, 3, 2), (5, 1, 5, 1), (5, 2, 2, 2), (9, 2, 4, 1),  # widths 1-5, heights 1, 2
    (1000, 563, 333, 187),  # neither a multiple of the tile
    (257, 131, 129, 67),
    (130, 10, 65, 5),       # a partial tile in both directions
    (1100, 20, 2, 2),       # a pixel's 550 column taps cross the 512-pixel chunk, its 10 row taps the 8-row chunk
]


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("w,h,ow,oh", SIZES)
def test_bit_exact_formats_and_sizes(ctx, fmt, w, h, ow, oh):
    src = frame(fmt, w, h, 7 + w + 3 * fmt)
    assert_same_bits(run_prepare(ctx, src, fmt, ow, oh), P.prepare(src, ow, oh))


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("w,h,ow,oh", [(3840, 2160, 1200, 675), (1999, 1201, 1200, 721)])
def test_bit_exact_large_frames(ctx, fmt, w, h, ow, oh):
    src = frame(fmt, w, h, 5)
    assert_same_bits(run_prepare(ctx, src, fmt, ow, oh), P.prepare(src, ow, oh))


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_identity_is_the_conversion_alone(ctx, fmt):
    src = frame(fmt, 333, 77, 12)
    got = run_prepare(ctx, src, fmt, 333, 77)
    if fmt == 2:
        exp = src + np.float32(0.0)  # (0 + 1 * p: -0.0 becomes +0.0, everything else is itself)
    else:
        c = src.astype(np.int64)
        luma = src if fmt == 0 else (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
        exp = luma.astype(np.float32) / np.float32(256.0)
    assert_same_bits(got, exp)


def test_u8x3_source_whose_first_byte_is_at_an_odd_offset(ctx):
    """the unaligned row start of the staging fetch, on the shapes that walk a partial tile and both chunk loops"""
    for w, h, ow, oh in ((130, 10, 65, 5), (1100, 20, 2, 2), (1, 1, 1, 1)):
        src = frame(1, w, h, 50 + w)
        for src_off, src_pad in ((1, 0), (3, 2)):
            assert_same_bits(run_prepare(ctx, src, 1, ow, oh, src_pad=src_pad, src_off=src_off), P.prepare(src, ow, oh))


def test_trim_frees_the_span_table_and_the_next_call_makes_it_again(ctx):
    src = frame(1, 320, 160, 44)
    exp = P.prepare(src, 100, 50)
    assert_same_bits(run_prepare(ctx, src, 1, 100, 50), exp)
    ctx.trim()
    assert_same_bits(run_prepare(ctx, src, 1, 100, 50), exp)  # the same size pair: no stale table
    assert_same_bits(run_prepare(ctx, src, 1, 320, 160), P.prepare(src, 320, 160))


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_padded_and_odd_strides(ctx, fmt):
    w, h, ow, oh = 301, 97, 94, 31
    src = frame(fmt, w, h, 31)
    exp = P.prepare(src, ow, oh)
    # u8x3 with w * 3 + 2 = 905 bytes a row: rows start at every alignment; f32 stays 4-byte aligned
    for src_pad, dst_pad, src_off, dst_off in ((0, 0, 0, 0), (2, 4, 1, 4), (5, 12, 3, 8), (7, 0, 2, 0)):
        if fmt == 2:
            src_pad, src_off = 4 * src_pad, 4 * src_off
        assert_same_bits(run_prepare(ctx, src, fmt, ow, oh, src_pad, dst_pad, src_off, dst_off), exp)


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_batch_with_image_strides_larger_than_a_frame(ctx, fmt):
    w, h, ow, oh, B = 257, 131, 80, 41, 5
    bpp = BPP[fmt]
    frames = [frame(fmt, w, h, 100 + b) for b in range(B)]
    srow, drow = w * bpp + (4 if fmt == 2 else 1), ow * 4 + 8
    simg, dimg = h * srow + (12 if fmt == 2 else 7), oh * drow + 20
    sbuf = np.zeros(B * simg, np.uint8)
    for b, f in enumerate(frames):
        sbuf[b * simg: b * simg + h * srow].reshape(h, srow)[:, : w * bpp] = f.reshape(h, -1).view(np.uint8)
    d_src = ctx.device_upload(sbuf)
    d_dst = ctx.device_upload(np.full(B * dimg, 0xAB, np.uint8))
    try:
        ctx.prepare_device(d_src, simg, B, w, h, srow, fmt, d_dst, dimg, ow, oh, drow)
        got = ctx.device_download(d_dst, (B * dimg,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    for b in range(B):
        rows = got[b * dimg: b * dimg + oh * drow].reshape(oh, drow)
        assert (rows[:, ow * 4:] == 0xAB).all() and (got[b * dimg + oh * drow: (b + 1) * dimg] == 0xAB).all()
        out = np.ascontiguousarray(rows[:, : ow * 4]).view(np.float32).reshape(oh, ow)
        assert_same_bits(out, P.prepare(frames[b], ow, oh))
    single = ctx.prepare(np.stack(frames), 80) if fmt != 2 else None
    if single is not None:  # Context.prepare on the same batch: prepared_size(257, 131, 80) = (80, 41)
        assert single.shape == (B, oh, ow)
        for b in range(B):
            assert_same_bits(single[b], P.prepare(frames[b], ow, oh))


def test_batch_whose_source_offsets_pass_4_gib(L, ctx):
    """Three u8x3 frames 2^31 + 77 bytes apart: the third starts past 4 GiB.  Only the frames are uploaded."""
    w, h, ow, oh, sib = 300, 200, 94, 63, 2**31 + 77
    frames = [frame(1, w, h, 60 + b) for b in range(3)]
    span = 2 * sib + w * h * 3
    assert 2 * sib > 2**32
    p = C.c_void_p()
    assert L.lib().lr_device_malloc(ctx._h, span, C.byref(p)) == 0, L.lib().lr_last_error()
    d_src = p.value
    d_dst = ctx.device_upload(np.zeros(3 * ow * oh, np.float32))
    try:
        for b, f in enumerate(frames):
            assert L.lib().lr_memcpy_h2d(ctx._h, C.c_void_p(d_src + b * sib), f.ctypes.data_as(C.c_void_p), f.nbytes) == 0
        ctx.prepare_device(d_src, sib, 3, w, h, w * 3, 1, d_dst, ow * oh * 4, ow, oh, ow * 4)
        got = ctx.device_download(d_dst, (3, oh, ow), np.float32)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    for b in range(3):
        assert_same_bits(got[b], P.prepare(frames[b], ow, oh))


def test_doc_image_repeated_2x2_is_pinned_to_the_unscaled_run(L, ctx):
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    assert gray.shape == (563, 1000) and gray.dtype == np.uint8
    big = np.ascontiguousarray(np.repeat(np.repeat(gray, 2, axis=0), 2, axis=1))
    assert L.prepared_size(2000, 1126, 1000) == (1000, 563, np.float32(0.5))
    assert_same_bits(ctx.prepare(big, 1000), gray.astype(np.float32) / np.float32(256.0))
    small_lines, _, _ = ctx.rectify(gray)  # min_length 10 in both runs
    lines, t, warped = ctx.rectify(big, max_size=1000)
    assert len(lines) == len(small_lines) > 10
    np.testing.assert_array_equal(lines["group_id"], small_lines["group_id"])
    for k in ("x1", "y1", "x2", "y2"):
        assert_same_bits(lines[k], small_lines[k] * np.float32(2.0))
    for k in ("weight", "err"):
        assert_same_bits(lines[k], small_lines[k])
    # the transform is the full frame's and the warp reads the 8-bit frame itself
    T = L.compute_rectification_transform(lines, 2000, 1126, L.RectificationConfig(hmin=2.0))
    np.testing.assert_array_equal(t.as_array(), T.as_array())
    _, M, size = L.rectification_homography(T, 3.0)
    np.testing.assert_array_equal(warped, ctx.warp_perspective(big, M, size))


def synthetic_u8(w, h, seed):
    from librectify_amd import synth

    return np.clip(synth.frame(w, h, seed) * 255.0, 0, 255).astype(np.uint8)


def test_detector_on_a_device_prepared_frame_equals_the_host_frame(L, ctx):
    w, h = 3840, 2160
    src = synthetic_u8(w, h, 3)
    ow, oh, scale = L.prepared_size(w, h, 1200)
    assert (ow, oh) == (1200, 675)
    host_frame = P.prepare(src, ow, oh)
    d_src = ctx.device_upload(src)
    d_small = ctx.device_upload(np.zeros((oh, ow), np.float32))
    try:
        ctx.prepare_device(d_src, src.nbytes, 1, w, h, w, 0, d_small, ow * oh * 4, ow, oh, ow * 4)
        got = ctx.find_line_segment_groups_device(d_small, ow, oh, 12.0).copy()
        frame_back = ctx.device_download(d_small, (oh, ow), np.float32)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_small)
    assert_same_bits(frame_back, host_frame)
    ref = ctx.find_line_segment_groups(host_frame, 12.0)
    assert len(got) == len(ref) > 50 and got.tobytes() == ref.tobytes()
    # and Context.rectify(max_size=1200) is those lines, scaled back in float32
    lines, _, _ = ctx.rectify(src, max_size=1200)
    assert len(lines) == len(ref)
    for k in ("x1", "y1", "x2", "y2"):
        assert_same_bits(lines[k], ref[k] / scale)


def test_rectify_without_max_size_is_what_it_was(L, ctx):
    g = synthetic_u8(480, 360, 3)
    rgb = np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))
    for img in (g, rgb):
        lines, t, warped = ctx.rectify(img)
        again = ctx.rectify(img, max_size=None)
        if img.ndim == 3:
            c = img.astype(np.int32)
            gray = (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
        else:
            gray = img
        luma = gray.astype(np.float32) / np.float32(256.0)
        ref = ctx.find_line_segment_groups(luma, 480 / 100.0)
        assert len(ref) > 10 and lines.tobytes() == ref.tobytes() == again[0].tobytes()
        T = L.compute_rectification_transform(ref, 480, 360, L.RectificationConfig(hmin=2.0))
        np.testing.assert_array_equal(t.as_array(), T.as_array())
        np.testing.assert_array_equal(again[1].as_array(), T.as_array())
        _, M, size = L.rectification_homography(T, 3.0)
        want = ctx.warp_perspective(img, M, size)
        np.testing.assert_array_equal(warped, want)
        np.testing.assert_array_equal(again[2], want)


def test_failing_calls_fail_with_a_message_and_write_nothing(L, ctx):
    lib = L.lib()
    w, h, ow, oh = 64, 48, 32, 24
    src = frame(1, w, h, 2)
    d_src = ctx.device_upload(src)
    band = 256
    dbytes = band + w * h * 4 + band  # room for the (refused) identity-size outputs too
    d_buf = ctx.device_upload(np.full(dbytes, 0xAB, np.uint8))
    d_dst = d_buf + band
    PREP = L.WARP_PREPARE
    good = dict(src=d_src, sib=w * h * 3, batch=1, w=w, h=h, srow=w * 3, fmt=1 | PREP, M=None, dst=d_dst, dib=ow * oh * 4, ow=ow, oh=oh, drow=ow * 4)
    bad = [
        dict(fmt=1 | 0x200), dict(fmt=1 | PREP | 0x200), dict(fmt=1 | PREP | 0x10000), dict(fmt=1 | 0x400), dict(fmt=1 | PREP | (1 << 30)),  # other option bits
        dict(fmt=3 | PREP), dict(fmt=0xFF | PREP), dict(fmt=3), dict(fmt=-1),  # unknown low byte
        dict(ow=w + 1), dict(oh=h + 1), dict(ow=w + 1, oh=h + 1, drow=(w + 1) * 4),  # no upscaling
        dict(dst=d_dst + 1), dict(dst=d_dst + 2), dict(drow=ow * 4 + 2), dict(drow=ow * 4 - 4), dict(drow=ow * 4 - 1),
        dict(batch=2, sib=w * h * 3, dib=ow * oh * 4 + 2),  # image stride of the destination not 4-byte aligned
        dict(src=0), dict(dst=0), dict(batch=0), dict(batch=-3), dict(w=0), dict(h=-1), dict(ow=0), dict(oh=0),
        dict(srow=w * 3 - 1), dict(batch=2, sib=100), dict(batch=2, dib=100),
        dict(fmt=2 | PREP, srow=w * 4 + 2), dict(fmt=2 | PREP, src=d_src + 2, srow=w * 4),  # f32 source alignment
    ]
    try:
        for k, change in enumerate(bad):
            a = dict(good)
            a.update(change)
            rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(a["src"]), a["sib"], a["batch"], a["w"], a["h"], a["srow"], a["fmt"], a["M"],
                                                C.c_void_p(a["dst"]), a["dib"], a["ow"], a["oh"], a["drow"])
            assert rc != 0, (k, change)
            msg = lib.lr_last_error().decode()
            assert msg.startswith("lr_warp_perspective_device") and len(msg) > len("lr_warp_perspective_device: "), (k, msg)
            assert (ctx.device_download(d_buf, (dbytes,), np.uint8) == 0xAB).all(), (k, change, "a refused call wrote")
        # M is ignored and may be NULL or anything; the call after the refused ones is right and stays inside its rows
        for M in (None, np.full(9, np.nan)):
            ptr = None if M is None else M.ctypes.data_as(C.c_void_p)
            assert lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), w * h * 3, 1, w, h, w * 3, 1 | PREP, ptr, C.c_void_p(d_dst),
                                                  ow * oh * 4, ow, oh, ow * 4) == 0, lib.lr_last_error()
            got = ctx.device_download(d_buf, (dbytes,), np.uint8)
            assert (got[:band] == 0xAB).all() and (got[band + ow * oh * 4:] == 0xAB).all()
            assert_same_bits(got[band: band + ow * oh * 4].view(np.float32).reshape(oh, ow), P.prepare(src, ow, oh))
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_buf)


def test_recipe_device_prepare_writes_the_same_csv_files(L, ctx, tmp_path):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (gray.shape[1], gray.shape[0]) + gray.tobytes())
    g = synthetic_u8(777, 401, 7)
    rgb = np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))
    ppm = str(tmp_path / "syn.ppm")
    with open(ppm, "wb") as f:
        f.write(b"P6\n777 401\n255\n" + rgb.tobytes())
    for path, name in ((pgm, "doc"), (ppm, "syn")):
        for flag in ([], ["--device-prepare"]):
            prefix = str(tmp_path / (name + ("_dev" if flag else "_host")))
            r = subprocess.run([exe, path, prefix, "--max-size", "500"] + flag, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
        for kind in ("_lines.csv", "_tform.csv"):
            host = open(str(tmp_path / (name + "_host" + kind)), "rb").read()
            dev = open(str(tmp_path / (name + "_dev" + kind)), "rb").read()
            assert len(host) > 0 and host == dev, (name, kind)
        assert len(open(str(tmp_path / (name + "_host_lines.csv"))).readlines()) > 10
