"""LR_JPEG_SCALED on the GPU: lr_decode_jpeg_device with the bit and a scale denominator in entry [6] (kernels_jpeg_decode.hip,
the kScaled instantiations of the transform and the output pass) against tests/numpy_jpeg_scale_ref.py, byte for byte.  Every
status-0 file of the two fixture sets at 1/2, 1/4 and 1/8 into both output formats, at places of its own with wider strides and
guard bytes; one batch that mixes the four scales with a progressive file, a damaged scan and a frame allocated at the full
size; EXIF orientations of both shapes of the output pass on reduced pictures; the streams of several workgroups; the
pipeline on files, and the C recipe.  On the parent commit the bit is refused, so every test here fails there."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import numpy_jpeg_orient_ref as X
import numpy_jpeg_sampling_ref as S
import numpy_jpeg_scale_ref as Z

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = os.path.join(ROOT, "tests", "golden")
GUARD = 0xAB


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


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(G, "jpeg_sampling_kat.npz"))


@pytest.fixture(scope="module")
def old():
    return np.load(os.path.join(G, "jpeg_decode_kat.npz"))


@pytest.fixture(scope="module")
def doc():
    with open(os.path.join(G, "doc_image.jpg"), "rb") as f:
        return f.read()


_wanted = {}


def wanted(stream, N, fmt, orient=False):
    """the restatement's picture, computed once per (stream, scale, format, orient) and never changed"""
    key = (stream, N, fmt, orient)
    if key not in _wanted:
        status, img = Z.decode(stream, N, fmt, orient=orient)
        assert status == 0
        img.setflags(write=False)
        _wanted[key] = img
    return _wanted[key]


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d values differ, the first at %s" % (what, len(bad), bad[0].tolist()))


def batch_call(L, ctx, streams, fmt, sizes, order, scale, bit=True, orient=False, pad=7, gap=13):
    """tests/test_gpu_jpeg_sampling.py's, with entry [6]: the streams one behind the other (odd gaps), the pictures in `order`,
    each allocated for sizes[b], rows padded by `pad` bytes and `gap` guard bytes between and around them.  Returns (info, the
    destination region, per stream its (offset, row bytes, w, h))."""
    bpp = 3 if fmt == L.PIX_U8X3 else 1
    offs, end = [], 3
    for s in streams:
        offs.append(end)
        end += len(s) + 5
    region = np.full(end, 0x11, np.uint8)
    for s, o in zip(streams, offs):
        region[o:o + len(s)] = np.frombuffer(s, np.uint8)
    places, at = {}, gap
    for b in order:
        w, h = sizes[b]
        places[b] = (at, w * bpp + pad, w, h)
        at += h * (w * bpp + pad) + gap
    table = L.jpeg_decode_table([(o, len(s)) for s, o in zip(streams, offs)], [places[b][:2] for b in range(len(streams))],
                                [places[b][2:] for b in range(len(streams))], orient=orient, scale=scale)
    d_src, d_dst = ctx.device_upload(region), ctx.device_upload(np.full(at, GUARD, np.uint8))
    try:
        info = ctx.decode_jpeg_device(d_src, region, fmt | L.JPEG_ANY_SAMPLING | (L.JPEG_SCALED if bit else 0), table, d_dst, at)
        return info, ctx.device_download(d_dst, (at,), np.uint8), places
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def pictures_and_guards(dst, places, bpp):
    """(per stream its picture, a mask of the bytes that belong to no picture)"""
    free = np.ones(len(dst), bool)
    out = {}
    for b, (off, row, w, h) in places.items():
        rows = np.lib.stride_tricks.as_strided(dst[off:], (h, w * bpp), (row, 1))
        out[b] = np.ascontiguousarray(rows).reshape((h, w) + ((3,) if bpp == 3 else ()))
        for y in range(h):
            free[off + y * row: off + y * row + w * bpp] = False
    return out, free


def reduced(size, N):
    return (-(-size[0] // N), -(-size[1] // N))


@pytest.mark.parametrize("fmt", ["u8x3", "u8"])
@pytest.mark.parametrize("N", [2, 4, 8])
def test_every_fixture(L, ctx, old, kat, N, fmt):
    """all files of both sets in one call, each at a place of its own"""
    names = [(k, str(n)) for k in (old, kat) for n in k["names"]]
    streams = [k["stream_" + n].tobytes() for k, n in names]
    sizes = [reduced(k["pil_" + n].shape[1::-1], N) for k, n in names]
    assert len(names) == 35
    word, bpp = (L.PIX_U8X3, 3) if fmt == "u8x3" else (L.PIX_U8, 1)
    info, dst, places = batch_call(L, ctx, streams, word, sizes, list(range(len(names)))[::-1], N)
    assert info[:, 5].tolist() == [0] * len(names)
    got, free = pictures_and_guards(dst, places, bpp)
    assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
    for b, (_, n) in enumerate(names):
        assert info[b, :6].tolist() == Z.probe_row(streams[b], N)[:6] and info[b, 7] == 0, n
        same(got[b], wanted(streams[b], N, fmt), "%s 1/%d %s" % (fmt, N, n))


ORDER = [4, 9, 0, 7, 2, 10, 5, 1, 8, 3, 6]


def mixed(old, kat):
    """(streams, scales, allocated sizes, expected statuses)"""
    pick = [(old, "c420_203x117_rows", 1), (kat, "s41_67x35_r3", 2), (old, "c422_203x117_opt", 4), (kat, "t440_35x67", 8), (old, "g_17x33_r3", 1),
            (old, "c444_203x117_r1", 2), (kat, "s22_11_21_67x35", 4), (old, "c420_9x7", 8)]
    streams = [k["stream_" + n].tobytes() for k, n, _ in pick]
    scales = [N for _, _, N in pick]
    sizes = [reduced(k["pil_" + n].shape[1::-1], N) for k, n, N in pick]
    status = [0] * len(pick)
    streams.append(old["stream_progressive"].tobytes())  # 40 x 24
    scales.append(2)
    sizes.append((20, 12))
    status.append(2)
    whole = kat["stream_s12_67x35"].tobytes()
    scan = S.probe(whole).scan
    streams.append(whole[:scan + (len(whole) - scan) // 2])  # cut in the middle of its scan
    scales.append(2)
    sizes.append((34, 18))
    status.append(4)
    streams.append(old["stream_c420_17x33_r1_opt"].tobytes())  # allocated at the full size, while [6] says 1/2
    scales.append(2)
    sizes.append((17, 33))
    status.append(3)
    return streams, scales, sizes, status


@pytest.mark.parametrize("fmt", ["u8x3", "u8"])
def test_mixed_batch(L, ctx, old, kat, fmt):
    streams, scales, sizes, status = mixed(old, kat)
    assert sorted(ORDER) == list(range(len(streams)))
    word, bpp = (L.PIX_U8X3, 3) if fmt == "u8x3" else (L.PIX_U8, 1)
    info, dst, places = batch_call(L, ctx, streams, word, sizes, ORDER, scales)
    assert info[:, 5].tolist() == status
    assert info[10, :2].tolist() == [9, 17], "status 3 is held against the reduced size, which info tells"
    got, free = pictures_and_guards(dst, places, bpp)
    assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
    for b, st in enumerate(status):
        if st == 0:
            assert info[b, :6].tolist() == Z.probe_row(streams[b], scales[b])[:6]
            same(got[b], wanted(streams[b], scales[b], fmt), "%s frame %d at 1/%d" % (fmt, b, scales[b]))
        elif st in (2, 3):
            assert (got[b] == GUARD).all(), "the skipped frame's extent is untouched"
    # the frames of scale 1 are what a call without the bit makes of them
    ones = [b for b, N in enumerate(scales) if N == 1 and status[b] == 0]
    assert len(ones) == 2
    plain, dst_plain, places_plain = batch_call(L, ctx, [streams[b] for b in ones], word, [sizes[b] for b in ones], [1, 0], None, bit=False)
    got_plain, free_plain = pictures_and_guards(dst_plain, places_plain, bpp)
    assert (dst_plain[free_plain] == GUARD).all()
    for i, b in enumerate(ones):
        assert plain[i].tolist() == info[b].tolist()
        same(got[b], got_plain[i], "frame %d with the bit and without" % b)
        status_1, full = S.decode(streams[b], fmt)
        same(got[b], full, "frame %d against the unscaled restatement" % b)


def test_scale_1_throughout_is_the_call_without_the_bit(L, ctx, old):
    """a call with the bit whose frames are all of scale 1 launches the kernels it launches without it"""
    names = [str(n) for n in old["names"]]
    streams = [old["stream_" + n].tobytes() for n in names]
    sizes = [old["pil_" + n].shape[1::-1] for n in names]
    order = list(range(len(names)))
    a, dst_a, _ = batch_call(L, ctx, streams, L.PIX_U8X3, sizes, order, 1)
    b, dst_b, _ = batch_call(L, ctx, streams, L.PIX_U8X3, sizes, order, None, bit=False)
    assert a[:, 5].tolist() == [0] * len(names) and np.array_equal(a, b) and np.array_equal(dst_a, dst_b)


@pytest.mark.parametrize("o,N", [(3, 2), (6, 2), (8, 4)])
@pytest.mark.parametrize("name", ["c420_203x117", "s12_67x35"])
def test_orientation(L, ctx, old, kat, name, o, N):
    """2..4 keep the thread-per-pixel shape of the output pass, 5..8 take the transposing squares; the reduced picture is
    turned as a full one is"""
    k = old if name.startswith("c") else kat
    plain = k["stream_" + name].tobytes()
    stream = X.with_exif(plain, o)
    rw, rh = reduced(k["pil_" + name].shape[1::-1], N)
    size = (rw, rh) if o < 5 else (rh, rw)
    for fmt, word, bpp in (("u8x3", L.PIX_U8X3, 3), ("u8", L.PIX_U8, 1)):
        info, dst, places = batch_call(L, ctx, [stream], word, [size], [0], N, orient=True)
        assert info[0, 5] == 0 and info[0, 7] == o and info[0].tolist()[:6] == Z.probe_row(stream, N, orient=True)[:6]
        assert info[0, :2].tolist() == list(size)
        got, free = pictures_and_guards(dst, places, bpp)
        assert (dst[free] == GUARD).all()
        same(got[0], wanted(stream, N, fmt, orient=True), "%s orientation %d at 1/%d" % (fmt, o, N))
        same(wanted(stream, N, fmt, orient=True), X.orient(wanted(plain, N, fmt), o), "the restatement's own orientation")


def test_large_streams(L, ctx, kat, doc):
    """streams of several workgroups of the entropy stage, and pictures of many output tiles"""
    big = kat["stream_big440"].tobytes()
    assert len(big) > 2 * 256 * 128
    for stream, size, scales in ((big, (320, 240), (2,)), (doc, (1000, 563), (4, 8))):
        for N in scales:
            info, dst, places = batch_call(L, ctx, [stream], L.PIX_U8X3, [reduced(size, N)], [0], N)
            assert info[0, 5] == 0 and info[0, :2].tolist() == list(reduced(size, N))
            got, free = pictures_and_guards(dst, places, 3)
            assert (dst[free] == GUARD).all()
            same(got[0], wanted(stream, N, "u8x3"), "%d x %d at 1/%d" % (size + (N,)))
    luma = ctx.decode_jpeg(doc, L.PIX_U8, scale=8)
    same(luma, wanted(doc, 8, "u8"), "decode_jpeg(scale=8), luminance")


def test_the_bit_on_other_calls_fails_cleanly(L, ctx):
    """with a context: the encoder and the warps refuse the decoder's bit as they refuse every unknown one"""
    frame = np.zeros((16, 16, 3), np.uint8)
    d = ctx.device_upload(frame)
    try:
        for word, what in ((L.PIX_U8X3 | L.JPEG_SCALED, "unknown option"), (L.PIX_U8X3 | L.WARP_JPEG | L.JPEG_SCALED, "another option bit"),
                           (L.PIX_U8X3 | L.WARP_RAGGED | L.JPEG_SCALED, "unknown option")):
            rc = L.lib().lr_warp_perspective_device(ctx._h, C.c_void_p(d), frame.nbytes, 1, 0, 0, 0, word, None, C.c_void_p(d), frame.nbytes, 0, 0, 0)
            assert rc != 0 and what in L.lib().lr_last_error().decode(), hex(word)
    finally:
        ctx.device_free(d)


def detector_frame(w, h, seed):
    from librectify_amd import synth

    g = np.clip(synth.frame(w, h, seed, bars=40) * 255.0, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))


_files = []


def detector_files(ctx):
    """a 4:4:0 file (from the fixtures' writer) and a 4:2:0 file (the library's encoder) of a picture with lines in it, twice
    the size the detector is to see; written once"""
    if not _files:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import make_jpeg_sampling_fixtures as F

        frame = detector_frame(640, 480, 5)
        _files.extend([F.encode(frame, F.SAMPLINGS["s12"], 92), ctx.encode_jpeg(frame, 92, 0)])
    return _files


@pytest.mark.parametrize("jpeg", [None, 95])
def test_rectify_batch_on_files_at_half_size(L, ctx, jpeg):
    files = detector_files(ctx)
    assert L.jpeg_info(files, any_sampling=True, scale=2)[:, :4].tolist() == [[320, 240, 3, 0x12], [320, 240, 3, 0]]
    arrays = [wanted(f, 2, "u8x3") for f in files]
    decoded = ctx.decode_jpeg_batch(files, any_sampling=True, scale=2)
    for b in range(2):
        same(decoded[b], arrays[b], "decode_jpeg_batch, file %d" % b)
    got = ctx.rectify_batch(files, any_sampling=True, decode_scale=2, jpeg=jpeg)
    ref = [ctx.rectify(np.array(a), jpeg=jpeg) for a in arrays]
    assert len(got[0][0]) > 10 and got[0][2] is not None
    for b, (g, r) in enumerate(zip(got, ref)):
        assert g[0].tobytes() == r[0].tobytes() and bytes(g[1]) == bytes(r[1]), "frame %d" % b
        assert (bytes(g[2]) == bytes(r[2])) if jpeg else np.array_equal(g[2], r[2]), "frame %d" % b
    one = ctx.rectify(files[0], any_sampling=True, decode_scale=2, jpeg=jpeg)
    assert one[0].tobytes() == ref[0][0].tobytes() and bytes(one[1]) == bytes(ref[0][1])
    # decode_max_size picks the same scale: 640 -> 320 >= 300, and 160 is not
    by_size = ctx.rectify_batch(files, any_sampling=True, decode_max_size=300, jpeg=jpeg)
    for g, m in zip(got, by_size):
        assert g[0].tobytes() == m[0].tobytes() and bytes(g[1]) == bytes(m[1])
        assert (bytes(g[2]) == bytes(m[2])) if jpeg else np.array_equal(g[2], m[2])
    if jpeg is None:
        lines = [g[0] for g in got]
        drawn = ctx.draw_lines_batch(files, lines, any_sampling=True, decode_scale=[2, 2])
        want = ctx.draw_lines_batch([np.array(a) for a in arrays], lines)
        for d, w in zip(drawn, want):
            assert np.array_equal(d, w)


def test_recipe_scale(L, ctx, doc, tmp_path):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    path, prefix = os.path.join(G, "doc_image.jpg"), str(tmp_path / "out")
    r = subprocess.run([exe, path, prefix, "--jpeg-in", "--scale", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines, _, _ = ctx.rectify(doc, max_size=1200, decode_scale=2)
    rows = ["%g,%g,%g,%g,%g,%g,%d" % (l["x1"], l["y1"], l["x2"], l["y2"], l["weight"], l["err"], l["group_id"]) for l in lines]
    with open(prefix + "_lines.csv") as f:
        assert f.read().splitlines() == rows and len(rows) > 10
    assert max(float(l["x1"]) for l in lines) < 500, "the segments are in the decoded picture's coordinates"
    r = subprocess.run([exe, path, prefix, "--scale", "2"], capture_output=True, text=True)
    assert r.returncode != 0 and "--scale" in r.stderr
    r = subprocess.run([exe, path, prefix, "--jpeg-in", "--scale", "3"], capture_output=True, text=True)
    assert r.returncode != 0 and "--scale" in r.stderr
