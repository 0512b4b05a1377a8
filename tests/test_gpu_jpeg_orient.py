"""EXIF orientation in the GPU JPEG decoder: entry [7] of lr_decode_jpeg_device's table (kernels_jpeg_decode.hip, the
output pass) against tests/numpy_jpeg_orient_ref.py, byte for byte.  The eight orientations over the four samplings into
both output formats at sizes that are multiples neither of the 32 x 8 tile, nor of the 32 x 32 square of the transposing
path, nor of an MCU; shapes of one pixel, one row, one column and more than one square each way; a mixed batch at places
of its own with guard bytes, a frame that keeps [7] = 0, one without Exif, one given the stored size, a refused file; the
pipeline (rectify, rectify_batch, draw_lines_batch on files) and the recipe's --orient."""
import os
import subprocess

import numpy as np
import pytest

import numpy_jpeg_decode_ref as D
import numpy_jpeg_orient_ref as X
import numpy_jpeg_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = os.path.join(ROOT, "tests", "golden")
GUARD = 0xAB
KINDS = ["u8", "444", "422", "420"]
FORMATS = ["u8", "u8x3"]


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
    return np.load(os.path.join(G, "jpeg_decode_kat.npz"))


@pytest.fixture(scope="module")
def doc():
    with open(os.path.join(G, "doc_image.jpg"), "rb") as f:
        return f.read()


def textured(w, h, seed, kind):
    """a ramp that differs along x and y under noise of +-20: no two orientations of it are alike"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    ramp = (3 * x + 2 * y) % 256
    if kind == "u8":
        return np.clip(ramp + rng.integers(-20, 21, (h, w)), 0, 255).astype(np.uint8)
    ramp = np.stack([ramp, (ramp + 85) % 256, (2 * ramp) % 256], axis=-1)
    return np.clip(ramp + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


_plain, _stored = {}, {}


def plain_stream(kind, shape):
    """the stream without Exif, encoded once per (kind, shape)"""
    if (kind, shape) not in _plain:
        img = textured(shape[0], shape[1], 7 + shape[0], kind)
        _plain[(kind, shape)] = X.encode_422(img, 85) if kind == "422" else R.encode(img, 85, 1 if kind == "444" else 0)
    return _plain[(kind, shape)]


def stored(kind, shape, fmt):
    """the restatement's decode of the stored picture, computed once per (kind, shape, format): the eight orientations
    are permutations of it"""
    key = (kind, shape, fmt)
    if key not in _stored:
        status, img = D.decode(plain_stream(kind, shape), fmt)
        assert status == 0
        _stored[key] = img
    return _stored[key]


def decode(L, ctx, stream, fmt, orient=True):
    """the raw call for one stream, probe first as a caller does: (info row, picture)"""
    bpp = 3 if fmt == "u8x3" else 1
    w, h = (int(v) for v in L.jpeg_info([stream], orient=orient)[0, :2])
    region = np.frombuffer(stream, np.uint8)
    table = L.jpeg_decode_table([(0, len(stream))], [(0, w * bpp)], [(w, h)], orient=orient)
    total = w * h * bpp
    d_src, d_dst = ctx.device_upload(region), ctx.device_upload(np.full(total, GUARD, np.uint8))
    try:
        rows = ctx.decode_jpeg_device(d_src, region, L.PIX_U8X3 if bpp == 3 else L.PIX_U8, table, d_dst, total)
        out = ctx.device_download(d_dst, (total,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    return rows[0], out.reshape((h, w) + ((3,) if bpp == 3 else ()))


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d values differ, the first at %s" % (what, len(bad), bad[0].tolist()))


@pytest.mark.parametrize("shape", [(47, 70), (33, 9)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("o", range(1, 9))
def test_orientations(L, ctx, o, kind, shape):
    stream = X.with_exif(plain_stream(kind, shape), o, "II" if o & 1 else "MM")
    assert X.exif_orientation(stream) == o and D.probe(stream).layout == {"u8": 0, "444": 1, "422": 2, "420": 0}[kind]
    for fmt in FORMATS:
        row, got = decode(L, ctx, stream, fmt)
        want_row = X.info_row(stream, True)
        assert row[5] == 0 and row[:5].tolist() == want_row[:5] and row[7] == o
        same(got, X.orient(stored(kind, shape, fmt), o), "%s orientation %d" % (fmt, o))
    # and with [7] = 0 the file is the stored picture, its last column 0
    row, got = decode(L, ctx, stream, "u8x3", orient=False)
    assert row[7] == 0 and row[:2].tolist() == list(shape)
    same(got, stored(kind, shape, "u8x3"), "as stored")


@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (40, 1), (130, 35)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("o", [3, 6, 7])
def test_degenerate_shapes(L, ctx, o, shape):
    stream = X.with_exif(plain_stream("420", shape), o)
    row, got = decode(L, ctx, stream, "u8x3")
    assert row[5] == 0 and row[7] == o and row[:2].tolist() == list(shape if o < 5 else shape[::-1])
    same(got, X.orient(stored("420", shape, "u8x3"), o), "orientation %d" % o)


# ---- the raw call: a mixed batch at places of its own, guard bytes ----

def batch_call(L, ctx, streams, flags, fmt, sizes, order, pad=7, gap=13):
    """The streams one behind the other (odd gaps), the pictures in `order`, each allocated for sizes[b], with rows padded
    by `pad` bytes and `gap` guard bytes between them.  Returns (info, the destination region, per stream its (offset,
    row bytes, w, h))."""
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
                                [places[b][2:] for b in range(len(streams))], orient=flags)
    d_src, d_dst = ctx.device_upload(region), ctx.device_upload(np.full(at, GUARD, np.uint8))
    try:
        info = ctx.decode_jpeg_device(d_src, region, fmt, table, d_dst, at)
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


def test_mixed_batch_of_eight(L, ctx, kat):
    # (kind, shape, orientation in the file or None, [7])
    frames = [("420", (47, 70), 6, True), ("u8", (33, 9), 3, True), ("422", (47, 70), 8, False), ("444", (33, 9), None, True),
              ("422", (130, 35), 5, True), ("420", (33, 9), 6, True), (None, None, None, True), ("444", (47, 70), 2, True)]
    REFUSED, PROGRESSIVE = 5, 6  # frame 5 is given its stored size
    streams, flags, sizes, wants = [], [], [], {}
    for b, (kind, shape, o, flag) in enumerate(frames):
        if b == PROGRESSIVE:
            streams.append(X.with_exif(kat["stream_progressive"].tobytes(), 6))
            sizes.append((24, 40))  # (its upright size: accepted by the table, the file refused)
        else:
            plain = plain_stream(kind, shape)
            streams.append(plain if o is None else X.with_exif(plain, o))
            applied = o if (flag and o) else 1
            sizes.append(shape if b == REFUSED or applied < 5 else shape[::-1])
        flags.append(flag)
    for fmt, name, bpp in ((L.PIX_U8X3, "u8x3", 3), (L.PIX_U8, "u8", 1)):
        info, dst, places = batch_call(L, ctx, streams, flags, fmt, sizes, order=[5, 2, 7, 0, 3, 6, 1, 4])
        assert info[:, 5].tolist() == [0, 0, 0, 0, 0, 3, 2, 0]
        assert info[:, 7].tolist() == [6, 3, 0, 1, 5, 6, 6, 2]
        assert info[REFUSED, :2].tolist() == [9, 33] and info[2, :2].tolist() == [47, 70] and info[4, :2].tolist() == [35, 130]
        got, free = pictures_and_guards(dst, places, bpp)
        assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
        assert (got[REFUSED] == GUARD).all() and (got[PROGRESSIVE] == GUARD).all(), "the extents of the skipped frames are untouched"
        for b, (kind, shape, o, flag) in enumerate(frames):
            if b not in (REFUSED, PROGRESSIVE):
                same(got[b], X.orient(stored(kind, shape, name), o if (flag and o) else 1), "%s frame %d" % (name, b))


# ---- the pipeline ----

def detector_frame(w, h, seed):
    from librectify_amd import synth

    g = np.clip(synth.frame(w, h, seed, bars=40) * 255.0, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))


def same_results(got, ref):
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        assert g[0].tobytes() == r[0].tobytes() and bytes(g[1]) == bytes(r[1]), "frame %d: lines and transform" % b
        if isinstance(r[2], np.ndarray):
            assert np.array_equal(g[2], r[2]), "frame %d: the picture" % b
        else:
            assert g[2] == r[2], "frame %d: the stream" % b


def test_rectify_on_sideways_files(L, ctx):
    plain = ctx.encode_jpeg(detector_frame(320, 240, 5), 92, 0)
    files = {6: X.with_exif(plain, 6), 8: X.with_exif(plain, 8, "II")}
    as_stored = ctx.decode_jpeg(plain)
    uprights = {6: np.ascontiguousarray(np.rot90(as_stored, -1)), 8: np.ascontiguousarray(np.rot90(as_stored, 1))}
    for o, data in files.items():
        assert np.array_equal(ctx.decode_jpeg(data), as_stored), "without orient the file is the stored picture"
        assert np.array_equal(ctx.decode_jpeg(data, orient=True), uprights[o])
        assert np.array_equal(ctx.decode_jpeg(data, L.PIX_U8, orient=True), np.rot90(ctx.decode_jpeg(plain, L.PIX_U8), -1 if o == 6 else 1))
        got, ref = ctx.rectify(data, orient=True), ctx.rectify(uprights[o])
        assert len(got[0]) > 10 and got[2] is not None and got[2].shape[2] == 3
        same_results([got], [ref])
    order = [files[6], files[8], plain]
    arrays = [uprights[6], uprights[8], as_stored]
    assert [a.shape for a in ctx.decode_jpeg_batch(order, orient=True)] == [a.shape for a in arrays]
    got = ctx.rectify_batch(order, orient=True, jpeg=95)
    same_results(got, [ctx.rectify(a, jpeg=95) for a in arrays])
    same_results(got, ctx.rectify_batch(arrays, jpeg=95))
    lines = [g[0] for g in got]
    assert ctx.draw_lines_batch(order, lines, jpeg=85, orient=True) == ctx.draw_lines_batch(arrays, lines, jpeg=85)
    for call in (lambda: ctx.rectify(as_stored, orient=True), lambda: ctx.rectify_batch(arrays, orient=True),
                 lambda: ctx.rectify_batch(np.stack(arrays[:1]), orient=True), lambda: ctx.draw_lines_batch(arrays, lines, orient=True)):
        with pytest.raises(ValueError, match="orient"):
            call()


def test_recipe_orient_writes_what_python_computes(L, ctx, doc, tmp_path):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    sideways = X.with_exif(doc, 6)
    path = str(tmp_path / "sideways.jpg")
    with open(path, "wb") as f:
        f.write(sideways)
    prefix = str(tmp_path / "doc")
    r = subprocess.run([exe, path, prefix, "--jpeg-in", "--orient"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines, t, _ = ctx.rectify(sideways, max_size=1200, orient=True)
    rows = ["%g,%g,%g,%g,%g,%g,%d" % (l["x1"], l["y1"], l["x2"], l["y2"], l["weight"], l["err"], l["group_id"]) for l in lines]
    with open(prefix + "_lines.csv") as f:
        assert f.read().splitlines() == rows and len(rows) > 10
    with open(prefix + "_tform.csv") as f:
        got = f.read().splitlines()
    pts = [t.top_left, t.top_right, t.bottom_left, t.bottom_right]
    assert got[:4] == ["%g,%g" % (p.x, p.y) for p in pts]
    assert got[4:] == ["%g,%g,%g" % (p.x, p.y, p.z) for p in (t.horizontal_vp, t.vertical_vp)]
    # --orient goes with --jpeg-in alone
    r = subprocess.run([exe, path, prefix, "--orient"], capture_output=True, text=True)
    assert r.returncode != 0 and "--orient" in r.stderr
