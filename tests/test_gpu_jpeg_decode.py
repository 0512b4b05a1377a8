"""Baseline JPEG files decoded on the GPU: lr_decode_jpeg_device (kernels_jpeg_decode.hip) against
tests/numpy_jpeg_decode_ref.py, byte for byte: the shapes at which the entropy decoder and the transform take another path
(less than a block, partial MCUs, a scan of one 128-byte part, scans of many parts and of several workgroups with and
without restart markers), the four samplings into both output formats, foreign files (optimised code tables, no DRI, a DRI
of one MCU), the contents that reach the longest codes and stuffed bytes across a part's boundary, a batch at unordered
places with guard bytes and a refused file among it, damaged scans (a cut-off download; the restatement runs on the same
bytes first), the pipeline (rectify_batch, rectify and draw_lines_batch on files), trim and the recipe's --jpeg-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_jpeg_decode_ref as D
import numpy_jpeg_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = os.path.join(ROOT, "tests", "golden")
GUARD = 0xAB
PART = 128  # bytes of a scan that one lane decodes (kernels_jpeg_decode.hip: kPartBytes)
KINDS = ["u8", "420", "444"]  # what the encoder's restatement writes; 4:2:2 comes from the fixture file
SHAPES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (203, 117), (300, 150), (640, 360)]
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


_wanted = {}


def want(stream, fmt):
    """the restatement's decode, computed once per (stream, format)"""
    key = (stream, fmt)
    if key not in _wanted:
        status, img = D.decode(stream, fmt)
        assert status == 0
        _wanted[key] = img
    return _wanted[key]


def textured(w, h, seed, kind):
    """a ramp under noise of +-20: every coefficient class occurs"""
    rng = np.random.default_rng(seed)
    shape = (h, w) if kind == "u8" else (h, w, 3)
    y, x = np.mgrid[0:h, 0:w]
    ramp = (3 * x + 2 * y) % 256
    if kind != "u8":
        ramp = np.stack([ramp, (ramp + 85) % 256, (2 * ramp) % 256], axis=-1)
    return np.clip(ramp + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)


def as_kind(gray, kind):
    return gray if kind == "u8" else np.ascontiguousarray(np.stack([gray, gray, gray], axis=-1))


_streams = {}


def shape_stream(kind, shape):
    if (kind, shape) not in _streams:
        w, h = shape
        _streams[(kind, shape)] = R.encode(textured(w, h, 7 + w, kind), 85, 1 if kind == "444" else 0)
    return _streams[(kind, shape)]


def parts(stream):
    return max(1, -(-(len(stream) - D.probe(stream).scan) // PART))


def decode(L, ctx, stream, fmt):
    """the raw call for one stream: (info row, picture)"""
    info = D.probe(stream)
    bpp = 3 if fmt == "u8x3" else 1
    region = np.frombuffer(stream, np.uint8)
    table = L.jpeg_decode_table([(0, len(stream))], [(0, info.width * bpp)], [(info.width, info.height)])
    total = info.width * info.height * bpp
    d_src, d_dst = ctx.device_upload(region), ctx.device_upload(np.full(total, GUARD, np.uint8))
    try:
        rows = ctx.decode_jpeg_device(d_src, region, L.PIX_U8X3 if bpp == 3 else L.PIX_U8, table, d_dst, total)
        out = ctx.device_download(d_dst, (total,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    return rows[0], out.reshape((info.height, info.width) + ((3,) if bpp == 3 else ()))


def check(L, ctx, stream, formats=FORMATS):
    row = None
    for fmt in formats:
        row, got = decode(L, ctx, stream, fmt)
        assert row[5] == 0 and row[:5].tolist() == D.probe(stream).row()[:5] and row[7] == 0
        w = want(stream, fmt)
        if not np.array_equal(got, w):
            bad = np.argwhere(got != w)
            raise AssertionError("%s: %d values differ, the first at %s" % (fmt, len(bad), bad[0].tolist()))
    return row


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_shapes(L, ctx, kind, shape):
    check(L, ctx, shape_stream(kind, shape))


def test_fixture_files(L, ctx, kat):
    layouts = set()
    for name in kat["names"]:
        stream = kat["stream_" + str(name)].tobytes()
        row = check(L, ctx, stream)
        layouts.add((int(row[2]), int(row[3])))
    assert layouts == {(1, 0), (3, 0), (3, 1), (3, 2)}, "one component, 4:2:0, 4:4:4, 4:2:2"


def test_the_cases_cover_one_part_many_parts_and_more_than_one_decode(L, ctx, kat):
    assert parts(shape_stream("u8", (1, 1))) == 1
    long_one = kat["stream_c420_203x117"].tobytes()
    assert D.probe(long_one).restart == 0 and parts(long_one) >= 64 and not any(
        long_one[i] == 0xFF and 0xD0 <= long_one[i + 1] <= 0xD7 for i in range(D.probe(long_one).scan, len(long_one) - 1))
    assert parts(shape_stream("444", (640, 360))) > 256, "more than one workgroup of parts"
    assert R.intervals(640, 360, 1, 3) > 8 and (80 * 45) % 32, "our DRI: the marker numbers wrap, a partial last interval"
    row, _ = decode(L, ctx, shape_stream("u8", (1, 1)), "u8")
    assert row[6] == 1, "one part is decoded once"
    row, _ = decode(L, ctx, long_one, "u8x3")
    assert row[5] == 0 and row[6] >= 2, "parts that start on a guess are decoded again from their true state"


@pytest.mark.parametrize("kind", KINDS)
def test_constant_frames(L, ctx, kind):
    for value in (0, 128, 255):
        check(L, ctx, R.encode(as_kind(np.full((24, 40), value, np.uint8), kind), 75, 1 if kind == "444" else 0))


@pytest.mark.parametrize("kind", KINDS)
def test_noise_at_quality_100_with_stuffed_bytes_across_a_boundary(L, ctx, kind):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (150, 300) if kind == "u8" else (150, 300, 3), dtype=np.uint8)
    stream = R.encode(img, 100, 1 if kind == "444" else 0)
    scan = D.probe(stream).scan
    stuffed = [i for i in range(scan, len(stream) - 1) if stream[i] == 0xFF and stream[i + 1] == 0]
    assert stuffed, "the case has stuffed bytes"
    assert any((i - scan) % PART == PART - 1 for i in stuffed), "one of them with its zero in the next part"
    check(L, ctx, stream)


@pytest.mark.parametrize("kind", KINDS)
def test_alternating_blocks_reach_category_11(L, ctx, kind):
    by, bx = np.mgrid[0:8, 0:8]
    gray = np.kron(((by + bx) & 1) * 255, np.ones((8, 8), np.int64)).astype(np.uint8)
    img = as_kind(gray, kind)
    coefs, _ = R.coefficients(img, 100, 1 if kind == "444" else 0)
    dc = coefs[:, 0, 0] if kind != "420" else coefs[:, :4, 0].reshape(-1)
    assert np.abs(np.diff(dc)).max() >= 1024, "a DC difference of category 11"
    check(L, ctx, R.encode(img, 100, 1 if kind == "444" else 0))


@pytest.mark.parametrize("kind", KINDS)
def test_one_late_coefficient_gives_zrl_and_no_eob(L, ctx, kind):
    i = np.arange(8)
    wave = np.cos((2 * i + 1) * 7 * np.pi / 16)
    gray = np.tile(np.round(128 + 100 * np.outer(wave, wave)), (3, 5)).astype(np.uint8)
    img = as_kind(gray, kind)
    layout = 1 if kind == "444" else 0
    blocks = R.coefficients(img, 95, layout)[0].reshape(-1, 64)
    assert len(blocks[(blocks[:, 63] != 0) & ~blocks[:, 1:63].any(axis=1)]), "a block whose only AC coefficient is index 63"
    check(L, ctx, R.encode(img, 95, layout))
    check(L, ctx, R.encode(img, 100, layout))


def test_doc_image(L, ctx, doc):
    row = check(L, ctx, doc)
    assert row[:6].tolist() == [1000, 563, 3, 0, 0, 0]
    assert parts(doc) > 1024 and row[6] >= 2


# ---- the raw call: a batch at places of its own, guard bytes, a refused file, damaged scans ----

def batch_call(L, ctx, streams, fmt, order=None, pad=7, gap=13):
    """The streams one behind the other (odd gaps), the pictures in `order` with rows padded by `pad` bytes and `gap`
    guard bytes between them.  Returns (info, the destination region, per stream its (offset, row bytes, w, h))."""
    bpp = 3 if fmt == L.PIX_U8X3 else 1
    infos = [D.probe(s) for s in streams]
    offs, end = [], 3
    for s in streams:
        offs.append(end)
        end += len(s) + 5
    region = np.full(end, 0x11, np.uint8)
    for s, o in zip(streams, offs):
        region[o:o + len(s)] = np.frombuffer(s, np.uint8)
    places, at = {}, gap
    for b in (order or range(len(streams))):
        w, h = max(infos[b].width, 1), max(infos[b].height, 1)
        places[b] = (at, w * bpp + pad, w, h)
        at += h * (w * bpp + pad) + gap
    table = L.jpeg_decode_table([(o, len(s)) for s, o in zip(streams, offs)], [places[b][:2] for b in range(len(streams))],
                                [places[b][2:] for b in range(len(streams))])
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


def test_batch_of_eight_with_a_refused_file_among_them(L, ctx, kat):
    names = ["c420_203x117_opt", "g_17x33_r3", "c422_203x117_opt", "progressive", "c444_17x33", "c420_17x33_r1_opt", "c422_9x7", "g_203x117_opt"]
    streams = [kat["stream_" + n].tobytes() for n in names]
    for fmt, name, bpp in ((L.PIX_U8X3, "u8x3", 3), (L.PIX_U8, "u8", 1)):
        info, dst, places = batch_call(L, ctx, streams, fmt, order=[5, 2, 7, 0, 3, 6, 1, 4])
        assert info[:, 5].tolist() == [0, 0, 0, 2, 0, 0, 0, 0]
        got, free = pictures_and_guards(dst, places, bpp)
        assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
        assert (got[3] == GUARD).all(), "the refused file's extent is untouched"
        for b, s in enumerate(streams):
            if b != 3:
                assert np.array_equal(got[b], want(s, name)), names[b]


def test_damaged_scans_get_status_4_and_write_nothing_outside(L, ctx, doc, kat):
    rng = np.random.default_rng(3)
    scan = D.probe(doc).scan
    half = scan + (len(doc) - scan) // 2
    damaged = [doc[:100000], doc[:half] + rng.integers(0, 256, len(doc) - half, dtype=np.uint8).tobytes()]
    good = kat["stream_c444_17x33"].tobytes()
    for bad in damaged:
        assert D.decode(bad)[0] == D.DAMAGED, "the restatement, on the same bytes, first"
        info, dst, places = batch_call(L, ctx, [good, bad], L.PIX_U8X3, order=[1, 0])
        assert info[:, 5].tolist() == [0, 4] and info[1, :3].tolist() == [1000, 563, 3]
        got, free = pictures_and_guards(dst, places, 3)
        assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
        assert np.array_equal(got[0], want(good, "u8x3")), "the sound stream of the same call"
        check(L, ctx, good)  # the next call on the context


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


def test_rectify_batch_on_files(L, ctx):
    frames = [detector_frame(w, h, 3 + b) for b, (w, h) in enumerate([(160, 120), (120, 160), (200, 150)])]
    streams = ctx.encode_jpeg_batch(frames, 92, 0)
    arrays = ctx.decode_jpeg_batch(streams)
    for s, a in zip(streams, arrays):
        assert np.array_equal(a, want(s, "u8x3"))
    got = ctx.rectify_batch(streams, max_size=1200, jpeg=90)
    assert sum(g[2] is not None for g in got) >= 2, "the case has pictures"
    same_results(got, ctx.rectify_batch(arrays, max_size=1200, jpeg=90))
    same_results(ctx.rectify_batch(streams), ctx.rectify_batch(arrays))
    with pytest.raises(ValueError):
        ctx.rectify_batch([streams[0], arrays[1]])
    with pytest.raises(ValueError):
        ctx.draw_lines_batch([arrays[0], streams[1]], [got[0][0], got[1][0]])
    lines = [g[0] for g in got]
    assert ctx.draw_lines_batch(streams, lines, jpeg=85) == ctx.draw_lines_batch(arrays, lines, jpeg=85)
    # a list of one-component files is decoded to u8: the call on decode_jpeg_batch(files, PIX_U8)'s arrays
    gray = ctx.encode_jpeg_batch([np.ascontiguousarray(f[..., 0]) for f in frames], 92, 0)
    gray_arrays = ctx.decode_jpeg_batch(gray, L.PIX_U8)
    assert all(a.ndim == 2 for a in gray_arrays)
    same_results(ctx.rectify_batch(gray, max_size=1200, jpeg=90), ctx.rectify_batch(gray_arrays, max_size=1200, jpeg=90))
    same_results(ctx.rectify_batch(gray), ctx.rectify_batch(gray_arrays))
    assert ctx.draw_lines_batch(gray, lines, jpeg=85) == ctx.draw_lines_batch(gray_arrays, lines, jpeg=85)
    # a refused file is named
    with pytest.raises(L.LibrectifyError, match="frame 1"):
        ctx.decode_jpeg_batch([streams[0], b"\xFF\xD8\xFF"])


def test_rectify_on_the_doc_file(L, ctx, doc):
    array = ctx.decode_jpeg(doc)
    for kw in (dict(), dict(max_size=1200, jpeg=90)):
        got, ref = ctx.rectify(doc, **kw), ctx.rectify(array, **kw)
        same_results([got], [ref])
    assert len(ctx.rectify(doc)[0]) > 10


def test_trim_and_the_next_call(L, ctx, kat):
    stream = kat["stream_c422_203x117_opt"].tobytes()
    check(L, ctx, stream, ["u8x3"])
    ctx.trim()
    check(L, ctx, stream, ["u8x3"])
    got = ctx.decode_jpeg_batch([stream, kat["stream_g_9x7"].tobytes()], L.PIX_U8)
    assert np.array_equal(got[0], want(stream, "u8")) and got[1].shape == (7, 9)


def test_recipe_jpeg_in_writes_what_python_computes(L, ctx, doc, tmp_path):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    prefix = str(tmp_path / "doc")
    r = subprocess.run([exe, os.path.join(G, "doc_image.jpg"), prefix, "--jpeg-in"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines, t, _ = ctx.rectify(doc, max_size=1200)
    rows = ["%g,%g,%g,%g,%g,%g,%d" % (l["x1"], l["y1"], l["x2"], l["y2"], l["weight"], l["err"], l["group_id"]) for l in lines]
    with open(prefix + "_lines.csv") as f:
        assert f.read().splitlines() == rows and len(rows) > 10
    with open(prefix + "_tform.csv") as f:
        got = f.read().splitlines()
    pts = [t.top_left, t.top_right, t.bottom_left, t.bottom_right]
    assert got[:4] == ["%g,%g" % (p.x, p.y) for p in pts]
    assert got[4:] == ["%g,%g,%g" % (p.x, p.y, p.z) for p in (t.horizontal_vp, t.vertical_vp)]
