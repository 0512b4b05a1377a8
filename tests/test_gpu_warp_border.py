"""LR_WARP_BORDER on the GPU against its NumPy second source (tests/numpy_warp_border_ref.py), byte for byte: three pixel
formats, both sampling rules, four border rules, the plain, the packed and the ragged launch, sources down to 1 x 1, maps that
fold a reflection thousands of times; the bit with every word 0 against the call without it; one ragged batch with a border
per frame; what is refused; and border= / crop= of the Python paths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_border_ref as RB
import numpy_warp_cubic_ref as RC
import numpy_warp_ref as R
from test_gpu_rectify_warp import BPP, DTYPE, assert_same, frame, read_pnm, synthetic_rgb
from test_gpu_warp_cubic import content, destination_table, six_frames

pytestmark = pytest.mark.gpu

CUBIC, BORDER, PACKED, RAGGED = 0x8000, 0x40000, 0x200, 0x800
SENTINEL = 0xAB
VALUE = {0: 200, 1: (7, 200, 31), 2: -1.5}  # the constant border's value per format
NAMES = ["constant", "replicate", "reflect", "reflect101"]


def borders(fmt):
    return [(RB.CONSTANT, VALUE[fmt]), (RB.REPLICATE, 0), (RB.REFLECT, 0), (RB.REFLECT_101, 0)]


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


# sources smaller than either support and one of several loads a row; outputs of three tile columns and rows with partial
# tiles, widths that are no multiple of a lane's four pixels
SOURCES = [(1, 1), (1, 7), (7, 1), (2, 3), (67, 35)]
OUTS = [(131, 37), (67, 33), (65, 17), (130, 35), (33, 37)]


def the_maps(w, h, ow, oh):
    """a shift by -10 pixels, a x 3 magnification, a strong perspective, a denominator that changes sign inside the output,
    and a map scaled by 1e5: its coordinates saturate and a reflection folds thousands of times"""
    return [
        np.array([[1.0, 0, -10], [0, 1, -10], [0, 0, 1]]),
        np.array([[1 / 3.0, 0, -2.4], [0, 1 / 3.0, -1.7], [0, 0, 1]]),
        np.array([[1.2, 0.3, -0.4 * w - 2], [-0.25, 1.0, 0.3 * h - 3], [0.9 / ow, 0.7 / oh, 1.0]]),
        np.array([[0.9, 0.1, -1.0], [0.05, 1.1, -2.0], [1.0 / ow, 1.7 / oh, -1.3]]),
        np.array([[1e5, 1e4, -3e5], [2e4, 1e5, -2e5], [0, 0, 1.0]]),
    ]


_SRC, _REF = {}, {}


def source(fmt, si):
    if (fmt, si) not in _SRC:
        _SRC[fmt, si] = frame(fmt, SOURCES[si][0], SOURCES[si][1], 300 + si)
    return _SRC[fmt, si]


def ref(fmt, si, mi, bi, cubic):
    """the second source's picture, computed once and shared by the three layouts"""
    key = (fmt, si, mi, bi, cubic)
    if key not in _REF:
        w, h = SOURCES[si]
        ow, oh = OUTS[mi]
        mode, value = borders(fmt)[bi]
        _REF[key] = RB.warp(source(fmt, si), the_maps(w, h, ow, oh)[mi], ow, oh, mode, value, cubic)
        _REF[key].setflags(write=False)
    return _REF[key]


def lay_sources(fmt, srcs, uniform):
    """the sources in one buffer at odd offsets with padded rows (f32: multiples of 4); uniform: one row and image stride"""
    bpp, step = BPP[fmt], 4 if fmt == 2 else 1
    places, cursor = [], 3 * step
    for k, s in enumerate(srcs):
        h, w = s.shape[:2]
        row = w * bpp + (1 if uniform else (1, 3, 0)[k % 3]) * step
        places.append((w, h, cursor, row))
        cursor += h * row + (5 if uniform else (5, 0, 2)[k % 3]) * step
    buf = np.full(cursor, 0x5A, np.uint8)
    for s, (w, h, off, row) in zip(srcs, places):
        np.lib.stride_tricks.as_strided(buf[off:], (h, w * bpp), (row, 1))[:] = np.ascontiguousarray(s).reshape(h, -1).view(np.uint8)
    return buf, places


def check_outputs(got, fmt, places, expected):
    """places: (ow, oh, offset, row stride) per frame; every frame is the expected one and nothing else was written"""
    bpp = BPP[fmt]
    written = np.zeros(got.shape, bool)
    for b, ((ow, oh, off, row), exp) in enumerate(zip(places, expected)):
        rows = np.lib.stride_tricks.as_strided(got[off:], (oh, ow * bpp), (row, 1))
        np.lib.stride_tricks.as_strided(written[off:], (oh, ow * bpp), (row, 1))[:] = True
        out = np.ascontiguousarray(rows).view(DTYPE[fmt]).reshape((oh, ow, 3) if fmt == 1 else (oh, ow))
        try:
            assert_same(out, exp)
        except AssertionError as e:
            raise AssertionError("frame %d: %s" % (b, e)) from None
    assert (got[~written] == SENTINEL).all(), "bytes outside the frames' pixels were written"


def launch(ctx, fmt, layout, opts, srcs, Ms, words, out_sizes):
    """One launch in the given layout (0 plain, PACKED, RAGGED) of the frames (source array, map, border word or None, output
    size); plain and packed take sources of one size, plain one output size.  Returns (destination bytes, places)."""
    bpp, step = BPP[fmt], 4 if fmt == 2 else 1
    n = len(srcs)
    sbuf, splaces = lay_sources(fmt, srcs, layout != RAGGED)
    w, h, soff, srow = splaces[0]
    simg = splaces[1][2] - soff if n > 1 else h * srow
    tail = [[float(x)] for x in words] if opts & BORDER else [[] for _ in words]
    if layout == 0:
        ow, oh = out_sizes[0]
        drow = ow * bpp + 3 * step
        dimg, doff = oh * drow + 5 * step, 2 * step
        places = [(ow, oh, doff + b * dimg, drow) for b in range(n)]
        region = doff + n * dimg
        table = np.array([list(np.asarray(M).reshape(9)) + t for M, t in zip(Ms, tail)])
    else:
        base, region = destination_table(out_sizes, bpp, 13) if n == 6 else packed_places(out_sizes, bpp)
        places = [tuple(int(v) for v in base[b, 9:13]) for b in range(n)]
        rows = []
        for b in range(n):
            r = list(np.asarray(Ms[b]).reshape(9)) + list(base[b, 9:13])
            if layout == RAGGED:
                r += list(splaces[b]) + ([float(words[b])] if opts & BORDER else [0.0])
            else:
                r += tail[b]
            rows.append(r)
        table = np.array(rows)
    d_src, d_dst = ctx.device_upload(sbuf), ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    try:
        if layout == 0:
            ctx.warp_perspective_device(d_src + soff, simg, n, w, h, srow, fmt | opts, table, d_dst + places[0][2], dimg, ow, oh, drow)
        elif layout == PACKED:
            ctx.warp_perspective_packed_device(d_src + soff, simg, n, w, h, srow, fmt | opts, table, d_dst, region)
        else:
            ctx.warp_perspective_ragged_device(d_src, len(sbuf), fmt | opts, table, d_dst, region)
        return ctx.device_download(d_dst, (region,), np.uint8), places
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def packed_places(out_sizes, bpp):
    """outputs one after the other with gaps and padded rows, in reverse order"""
    step = 4 if bpp == 4 else 1
    table = np.zeros((len(out_sizes), 13), np.float64)
    cursor = 4 * step
    for b in reversed(range(len(out_sizes))):
        ow, oh = out_sizes[b]
        row = ow * bpp + (3, 0, 5)[b % 3] * step
        table[b, 9:13] = (ow, oh, cursor, row)
        cursor += (oh - 1) * row + ow * bpp + (2, 7, 0)[b % 3] * step
    return table, cursor + 12


@pytest.mark.parametrize("layout", [0, PACKED, RAGGED], ids=["plain", "packed", "ragged"])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_byte_for_byte_against_the_second_source(ctx, fmt, layout):
    for cubic in (False, True):
        opts = BORDER | (CUBIC if cubic else 0)
        if layout == 0:  # a launch: one source, one map, the four borders as four frames
            for si, (w, h) in enumerate(SOURCES):
                for mi, (ow, oh) in enumerate(OUTS):
                    M = the_maps(w, h, ow, oh)[mi]
                    words = [RB.word(m, v, source(fmt, si)) for m, v in borders(fmt)]
                    got, places = launch(ctx, fmt, 0, opts, [source(fmt, si)] * 4, [M] * 4, words, [(ow, oh)] * 4)
                    check_outputs(got, fmt, places, [ref(fmt, si, mi, bi, cubic) for bi in range(4)])
        elif layout == PACKED:  # a launch: one source, the five maps; frame k's border is (k + r) % 4
            for si, (w, h) in enumerate(SOURCES):
                Ms = [the_maps(w, h, ow, oh)[mi] for mi, (ow, oh) in enumerate(OUTS)]
                for r in range(4):
                    bis = [(k + r) % 4 for k in range(5)]
                    words = [RB.word(*borders(fmt)[bi], source(fmt, si)) for bi in bis]
                    got, places = launch(ctx, fmt, PACKED, opts, [source(fmt, si)] * 5, Ms, words, OUTS)
                    check_outputs(got, fmt, places, [ref(fmt, si, mi, bis[mi], cubic) for mi in range(5)])
        else:  # a launch: the 25 frames of five sources by five maps
            pairs = [(si, mi) for si in range(5) for mi in range(5)]
            Ms = [the_maps(*SOURCES[si], *OUTS[mi])[mi] for si, mi in pairs]
            for r in range(4):
                bis = [(si + mi + r) % 4 for si, mi in pairs]
                words = [RB.word(*borders(fmt)[bi], source(fmt, si)) for (si, _), bi in zip(pairs, bis)]
                got, places = launch(ctx, fmt, RAGGED, opts, [source(fmt, si) for si, _ in pairs], Ms, words, [OUTS[mi] for _, mi in pairs])
                check_outputs(got, fmt, places, [ref(fmt, si, mi, bi, cubic) for (si, mi), bi in zip(pairs, bis)])


def test_the_borders_differ_from_one_another():
    """(the comparisons above are not of four equal pictures)"""
    for fmt in (0, 1, 2):
        for cubic in (False, True):
            pictures = [ref(fmt, 4, 2, bi, cubic) for bi in range(4)]
            assert all((pictures[a] != pictures[b]).mean() > 0.05 for a in range(4) for b in range(a))


@pytest.mark.parametrize("layout", [0, PACKED, RAGGED], ids=["plain", "packed", "ragged"])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_words_of_zero_give_the_call_without_the_bit(ctx, fmt, layout):
    si = 4
    w, h = SOURCES[si]
    n = 1 if layout == 0 else 5
    outs = OUTS[:n]
    Ms = [the_maps(w, h, ow, oh)[mi] for mi, (ow, oh) in enumerate(outs)]
    for cubic in (False, True):
        rule = CUBIC if cubic else 0
        without, places = launch(ctx, fmt, layout, rule, [source(fmt, si)] * n, Ms, [None] * n, outs)
        with_bit, places_b = launch(ctx, fmt, layout, rule | BORDER, [source(fmt, si)] * n, Ms, [0] * n, outs)
        assert places == places_b and without.tobytes() == with_bit.tobytes()
        old = RC.warp if cubic else R.warp
        check_outputs(with_bit, fmt, places, [old(source(fmt, si), M, ow, oh) for M, (ow, oh) in zip(Ms, outs)])


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ragged_batch_of_six_frames_each_with_its_own_border(ctx, fmt):
    frames, Ms, out_sizes = six_frames(fmt, False)
    bs = borders(fmt)
    per_frame = [bs[1], None, bs[0], bs[3], None, bs[2]]  # (two frames with the word 0)
    words = [0 if b is None else RB.word(b[0], b[1], frames[0]) for b in per_frame]
    for cubic in (False, True):
        got, places = launch(ctx, fmt, RAGGED, BORDER | (CUBIC if cubic else 0), frames, Ms, words, out_sizes)
        old = RC.warp if cubic else R.warp
        exp = [old(f, M, ow, oh) if b is None else RB.warp(f, M, ow, oh, b[0], b[1], cubic)
               for f, M, (ow, oh), b in zip(frames, Ms, out_sizes, per_frame)]
        check_outputs(got, fmt, places, exp)


def test_refusals_leave_the_destination_as_it_was(L, ctx):
    lib = L.lib()
    w, h = 64, 48
    n = w * h * 4
    d_src = ctx.device_upload(np.zeros(n, np.uint8))
    d_dst = ctx.device_upload(np.full(n, SENTINEL, np.uint8))
    M = np.eye(3).reshape(-1)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    f32 = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
    args = L.JpegArgs()  # (never read: the combination is refused first)

    def tables(word, bpp):
        """the same frame in the three layouts, the border word in its place"""
        plain = np.concatenate([M, [word]])
        packed = np.concatenate([M, [w, h, 0, w * bpp, word]])
        ragged = np.concatenate([M, [w, h, 0, w * bpp, w, h, 0, w * bpp, word]])
        return [(0, plain, w * bpp, w * bpp), (PACKED, packed, w * bpp, 0), (RAGGED, ragged, 0, 0)]

    def call(fmt_word, table, srow, drow, ww=w, hh=h):
        rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), n, 1, ww, hh, srow, fmt_word, P(table) if table is not None else None,
                                            C.c_void_p(d_dst), n, ww, hh, drow)
        return rc, lib.lr_last_error().decode()

    untouched = lambda: (ctx.device_download(d_dst, (n,), np.uint8) == SENTINEL).all()  # noqa: E731
    try:
        # the bit together with the calls that are no warp
        behind = C.cast(C.byref(args), C.c_void_p)
        for name, bit in (("LR_WARP_PREPARE", L.WARP_PREPARE), ("LR_WARP_LINES", L.WARP_LINES), ("LR_WARP_JPEG", L.WARP_JPEG),
                          ("LR_WARP_JPEG_DECODE", L.WARP_JPEG_DECODE)):
            rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), n, 1, 0, 0, 0, 1 | bit | BORDER, behind, C.c_void_p(d_dst), n, 0, 0, 0)
            err = lib.lr_last_error().decode()
            assert rc != 0 and "LR_WARP_BORDER" in err and name in err, (name, err)
        rc, err = call(1 | L.WARP_RAGGED | L.WARP_PREPARE | BORDER, tables(0.0, 3)[2][1], 0, 0)
        assert rc != 0 and "LR_WARP_BORDER" in err and "LR_WARP_PREPARE" in err
        assert untouched()
        # the word: not an integer in range, a refused mode, a value out of the format's range, a value with a mode that takes
        # none, f32 bits of no finite float
        bad = [(0, 0.5), (0, -1.0), (0, float("nan")), (0, float("inf")), (0, 2.0 ** 35), (1, 2.0 ** 35 + 8),
               (0, 3.0), (1, 5.0), (2, 6.0), (0, 7.0), (0, 3.0 + 8 * 9),
               (0, 8.0 * 256), (1, 8.0 * (1 << 24)), (0, 8.0 * 0xFFFFFFFF),
               (0, 1 + 8.0), (1, 2 + 8.0 * 255), (2, 4 + 8.0 * f32(1.0)),
               (2, 8.0 * f32(np.inf)), (2, 8.0 * f32(-np.inf)), (2, 8.0 * 0x7FC00000), (2, 8.0 * 0xFF800001)]
        for fmt, word in bad:
            for layout, table, srow, drow in tables(word, BPP[fmt]):
                for rule in (0, CUBIC):
                    rc, err = call(fmt | layout | BORDER | rule, table, srow, drow)
                    assert rc != 0, (fmt, word, layout)
                    assert err.startswith("lr_warp_perspective_device") and "LR_WARP_BORDER" in err and "frame 0" in err and "border word" in err, err
        assert untouched()
        # the second frame's word names the second frame
        two = np.concatenate([M, [1.0], M, [3.0]])
        rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), w * h, 2, w, h, w, 0 | BORDER, P(two), C.c_void_p(d_dst), w * h, w, h, w)
        assert rc != 0 and "frame 1" in lib.lr_last_error().decode()
        # what the call without the bit rejects, it rejects with it
        for layout, table, srow, drow in tables(1.0, 3):
            rc, err = call(3 | layout | BORDER, table, srow, drow)
            assert rc != 0 and "unknown pixel format" in err
            nan_map = table.copy()
            nan_map[4] = np.nan
            rc, err = call(1 | layout | BORDER, nan_map, srow, drow)
            assert rc != 0 and "not finite" in err
        # without the bit: a non-zero [17] and the unknown option bits stay refused, with the bit the unknown ones too
        rc, err = call(1 | RAGGED, tables(1.0, 3)[2][1], 0, 0)
        assert rc != 0 and "[17]" in err
        for unknown in (0x400, 0x10000, 1 << 30):
            for extra in (0, BORDER):
                for layout, table, srow, drow in tables(0.0, 3):
                    if not extra:
                        table = np.delete(table, len(table) - 1) if layout != RAGGED else table
                    rc, err = call(1 | layout | unknown | extra, table, srow, drow)
                    assert rc != 0 and "unknown option" in err, (hex(unknown), extra, layout, err)
        assert untouched()
        # and the next calls on the same context are right
        src = frame(1, w, h, 2)
        L._check(lib.lr_memcpy_h2d(ctx._h, C.c_void_p(d_src), P(src), src.nbytes))
        for layout, table, srow, drow in tables(float(RB.REFLECT), 3):
            rc, err = call(1 | layout | BORDER, table, srow, drow)
            assert rc == 0, err
            assert_same(ctx.device_download(d_dst, (h, w, 3), np.uint8), src)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


# ---- the Python level ----

def gray_of(rgb):
    c = rgb.astype(np.int32)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


@pytest.fixture(scope="module")
def pictures():
    rgb = [synthetic_rgb(w, h, seed) for w, h, seed in ((480, 360, 3), (333, 250, 4))]
    return {"colour": rgb, "gray": [gray_of(f) for f in rgb]}


SPECS = {0: [("replicate", RB.REPLICATE, 0), (("constant", 255), RB.CONSTANT, 255)],
         1: [("reflect101", RB.REFLECT_101, 0), (("constant", (255, 255, 255)), RB.CONSTANT, (255, 255, 255))]}


def test_warp_perspective_with_a_border(L, ctx):
    for fmt in (0, 1, 2):
        src = content(fmt, 33, 21, 8)
        M = the_maps(33, 21, 70, 45)[2]
        for name, (mode, value) in zip(NAMES, borders(fmt)):
            spec = ("constant", value) if name == "constant" else name
            for interp in ("linear", "cubic"):
                got = ctx.warp_perspective(src, M, (70, 45), interp=interp, border=spec)
                assert_same(got, RB.warp(src, M, 70, 45, mode, value, interp == "cubic"))
        assert_same(ctx.warp_perspective(src, M, (70, 45), border=None), R.warp(src, M, 70, 45))
    with pytest.raises(ValueError, match="warp_perspective"):
        ctx.warp_perspective(src, M, (70, 45), border="wrap")


def test_rectify_with_a_border_changes_the_picture_alone(L, ctx, pictures):
    for kind, fmt in (("colour", 1), ("gray", 0)):
        img = pictures[kind][0]
        lines0, t0, warped0 = ctx.rectify(img)
        _, M, size = L.rectification_homography(t0, 3.0)
        for spec, mode, value in SPECS[fmt]:
            for interp in ("linear", "cubic"):
                lines, t, warped = ctx.rectify(img, border=spec, interp=interp)
                assert lines.tobytes() == lines0.tobytes()
                np.testing.assert_array_equal(t.as_array(), t0.as_array())
                np.testing.assert_array_equal(warped, RB.warp(img, M, *size, mode, value, interp == "cubic"))
        assert (warped != warped0).any()
        # the prescaled path ends in the same launch
        _, t2, warped2 = ctx.rectify(img, max_size=400, border=SPECS[fmt][0][0])
        _, M2, size2 = L.rectification_homography(t2, 3.0)
        np.testing.assert_array_equal(warped2, RB.warp(img, M2, *size2, SPECS[fmt][0][1], 0))
    with pytest.raises(ValueError, match="rectify"):
        ctx.rectify(img, border=("constant", 300))


def test_rectify_with_crop_returns_the_second_sources_crop(L, ctx, pictures):
    img = pictures["colour"][0]
    lines0, t0, warped0 = ctx.rectify(img)
    H, M, size = L.rectification_homography(t0, 3.0)
    for interp in ("linear", "cubic"):
        cubic = interp == "cubic"
        M_ref, rect, _ = RB.crop(H, M, img.shape[1], img.shape[0], size[0], size[1], 1 if cubic else 0)
        exp = RB.warp(img, M_ref, rect[2], rect[3], RB.CONSTANT, (0, 0, 0), cubic)
        results = [ctx.rectify(img, crop=True, interp=interp, border=b) for b in (None, "reflect", ("constant", (255, 255, 255)))]
        for lines, t, warped, got_rect in results:
            assert lines.tobytes() == lines0.tobytes() and got_rect == rect
            np.testing.assert_array_equal(t.as_array(), t0.as_array())
            np.testing.assert_array_equal(warped, exp)
        assert rect[2] < size[0] and rect[3] < size[1]
    # (callers without crop get what they got)
    assert len(ctx.rectify(img, border="reflect")) == 3


@pytest.mark.parametrize("kind", ["gray", "colour"])
def test_rectify_batch_with_border_and_crop_is_a_loop_of_rectify(L, ctx, pictures, kind):
    frames = pictures[kind]
    fmt = 1 if kind == "colour" else 0
    specs = [SPECS[fmt][0][0], SPECS[fmt][1][0]]
    for interp, crop in (("linear", False), ("cubic", True), ("linear", True)):
        single = [ctx.rectify(f, border=b, crop=crop, interp=interp) for f, b in zip(frames, specs)]
        batch = ctx.rectify_batch(frames, border=specs, crop=crop, interp=interp)  # (two shapes: the ragged launch)
        same = ctx.rectify_batch(np.stack([frames[0], frames[0][::-1].copy()]), border=specs, crop=crop, interp=interp)  # (the packed launch)
        same_single = [ctx.rectify(frames[0], border=specs[0], crop=crop, interp=interp), ctx.rectify(frames[0][::-1].copy(), border=specs[1], crop=crop, interp=interp)]
        for got, exp in list(zip(batch, single)) + list(zip(same, same_single)):
            assert len(got) == len(exp) == (4 if crop else 3)
            assert got[0].tobytes() == exp[0].tobytes()
            np.testing.assert_array_equal(got[1].as_array(), exp[1].as_array())
            np.testing.assert_array_equal(got[2], exp[2])
            assert got[3:] == exp[3:]
        streams = ctx.rectify_batch(frames, jpeg=95, border=specs, crop=crop, interp=interp)
        for got, exp in zip(streams, single):
            assert got[2] == ctx.encode_jpeg(exp[2], 95) and got[3:] == exp[3:]
        assert ctx.rectify(frames[0], jpeg=95, border=specs[0], crop=crop, interp=interp)[2] == streams[0][2]
    with pytest.raises(ValueError, match="rectify_batch"):
        ctx.rectify_batch(frames, border=["reflect"])


def test_recipe_border_and_crop_write_what_the_library_computes(L, ctx, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(root, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(root, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    rgb = synthetic_rgb(480, 360, 7)
    ppm = str(tmp_path / "syn.ppm")
    with open(ppm, "wb") as f:
        f.write(b"P6\n480 360\n255\n" + rgb.tobytes())
    for bad in (["--border", "reflect"], ["--crop"], ["--warp", "--border", "wrap"], ["--warp", "--border", "reflect:3"], ["--warp", "--border", "constant:256"]):
        r = subprocess.run([exe, ppm, str(tmp_path / "none")] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and not os.path.exists(str(tmp_path / "none_lines.csv")), bad
    r = subprocess.run([exe, ppm, str(tmp_path / "a"), "--warp", "--border", "constant:255,128,0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "a_warp.ppm")), ctx.rectify(rgb, border=("constant", (255, 128, 0)))[2])
    r = subprocess.run([exe, ppm, str(tmp_path / "b"), "--warp", "--cubic", "--border", "reflect101", "--crop"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, _, want, rect = ctx.rectify(rgb, border="reflect101", crop=True, interp="cubic")
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "b_warp.ppm")), want)
    assert "crop %dx%d at (%d, %d)" % (rect[2], rect[3], rect[0], rect[1]) in r.stdout
