"""LR_WARP_AREA on the GPU against its NumPy second source (tests/numpy_warp_area_ref.py), byte for byte: three pixel formats,
five sampling factors, both sampling rules, every border mode, a lens, and all of them together; the GPU's own plain warp at
the fine size, box-averaged on the host, as a second check that involves no NumPy rule; mixed factors in one packed and one
ragged launch; what is refused; and out_max_size= of the Python paths and --out-max of the recipe."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_area_ref as RA
import numpy_warp_border_ref as RB
from test_gpu_rectify_warp import BPP, assert_same, frame, read_pnm
from test_gpu_warp_border import SENTINEL, check_outputs, lay_sources

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CUBIC, BORDER, PACKED, RAGGED, LENS, AREA = 0x8000, 0x40000, 0x200, 0x800, 0x100000, 0x400000


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


SOURCES = [(33, 21), (5, 5)]
OW, OH = 70, 19  # one full and one partial 64-wide tile, a second and partial tile row, a last lane with fewer than 4 pixels
FACTORS = [1, 2, 3, 5, 8]


def the_map(w, h):
    """a genuine perspective with wedges that minifies about 3 x and shows the source in the middle of the picture"""
    P = np.array([[1.1, 0.07, -3.2], [-0.05, 0.93, 2.5], [1e-4, -2e-4, 1.0]])
    return P @ np.array([[3.0, 0.0, 0.5 * w - 1.5 * OW], [0.0, 3.0, 0.5 * h - 1.5 * OH], [0.0, 0.0, 1.0]])


def the_lens(w, h):
    f = 0.6 * max(w, h)
    return (f, 1.1 * f, (w - 1) / 2.0 + 1.5, (h - 1) / 2.0 - 0.75, 0.25, 0.05, 0.01, -0.02, 0.02)


def border_specs(fmt):
    """(the Python spec, the reference's mode and value): none, constant 200, replicate, reflect, reflect-101"""
    v = {0: 200, 1: (7, 200, 31), 2: -1.5}[fmt]
    return [(None, RB.CONSTANT, (0, 0, 0) if fmt == 1 else 0), (("constant", v), RB.CONSTANT, v), ("replicate", RB.REPLICATE, 0),
            ("reflect", RB.REFLECT, 0), ("reflect101", RB.REFLECT_101, 0)]


# (interp, index into border_specs, with the lens): linear, cubic, each border mode once, a lens, and cubic + reflect-101 + lens
CASES = [("linear", 0, False), ("cubic", 0, False), ("linear", 1, False), ("linear", 2, False), ("cubic", 3, False), ("linear", 4, False),
         ("linear", 0, True), ("cubic", 4, True)]

_SRC = {}


def source(fmt, si):
    if (fmt, si) not in _SRC:
        _SRC[fmt, si] = frame(fmt, SOURCES[si][0], SOURCES[si][1], 700 + si)
    return _SRC[fmt, si]


def launch(L, ctx, fmt, layout, opts, srcs, Ms, out_sizes, areas, borders=None, lenses=None, odd=True):
    """One launch in the given layout (0 plain, PACKED, RAGGED) with tables from the package's builders; odd: align 1 (f32: 4)
    and padded rows, so that rows and frames start at odd addresses and the unaligned stores run.  areas: a factor per frame, or
    None (the bit is not set).  Returns (destination bytes, places)."""
    bpp, step = BPP[fmt], 4 if fmt == 2 else 1
    pad = (3 * step) if odd else 0
    n = len(srcs)
    sbuf, splaces = lay_sources(fmt, srcs, layout != RAGGED)
    w, h, soff, srow = splaces[0]
    simg = splaces[1][2] - soff if n > 1 else h * srow
    bits = opts | (BORDER if borders is not None else 0) | (LENS if lenses is not None else 0) | (AREA if areas is not None else 0)
    lead = pad if odd else 16
    align = step if odd else 4
    if layout == 0:
        ow, oh = out_sizes[0]
        drow = ow * bpp + pad
        dimg = oh * drow + (5 * step if odd else 0)
        places = [(ow, oh, lead + b * dimg, drow) for b in range(n)]
        region = lead + n * dimg + 16
        rows = []
        for b in range(n):
            _, row = L._border_bit_and_map(None if borders is None else borders[b], fmt, Ms[b], "test", None if lenses is None else lenses[b],
                                           None if areas is None else areas[b])
            row = np.asarray(row, np.float64).reshape(-1)
            if borders is not None and borders[b] is None:  # (a frame of the bordered launch with the zero border: the word 0)
                row = np.concatenate([row[:9], [0.0], row[9:]])
            rows.append(row)
        table = np.stack(rows)
    elif layout == PACKED:
        table, total = L.warp_table(np.stack(Ms), np.array(out_sizes), bpp, align=align, border=borders, lens=lenses, area=areas)
    else:
        table, total = L.ragged_table(np.stack(Ms), np.array(out_sizes), np.array(splaces), bpp, align=align, border=borders, lens=lenses, area=areas)
    if layout != 0:
        places = [tuple(int(v) for v in table[b, 9:13]) for b in range(n)]
        region = lead + total + 16
    d_src, d_dst = ctx.device_upload(sbuf), ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    try:
        if layout == 0:
            ctx.warp_perspective_device(d_src + soff, simg, n, w, h, srow, fmt | bits, table, d_dst + lead, dimg, ow, oh, drow)
        elif layout == PACKED:
            ctx.warp_perspective_packed_device(d_src + soff, simg, n, w, h, srow, fmt | bits, table, d_dst + lead, total)
        else:
            ctx.warp_perspective_ragged_device(d_src, len(sbuf), fmt | bits, table, d_dst + lead, total)
        got = ctx.device_download(d_dst, (region,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    if layout != 0:
        places = [(ow, oh, off + lead, row) for ow, oh, off, row in places]
    return got, places


@pytest.mark.parametrize("S", FACTORS)
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_byte_for_byte_against_the_second_source(L, ctx, fmt, S):
    """one plain launch per source size with a frame per case: every frame has the factor S"""
    specs = border_specs(fmt)
    for si, (w, h) in enumerate(SOURCES):
        src, M, lens = source(fmt, si), the_map(w, h), the_lens(w, h)
        for cubic in (False, True):
            cases = [c for c in CASES if (c[0] == "cubic") == cubic]
            n = len(cases)
            borders = [specs[bi][0] for _, bi, _ in cases]
            lenses = [L.Lens(*lens) if lensed else L.Lens(1.0, 1.0, 0.0, 0.0) for _, _, lensed in cases]
            exp = [RA.warp_area(src, M, OW, OH, S, lens if lensed else None, specs[bi][1], specs[bi][2], cubic) for _, bi, lensed in cases]
            for odd in ((True, False) if fmt == 1 else (True,)):  # (u8x3: an odd row stride for the unaligned stores, an even one for the dwords)
                got, places = launch(L, ctx, fmt, 0, CUBIC if cubic else 0, [src] * n, [M] * n, [(OW, OH)] * n, [S] * n, borders, lenses, odd)
                check_outputs(got, fmt, places, exp)
            if S > 1:  # (the comparison is not one of equal pictures: the factor changes the picture)
                plain = RA.warp_area(src, M, OW, OH, 1, None, specs[0][1], specs[0][2], cubic)
                assert si == 1 or (plain != exp[0]).mean() > 0.02
    # without a border word and without lens entries: rows of ten doubles
    src, M = source(fmt, 0), the_map(*SOURCES[0])
    got, places = launch(L, ctx, fmt, 0, 0, [src], [M], [(OW, OH)], [S])
    check_outputs(got, fmt, places, [RA.warp_area(src, M, OW, OH, S)])
    assert_same(ctx.warp_perspective(src, M, (OW, OH), area=S), RA.warp_area(src, M, OW, OH, S))


@pytest.mark.parametrize("S", [2, 3, 8])
@pytest.mark.parametrize("fmt,interp", [(0, "linear"), (1, "linear"), (2, "linear"), (1, "cubic")])
def test_the_area_call_is_the_box_mean_of_the_plain_warp_at_the_fine_size(L, ctx, fmt, interp, S):
    """no NumPy rule involved: the GPU's own warp without the bit, map area_fine_map(M, S), into S 70 x S 19, averaged here"""
    for si, (w, h) in enumerate(SOURCES):
        src, M = source(fmt, si), the_map(w, h)
        fine = ctx.warp_perspective(src, L.area_fine_map(M, S), (S * OW, S * OH), interp=interp)
        assert fine.shape[:2] == (S * OH, S * OW)
        assert_same(ctx.warp_perspective(src, M, (OW, OH), interp=interp, area=S), RA.box_mean(fine, S))


@pytest.mark.parametrize("S", [4, 6, 7])
def test_the_other_factors(L, ctx, S):
    """the factors the cases above leave out: 6 and 7 do not divide the kernel's 64 x 16 tile of samples, 4 does"""
    for fmt in (0, 1, 2):
        src, M = source(fmt, 0), the_map(*SOURCES[0])
        for interp, border, mode in (("linear", None, RB.CONSTANT), ("cubic", "reflect", RB.REFLECT)):
            got = ctx.warp_perspective(src, M, (OW, OH), interp=interp, border=border, area=S)
            assert_same(got, RA.warp_area(src, M, OW, OH, S, None, mode, (0, 0, 0) if fmt == 1 else 0, interp == "cubic"))


FOUR = [((70, 19), 1), ((33, 40), 4), ((129, 5), 2), ((8, 17), 8)]  # (output size, factor) of four frames in one launch


@pytest.mark.parametrize("layout", [PACKED, RAGGED], ids=["packed", "ragged"])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_four_frames_with_different_factors_in_one_launch(L, ctx, fmt, layout):
    sizes = [(33, 21)] * 4 if layout == PACKED else [(33, 21), (5, 5), (45, 30), (17, 64)]
    srcs = [frame(fmt, w, h, 720 + k) for k, (w, h) in enumerate(sizes)]
    Ms = [np.array([[1.0, 0.0, 0.5 * w], [0.0, 1.0, 0.5 * h], [0.0, 0.0, 1.0]]) @ np.array([[1.1, 0.07, 0.0], [-0.05, 0.93, 0.0], [1e-4, -2e-4, 1.0]])
          @ np.array([[3.0 * w / 33.0, 0.0, -1.5 * w / 33.0 * ow], [0.0, 3.0 * h / 21.0, -1.5 * h / 21.0 * oh], [0.0, 0.0, 1.0]])
          for (w, h), ((ow, oh), _) in zip(sizes, FOUR)]
    out_sizes, factors = [f[0] for f in FOUR], [f[1] for f in FOUR]
    for cubic, borders, lensed in ((False, None, False), (True, ["reflect", None, "replicate", "reflect101"], True)):
        interp = "cubic" if cubic else "linear"
        lenses = [L.Lens(*the_lens(w, h)) if k != 2 else None for k, (w, h) in enumerate(sizes)] if lensed else None
        got, places = launch(L, ctx, fmt, layout, CUBIC if cubic else 0, srcs, Ms, out_sizes, factors, borders, lenses)
        single = [ctx.warp_perspective(srcs[k], Ms[k], out_sizes[k], interp=interp, border=None if borders is None else borders[k],
                                       lens=None if lenses is None else lenses[k], area=factors[k]) for k in range(4)]
        check_outputs(got, fmt, places, single)  # (and nothing outside the frames' pixels was written)
        # the frame with S = 1 is the frame of the call without the bit
        assert_same(single[0], ctx.warp_perspective(srcs[0], Ms[0], out_sizes[0], interp=interp, border=None if borders is None else borders[0],
                                                    lens=None if lenses is None else lenses[0]))
        for k in (1, 3):
            b = border_specs(fmt)[{None: 0, "reflect101": 4}[None if borders is None else borders[k]]]
            assert_same(single[k], RA.warp_area(srcs[k], Ms[k], out_sizes[k][0], out_sizes[k][1], factors[k], None if lenses is None else lenses[k], b[1], b[2], cubic))
    # every factor 1: byte for byte the launch without the bit
    ones, places1 = launch(L, ctx, fmt, layout, 0, srcs, Ms, out_sizes, [1] * 4)
    without, places0 = launch(L, ctx, fmt, layout, 0, srcs, Ms, out_sizes, None)
    assert places1 == places0 and ones.tobytes() == without.tobytes()


def test_refusals_leave_the_destination_as_it_was(L, ctx):
    lib = L.lib()
    w, h = 64, 48
    n = w * h * 4
    d_src = ctx.device_upload(np.zeros(n, np.uint8))
    d_dst = ctx.device_upload(np.full(n, SENTINEL, np.uint8))
    M = np.eye(3).reshape(-1)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = L.JpegArgs()  # (never read: the combination is refused first)
    lens = np.array([50.0, 50.0, 31.5, 23.5, -0.2, 0.05, 0.001, -0.001, 0.0])

    def tables(S, bpp, word=None, lensed=False):
        """the same frame in the three layouts, the factor at the very end of its row (behind the border word and the lens, if any)"""
        tail = np.concatenate([[] if word is None else [word], lens if lensed else [], [S]])
        plain = np.concatenate([M, tail])
        packed = np.concatenate([M, [w, h, 0, w * bpp], tail])
        ragged = np.concatenate([M, [w, h, 0, w * bpp, w, h, 0, w * bpp, 0.0 if word is None else word], lens if lensed else [], [S]])
        return [(0, plain, w * bpp, w * bpp), (PACKED, packed, w * bpp, 0), (RAGGED, ragged, 0, 0)]

    def call(fmt_word, table, srow, drow):
        rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), n, 1, w, h, srow, fmt_word, P(table), C.c_void_p(d_dst), n, w, h, drow)
        return rc, lib.lr_last_error().decode()

    untouched = lambda: (ctx.device_download(d_dst, (n,), np.uint8) == SENTINEL).all()  # noqa: E731
    try:
        # the bit together with the calls that are no warp
        behind = C.cast(C.byref(args), C.c_void_p)
        for name, bit in (("LR_WARP_PREPARE", L.WARP_PREPARE), ("LR_WARP_LINES", L.WARP_LINES), ("LR_WARP_JPEG", L.WARP_JPEG),
                          ("LR_WARP_JPEG_DECODE", L.WARP_JPEG_DECODE)):
            rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), n, 1, 0, 0, 0, 1 | bit | AREA, behind, C.c_void_p(d_dst), n, 0, 0, 0)
            err = lib.lr_last_error().decode()
            assert rc != 0 and "LR_WARP_AREA" in err and name in err, (name, err)
        rc, err = call(1 | L.WARP_RAGGED | L.WARP_PREPARE | AREA, tables(2.0, 3)[2][1], 0, 0)
        assert rc != 0 and "LR_WARP_AREA" in err and "LR_WARP_PREPARE" in err
        assert untouched()
        # a factor that is no integer from 1 to 8
        for S in (0.0, 9.0, 2.5, float("nan"), -1.0, float("inf"), 1e300):
            for fmt in (0, 1, 2):
                for word, lensed in ((None, False), (1.0, False), (None, True), (2.0, True)):
                    for layout, table, srow, drow in tables(S, BPP[fmt], word, lensed):
                        for rule in (0, CUBIC):
                            rc, err = call(fmt | layout | AREA | rule | (BORDER if word is not None else 0) | (LENS if lensed else 0), table, srow, drow)
                            assert rc != 0, (S, fmt, layout)
                            assert err.startswith("lr_warp_perspective_device") and "LR_WARP_AREA" in err and "frame 0" in err and "1 to 8" in err, err
        assert untouched()
        # the second frame's factor names the second frame
        two = np.concatenate([M, [2.0], M, [9.0]])
        rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), w * h, 2, w, h, w, 0 | AREA, P(two), C.c_void_p(d_dst), w * h, w, h, w)
        assert rc != 0 and "frame 1" in lib.lr_last_error().decode()
        # what the call without the bit rejects, it rejects with it; unknown option bits stay unknown
        for layout, table, srow, drow in tables(2.0, 3):
            rc, err = call(3 | layout | AREA, table, srow, drow)
            assert rc != 0 and "unknown pixel format" in err
            nan_map = table.copy()
            nan_map[4] = np.nan
            rc, err = call(1 | layout | AREA, nan_map, srow, drow)
            assert rc != 0 and "not finite" in err
            for unknown in (0x400, 0x10000, 0x200000, 1 << 30):
                rc, err = call(1 | layout | unknown | AREA, table, srow, drow)
                assert rc != 0 and "unknown option" in err, (hex(unknown), layout, err)
        bad_word = tables(2.0, 3, 3.0)  # (border mode 3 is refused as without the bit)
        for layout, table, srow, drow in bad_word:
            rc, err = call(1 | layout | AREA | BORDER, table, srow, drow)
            assert rc != 0 and "LR_WARP_BORDER" in err
        assert untouched()
        # and the next calls on the same context are right
        src = frame(1, w, h, 2)
        L._check(lib.lr_memcpy_h2d(ctx._h, C.c_void_p(d_src), P(src), src.nbytes))
        for layout, table, srow, drow in tables(2.0, 3, None, True):
            rc, err = call(1 | layout | AREA | LENS, table, srow, drow)
            assert rc == 0, err
            assert_same(ctx.device_download(d_dst, (h, w, 3), np.uint8), RA.warp_area(src, np.eye(3), w, h, 2, lens))
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def test_a_factor_times_the_output_size_above_int_max_is_refused(L, ctx):
    """S * out_width and S * out_height above 2^31 - 1: an output of 2^28 + 1 pixels in a row, or in a column, with S = 8.  The
    destination is as large as the call says, and its two ends are looked at."""
    lib = L.lib()
    big = 2 ** 28 + 1
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    d_src = ctx.device_upload(np.zeros(64, np.uint8))
    d_dst = C.c_void_p()
    L._check(lib.lr_device_malloc(ctx._h, big, C.byref(d_dst)))
    ends = np.full(4096, SENTINEL, np.uint8)
    try:
        for at in (0, big - 4096):
            L._check(lib.lr_memcpy_h2d(ctx._h, C.c_void_p(d_dst.value + at), P(ends), 4096))
        M = np.eye(3).reshape(-1)
        for ow, oh, what in ((big, 1, "width"), (1, big, "height")):
            rows = [(0, np.concatenate([M, [8.0]]), 8, ow), (PACKED, np.concatenate([M, [ow, oh, 0, ow], [8.0]]), 8, 0),
                    (RAGGED, np.concatenate([M, [ow, oh, 0, ow, 8, 8, 0, 8, 0.0], [8.0]]), 0, 0)]
            for layout, table, srow, drow in rows:
                rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), 64, 1, 8, 8, srow, 0 | layout | AREA, P(table), d_dst, big, ow, oh, drow)
                err = lib.lr_last_error().decode()
                assert rc != 0 and "LR_WARP_AREA" in err and "frame 0" in err and what in err and "2^31" in err, (layout, err)
        for at in (0, big - 4096):
            assert (ctx.device_download(d_dst.value + at, (4096,), np.uint8) == SENTINEL).all()
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst.value)


# ---- the Python level ----

@pytest.fixture(scope="module")
def photograph():
    """the golden photograph's luma at half size, cropped to 320 x 240"""
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    return np.ascontiguousarray(gray[::2, ::2][21:261, 90:410])


def lens_of(img):
    h, w = img.shape[:2]
    return (0.8 * max(w, h), 0.8 * max(w, h), (w - 1) / 2.0, (h - 1) / 2.0, -0.12, 0.02, 0.001, -0.0005, 0.0)


def test_rectify_with_a_bound_on_the_size(L, ctx, photograph):
    img = photograph
    assert img.shape == (240, 320)
    lines0, t0, full = ctx.rectify(img)
    assert len(lines0) > 10 and max(full.shape) > 200
    lines, t, small = ctx.rectify(img, out_max_size=200)
    assert lines.tobytes() == lines0.tobytes()
    np.testing.assert_array_equal(t.as_array(), t0.as_array())
    H, M, size = L.rectification_homography(t, 3.0)
    H2, M2, size2, S = L.shrink_homography(H, M, size, 200)
    assert max(size2) == 200 and S >= 2 and small.shape == (size2[1], size2[0])
    np.testing.assert_array_equal(small, RA.warp_area(img, M2, size2[0], size2[1], S))
    np.testing.assert_array_equal(small, ctx.warp_perspective(img, M2, size2, area=S))
    # None, and a bound the picture already fits: today's call
    np.testing.assert_array_equal(ctx.rectify(img, out_max_size=None)[2], full)
    np.testing.assert_array_equal(ctx.rectify(img, out_max_size=max(size))[2], full)
    # with the other options of the call: cubic, a border, a lens; the prescale; the crop; the encoder
    lens = L.Lens(*lens_of(img))
    _, tl, got = ctx.rectify(img, out_max_size=150, interp="cubic", border="reflect101", lens=lens)
    _, Ml, sizel = L.rectification_homography(tl, 3.0)
    _, Ml, sizel, Sl = L.shrink_homography(None, Ml, sizel, 150)
    np.testing.assert_array_equal(got, ctx.warp_perspective(img, Ml, sizel, interp="cubic", border="reflect101", lens=lens, area=Sl))
    _, tp, got = ctx.rectify(img, out_max_size=120, max_size=200)
    _, Mp, sizep = L.rectification_homography(tp, 3.0)
    _, Mp, sizep, Sp = L.shrink_homography(None, Mp, sizep, 120)
    np.testing.assert_array_equal(got, ctx.warp_perspective(img, Mp, sizep, area=Sp))
    _, tc, got, rect = ctx.rectify(img, out_max_size=100, crop=True)
    Hc, Mc, sizec = L.rectification_homography(tc, 3.0)
    _, Mc, rect_c = L.crop_homography(Hc, Mc, 320, 240, sizec, 0)
    assert rect == rect_c  # (the rectangle stays in the uncropped full-size picture)
    _, Mc, sizec, Sc = L.shrink_homography(None, Mc, rect_c[2:], 100)  # (applied after the crop)
    assert max(got.shape) <= 100
    np.testing.assert_array_equal(got, ctx.warp_perspective(img, Mc, sizec, area=Sc))
    assert ctx.rectify(img, out_max_size=200, jpeg=90)[2] == ctx.encode_jpeg(small, 90)  # (it runs before the encoder)
    for bad in (0, -5, 2.5, True, "200"):
        with pytest.raises(ValueError, match="out_max_size"):
            ctx.rectify(img, out_max_size=bad)


def test_rectify_batch_with_a_bound_is_a_loop_of_rectify(L, ctx, photograph):
    same = [photograph, np.ascontiguousarray(photograph[::-1]), np.ascontiguousarray(photograph[:, ::-1])]  # (one shape: the packed warp)
    mixed = same[:2] + [np.ascontiguousarray(photograph[:200, :300])]  # (two shapes: the ragged warp)
    for frames in (np.stack(same), mixed):
        for kwargs in ({"out_max_size": 200}, {"out_max_size": 90, "interp": "cubic", "border": "replicate"}, {"out_max_size": 150, "crop": True}):
            single = [ctx.rectify(f, **kwargs) for f in frames]
            batch = ctx.rectify_batch(frames, **kwargs)
            assert len(batch) == 3
            for got, exp in zip(batch, single):
                assert len(got) == len(exp)
                assert got[0].tobytes() == exp[0].tobytes()
                np.testing.assert_array_equal(got[1].as_array(), exp[1].as_array())
                np.testing.assert_array_equal(got[2], exp[2])
                assert max(got[2].shape) <= kwargs["out_max_size"] and got[3:] == exp[3:]
        none = ctx.rectify_batch(frames, out_max_size=None)
        today = ctx.rectify_batch(frames)
        for got, exp in zip(none, today):
            np.testing.assert_array_equal(got[2], exp[2])
    # files in, files out: the bound runs behind the decoder and before the encoder
    data = [ctx.encode_jpeg(f, 95) for f in mixed]
    got = ctx.rectify_batch(data, out_max_size=160, jpeg=90)
    exp = [ctx.rectify(ctx.decode_jpeg(d, L.PIX_U8), out_max_size=160) for d in data]
    assert [g[2] for g in got] == [ctx.encode_jpeg(e[2], 90) for e in exp]
    # a lens per frame goes with it
    lenses = [L.Lens(*lens_of(f)) for f in mixed]
    got = ctx.rectify_batch(mixed, out_max_size=130, lens=lenses)
    for g, f, lens in zip(got, mixed, lenses):
        np.testing.assert_array_equal(g[2], ctx.rectify(f, out_max_size=130, lens=lens)[2])
    with pytest.raises(ValueError, match="out_max_size"):
        ctx.rectify_batch(mixed, out_max_size=0)


def test_recipe_out_max_writes_what_the_library_computes(L, ctx, tmp_path, photograph):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    img = photograph
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    for bad in (["--out-max", "200"], ["--warp", "--out-max", "0"], ["--warp", "--out-max"]):
        r = subprocess.run([exe, pgm, str(tmp_path / "none")] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and not os.path.exists(str(tmp_path / "none_lines.csv")), bad
    r = subprocess.run([exe, pgm, str(tmp_path / "a"), "--warp", "--out-max", "200"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "a_warp.pgm")), ctx.rectify(img, out_max_size=200)[2])
    r = subprocess.run([exe, pgm, str(tmp_path / "b"), "--warp", "--cubic", "--border", "reflect101", "--crop", "--out-max", "100"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "b_warp.pgm")), ctx.rectify(img, out_max_size=100, interp="cubic", border="reflect101", crop=True)[2])
