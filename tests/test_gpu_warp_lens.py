"""LR_WARP_LENS on the GPU against its NumPy second source (tests/numpy_warp_lens_ref.py), byte for byte: three pixel formats,
the plain, the packed and the ragged launch, both sampling rules, with and without border rules, three maps and four lenses
(one whose taps lie far outside, one that makes infinities and NaN inside the picture); rows of zero coefficients against the
call without the bit; what is refused; and lens= of the Python paths and of the recipe."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_border_ref as RB
import numpy_warp_lens_ref as RL
from test_gpu_rectify_warp import BPP, assert_same, frame, read_pnm, synthetic_rgb
from test_gpu_warp_border import SENTINEL, check_outputs, gray_of, lay_sources
from test_gpu_warp_cubic import six_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CUBIC, BORDER, PACKED, RAGGED, LENS = 0x8000, 0x40000, 0x200, 0x800, 0x100000


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


SOURCES = [(67, 35), (45, 70)]
OW, OH = 131, 37  # three tile columns and three tile rows, the last of each partial


def the_maps(w, h):
    """the identity, a perspective whose W0 = 0 line crosses the output, a rotation by 30 degrees with scale 0.7 about the
    source's centre"""
    c, s = 0.7 * math.cos(math.pi / 6), 0.7 * math.sin(math.pi / 6)
    cx, cy = w / 2.0, h / 2.0
    return [
        np.eye(3),
        np.array([[0.9, 0.1, 0.0], [0.05, 1.1, 0.0], [1.0 / OW, 1.7 / OH, -1.3]]),
        np.array([[c, -s, cx - c * 0.5 * OW + s * 0.5 * OH], [s, c, cy - s * 0.5 * OW - c * 0.5 * OH], [0, 0, 1.0]]),
    ]


def the_lenses(w, h):
    """barrel, pincushion with tangential terms, an extreme one (most taps far outside), and one with k3 = 1e300 and a focal
    length of half a pixel, whose radial term overflows a few pixels from the centre: infinities, and NaN (0 * inf) on the
    column and the row through the integer centre"""
    f, cx, cy = 0.6 * max(w, h), (w - 1) / 2.0, (h - 1) / 2.0
    return [
        (f, f, cx, cy, -0.3, 0.1, 0.0, 0.0, 0.0),
        (f, 1.1 * f, cx + 1.5, cy - 0.75, 0.25, 0.05, 0.01, -0.02, 0.02),
        (f, f, cx, cy, 50.0, 0.0, 0.0, 0.0, 0.0),
        (0.5, 0.5, float(w // 2), float(h // 2), 0.0, 0.0, 0.0, 0.0, 1e300),
    ]


def border_specs(fmt):
    """(the Python spec, the reference's mode and value): none, constant 200, replicate, reflect, reflect-101"""
    v = {0: 200, 1: (200, 200, 200), 2: 200.0}[fmt]
    return [(None, RB.CONSTANT, (0, 0, 0) if fmt == 1 else 0), (("constant", v), RB.CONSTANT, v), ("replicate", RB.REPLICATE, 0),
            ("reflect", RB.REFLECT, 0), ("reflect101", RB.REFLECT_101, 0)]


_SRC, _REF = {}, {}


def source(fmt, si):
    if (fmt, si) not in _SRC:
        _SRC[fmt, si] = frame(fmt, SOURCES[si][0], SOURCES[si][1], 500 + si)
    return _SRC[fmt, si]


def ref(fmt, si, mi, li, bi, cubic):
    """the second source's picture, computed once and shared by the three layouts; li None: no lens"""
    key = (fmt, si, mi, li, bi, cubic)
    if key not in _REF:
        w, h = SOURCES[si]
        _, mode, value = border_specs(fmt)[bi]
        lens = None if li is None else the_lenses(w, h)[li]
        _REF[key] = RL.warp(source(fmt, si), the_maps(w, h)[mi], OW, OH, lens, mode, value, cubic)
        _REF[key].setflags(write=False)
    return _REF[key]


def launch(L, ctx, fmt, layout, opts, srcs, Ms, out_sizes, borders=None, lenses=None):
    """One launch in the given layout (0 plain, PACKED, RAGGED) with tables from the package's builders, align=1 (f32: 4), so
    that rows and frames start at odd addresses; sources at odd offsets with padded rows.  borders / lenses: a list per frame or
    None (the bit is not set).  Returns (destination bytes, places)."""
    bpp, step = BPP[fmt], 4 if fmt == 2 else 1
    n = len(srcs)
    sbuf, splaces = lay_sources(fmt, srcs, layout != RAGGED)
    w, h, soff, srow = splaces[0]
    simg = splaces[1][2] - soff if n > 1 else h * srow
    bits = opts | (BORDER if borders is not None else 0) | (LENS if lenses is not None else 0)
    lead = 3 * step  # the frames start here in the region, and 16 bytes of sentinel follow the last
    if layout == 0:
        ow, oh = out_sizes[0]
        drow = ow * bpp + 3 * step
        dimg = oh * drow + 5 * step
        places = [(ow, oh, lead + b * dimg, drow) for b in range(n)]
        region = lead + n * dimg + 16
        rows = []
        for b in range(n):
            lens = None if lenses is None else (lenses[b] or L.Lens(1.0, 1.0, 0.0, 0.0))  # (a frame of None: zeros, as in the tables)
            _, row = L._border_bit_and_map(None if borders is None else borders[b], fmt, Ms[b], "test", lens)
            row = np.asarray(row, np.float64).reshape(-1)
            if borders is not None and borders[b] is None:  # (a frame of the bordered launch with the zero border: the word 0)
                row = np.concatenate([row[:9], [0.0], row[9:]])
            rows.append(np.asarray(row, np.float64).reshape(-1))
        table = np.stack(rows)
    elif layout == PACKED:
        table, total = L.warp_table(np.stack(Ms), np.array(out_sizes), bpp, align=step, border=borders, lens=lenses)
        places = [tuple(int(v) for v in table[b, 9:13]) for b in range(n)]
        region = lead + total + 16
    else:
        table, total = L.ragged_table(np.stack(Ms), np.array(out_sizes), np.array(splaces), bpp, align=step, border=borders, lens=lenses)
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


@pytest.mark.parametrize("layout", [0, PACKED, RAGGED], ids=["plain", "packed", "ragged"])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_byte_for_byte_against_the_second_source(L, ctx, fmt, layout):
    specs = border_specs(fmt)
    for cubic in (False, True):
        opts = CUBIC if cubic else 0
        # without LR_WARP_BORDER: every map with every lens; with it: one frame each of the four rules (frame k: map k % 3, lens k)
        plain_frames = [(mi, li, 0) for mi in range(3) for li in range(4)]
        border_frames = [(k % 3, k, k + 1) for k in range(4)]
        for frames, bordered in ((plain_frames, False), (border_frames, True)):
            groups = [[(si,) + f for f in frames] for si in range(2)] if layout != RAGGED else [[(si,) + f for si in range(2) for f in frames]]
            for group in groups:  # plain and packed: a launch per source size; ragged: both sources' frames in one launch
                srcs = [source(fmt, si) for si, _, _, _ in group]
                Ms = [the_maps(*SOURCES[si])[mi] for si, mi, _, _ in group]
                lenses = [L.Lens(*the_lenses(*SOURCES[si])[li]) for si, _, li, _ in group]
                borders = [specs[bi][0] for _, _, _, bi in group] if bordered else None
                got, places = launch(L, ctx, fmt, layout, opts, srcs, Ms, [(OW, OH)] * len(group), borders, lenses)
                check_outputs(got, fmt, places, [ref(fmt, si, mi, li, bi, cubic) for si, mi, li, bi in group])


def test_the_lenses_change_the_pictures_and_the_odd_ones_are_odd(L):
    """(the comparisons above are not of equal pictures; the extreme lens leaves most taps outside, the overflowing one makes
    infinities and NaN inside the picture)"""
    w, h = SOURCES[0]
    for cubic in (False, True):
        none = ref(0, 0, 0, None, 0, cubic)
        assert all((ref(0, 0, 0, li, 0, cubic) != none).mean() > 0.3 for li in range(4))
        assert (ref(0, 0, 0, 2, 0, cubic) == 0).mean() > 0.8
    lens = the_lenses(w, h)[3]
    d = L.lens_distort(L.Lens(*lens), np.stack(np.meshgrid(np.arange(float(OW)), np.arange(float(OH))), axis=-1))
    assert np.isinf(d).any() and np.isnan(d).any() and np.isfinite(d).any()
    X, Y = RL.fixed_coords(the_maps(w, h)[0], OW, OH, lens)
    assert (X[np.isnan(d[..., 0])] == -2147483648).all() and (X == 2147483647).any() and (X == w // 2 * 32).any()


@pytest.mark.parametrize("layout", [0, PACKED, RAGGED], ids=["plain", "packed", "ragged"])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_rows_of_zero_coefficients_give_the_call_without_the_bit(L, ctx, fmt, layout):
    si = 0
    w, h = SOURCES[si]
    n = 3
    Ms = the_maps(w, h)
    zeros = [L.Lens(40.0, 41.0, 3.0, 5.0), None, L.Lens(1e-3, 1e6, -7.0, 1e9, -0.0, 0.0, -0.0, 0.0, -0.0)]
    for cubic in (False, True):
        opts = CUBIC if cubic else 0
        for borders in (None, [None, "reflect", ("constant", border_specs(fmt)[1][0][1])]):
            without, places = launch(L, ctx, fmt, layout, opts, [source(fmt, si)] * n, Ms, [(OW, OH)] * n, borders, None)
            with_bit, places_b = launch(L, ctx, fmt, layout, opts, [source(fmt, si)] * n, Ms, [(OW, OH)] * n, borders, zeros)
            assert places == places_b and without.tobytes() == with_bit.tobytes()
        check_outputs(with_bit, fmt, places, [ref(fmt, si, 0, None, 0, cubic), ref(fmt, si, 1, None, 3, cubic), ref(fmt, si, 2, None, 1, cubic)])


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ragged_batch_of_six_frames_three_with_a_lens(L, ctx, fmt):
    frames, Ms, out_sizes = six_frames(fmt, False)
    lenses = []
    for b, f in enumerate(frames):
        h, w = f.shape[:2]
        lenses.append(L.Lens(*the_lenses(w, h)[b // 2]) if b in (0, 2, 4) else (None if b == 1 else L.Lens(30.0, 30.0, 1.0, 2.0)))
    for cubic in (False, True):
        got, places = launch(L, ctx, fmt, RAGGED, CUBIC if cubic else 0, frames, Ms, out_sizes, None, lenses)
        interp = "cubic" if cubic else "linear"
        single = [ctx.warp_perspective(f, M, size, interp=interp, lens=lens) for f, M, size, lens in zip(frames, Ms, out_sizes, lenses)]
        check_outputs(got, fmt, places, single)
        for b in (1, 3, 5):  # (the frames of zeros are the frames of the call without the bit)
            assert_same(single[b], ctx.warp_perspective(frames[b], Ms[b], out_sizes[b], interp=interp))
        for b in (0, 2, 4):
            assert_same(single[b], RL.warp(frames[b], Ms[b], out_sizes[b][0], out_sizes[b][1], lenses[b], cubic=cubic))


def test_refusals_leave_the_destination_as_it_was(L, ctx):
    lib = L.lib()
    w, h = 64, 48
    n = w * h * 4
    d_src = ctx.device_upload(np.zeros(n, np.uint8))
    d_dst = ctx.device_upload(np.full(n, SENTINEL, np.uint8))
    M = np.eye(3).reshape(-1)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = L.JpegArgs()  # (never read: the combination is refused first)
    good = np.array([50.0, 50.0, 31.5, 23.5, -0.2, 0.05, 0.001, -0.001, 0.0])

    def tables(lens, bpp, word=None):
        """the same frame in the three layouts, the nine lens entries at the end of its row (behind the border word, if any)"""
        tail = ([] if word is None else [word])
        plain = np.concatenate([M, tail, lens])
        packed = np.concatenate([M, [w, h, 0, w * bpp], tail, lens])
        ragged = np.concatenate([M, [w, h, 0, w * bpp, w, h, 0, w * bpp, 0.0 if word is None else word], lens])
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
            rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), n, 1, 0, 0, 0, 1 | bit | LENS, behind, C.c_void_p(d_dst), n, 0, 0, 0)
            err = lib.lr_last_error().decode()
            assert rc != 0 and "LR_WARP_LENS" in err and name in err, (name, err)
        rc, err = call(1 | L.WARP_RAGGED | L.WARP_PREPARE | LENS, tables(good, 3)[2][1], 0, 0)
        assert rc != 0 and "LR_WARP_LENS" in err and "LR_WARP_PREPARE" in err
        assert untouched()
        # fx = 0, fy < 0, a NaN coefficient, an infinite cx (and the other entries' non-finite values)
        bad = []
        for i, v in ((0, 0.0), (0, -0.0), (1, -3.0), (6, float("nan")), (2, float("inf")), (0, float("inf")), (1, float("nan")),
                     (3, -float("inf")), (4, float("inf")), (5, float("nan")), (7, float("nan")), (8, -float("inf"))):
            lens = good.copy()
            lens[i] = v
            bad.append(lens)
        for lens in bad:
            for fmt in (0, 1, 2):
                for word in (None, 1.0):
                    for layout, table, srow, drow in tables(lens, BPP[fmt], word):
                        for rule in (0, CUBIC):
                            rc, err = call(fmt | layout | LENS | rule | (BORDER if word is not None else 0), table, srow, drow)
                            assert rc != 0, (lens, fmt, layout)
                            assert err.startswith("lr_warp_perspective_device") and "LR_WARP_LENS" in err and "frame 0" in err, err
        assert untouched()
        # the second frame's lens names the second frame
        two = np.concatenate([M, good, M, bad[0]])
        rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), w * h, 2, w, h, w, 0 | LENS, P(two), C.c_void_p(d_dst), w * h, w, h, w)
        assert rc != 0 and "frame 1" in lib.lr_last_error().decode()
        # what the call without the bit rejects, it rejects with it; unknown option bits stay unknown
        for layout, table, srow, drow in tables(good, 3):
            rc, err = call(3 | layout | LENS, table, srow, drow)
            assert rc != 0 and "unknown pixel format" in err
            nan_map = table.copy()
            nan_map[4] = np.nan
            rc, err = call(1 | layout | LENS, nan_map, srow, drow)
            assert rc != 0 and "not finite" in err
            for unknown in (0x400, 0x10000, 0x200000, 1 << 30):
                rc, err = call(1 | layout | unknown | LENS, table, srow, drow)
                assert rc != 0 and "unknown option" in err, (hex(unknown), layout, err)
        assert untouched()
        # and the next calls on the same context are right
        src = frame(1, w, h, 2)
        L._check(lib.lr_memcpy_h2d(ctx._h, C.c_void_p(d_src), P(src), src.nbytes))
        for layout, table, srow, drow in tables(good, 3):
            rc, err = call(1 | layout | LENS, table, srow, drow)
            assert rc == 0, err
            assert_same(ctx.device_download(d_dst, (h, w, 3), np.uint8), RL.warp(src, np.eye(3), w, h, good))
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


# ---- the Python level ----

def test_undistort_is_the_identity_warp_with_the_lens(L, ctx):
    for fmt in (0, 1, 2):
        src = source(fmt, 1)
        h, w = src.shape[:2]
        lens = L.Lens(*the_lenses(w, h)[1])
        for interp in ("linear", "cubic"):
            for spec, mode, value in border_specs(fmt)[:3]:
                got = ctx.undistort(src, lens, interp=interp, border=spec)
                assert got.shape == src.shape
                assert_same(got, ctx.warp_perspective(src, np.eye(3), (w, h), interp=interp, border=spec, lens=lens))
                assert_same(got, RL.warp(src, np.eye(3), w, h, lens, mode, value, interp == "cubic"))
    with pytest.raises(ValueError, match="warp_perspective"):
        ctx.undistort(src, L.Lens(0.0, 1.0, 0.0, 0.0))
    # the points that lens_distort names are where the undistorted picture was read: rint(32 d) are the reference's coordinates
    X, Y = RL.fixed_coords(np.eye(3), w, h, lens)
    d = L.lens_distort(lens, np.stack(np.meshgrid(np.arange(float(w)), np.arange(float(h))), axis=-1))
    assert np.array_equal(np.rint(d[..., 0] * 32).astype(np.int64), X) and np.array_equal(np.rint(d[..., 1] * 32).astype(np.int64), Y)


@pytest.fixture(scope="module")
def photograph():
    """the golden photograph's luma at half size"""
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    return np.ascontiguousarray(gray[::2, ::2])


def lens_of(img, k1=-0.12, k2=0.02):
    h, w = img.shape[:2]
    return (0.8 * max(w, h), 0.8 * max(w, h), (w - 1) / 2.0, (h - 1) / 2.0, k1, k2, 0.001, -0.0005, 0.0)


def test_rectify_with_a_lens_detects_on_the_undistorted_frame_and_warps_the_original(L, ctx, photograph):
    img = photograph
    lens = L.Lens(*lens_of(img))
    ideal = ctx.undistort(img, lens)
    assert (ideal != img).mean() > 0.3
    for kwargs in ({}, {"interp": "cubic", "border": "replicate"}, {"max_size": 300}):
        lines0, t0, _ = ctx.rectify(ideal, **{k: v for k, v in kwargs.items() if k == "max_size"})
        lines, t, warped = ctx.rectify(img, lens=lens, **kwargs)
        assert len(lines) > 10 and lines.tobytes() == lines0.tobytes()
        np.testing.assert_array_equal(t.as_array(), t0.as_array())
        _, M, size = L.rectification_homography(t, 3.0)
        np.testing.assert_array_equal(warped, ctx.warp_perspective(img, M, size, interp=kwargs.get("interp", "linear"), border=kwargs.get("border"), lens=lens))
        if not kwargs:
            np.testing.assert_array_equal(warped, RL.warp(img, M, size[0], size[1], lens))
    # a file goes the same way: decoded once, the lens refers to the decoded frame
    data = ctx.encode_jpeg(img, 95)
    decoded = ctx.decode_jpeg(data, L.PIX_U8)
    got = ctx.rectify(data, lens=lens)
    exp = ctx.rectify(decoded, lens=lens)
    assert got[0].tobytes() == exp[0].tobytes()
    np.testing.assert_array_equal(got[2], exp[2])
    assert ctx.rectify(img, lens=lens, jpeg=90)[2] == ctx.encode_jpeg(ctx.rectify(img, lens=lens)[2], 90)


def test_rectify_batch_with_lenses_is_a_loop_of_rectify(L, ctx, photograph):
    frames = [photograph, np.ascontiguousarray(photograph[::-1]), gray_of(synthetic_rgb(333, 250, 4))]  # (two shapes)
    lenses = [L.Lens(*lens_of(frames[0])), None, L.Lens(*lens_of(frames[2], 0.1, -0.03))]
    for kwargs in ({}, {"interp": "cubic", "border": "reflect"}, {"max_size": 300}):
        single = [ctx.rectify(f, lens=lens, **kwargs) for f, lens in zip(frames, lenses)]
        batch = ctx.rectify_batch(frames, lens=lenses, **kwargs)
        for got, exp in zip(batch, single):
            assert len(got) == len(exp) == 3
            assert got[0].tobytes() == exp[0].tobytes()
            np.testing.assert_array_equal(got[1].as_array(), exp[1].as_array())
            np.testing.assert_array_equal(got[2], exp[2])
    # (the frame whose lens is None is the frame of the call without lens=)
    np.testing.assert_array_equal(single[1][2], ctx.rectify(frames[1], **kwargs)[2])
    same = ctx.rectify_batch(np.stack(frames[:2]), lens=lenses[0])  # (one Lens serves every frame)
    for got, f in zip(same, frames[:2]):
        np.testing.assert_array_equal(got[2], ctx.rectify(f, lens=lenses[0])[2])
    with pytest.raises(ValueError, match="rectify_batch"):
        ctx.rectify_batch(frames, lens=lenses[:2])
    with pytest.raises(ValueError, match="rectify_batch"):
        ctx.rectify_batch(frames, lens=[lenses[0], None, lenses[0]._replace(fy=0.0)])


def test_crop_together_with_a_lens_raises(L, ctx, photograph):
    lens = L.Lens(*lens_of(photograph))
    with pytest.raises(ValueError, match="crop"):
        ctx.rectify(photograph, lens=lens, crop=True)
    with pytest.raises(ValueError, match="crop"):
        ctx.rectify_batch([photograph], lens=lens, crop=True)
    with pytest.raises(ValueError, match="rectify"):
        ctx.rectify(photograph, lens=[lens, lens])


def test_recipe_lens_writes_what_the_library_computes(L, ctx, tmp_path, photograph):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    img = photograph
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    lens = L.Lens(*lens_of(img))
    text = ",".join(repr(float(v)) for v in lens)
    for bad in (["--lens", text], ["--warp", "--crop", "--lens", text], ["--warp", "--lens", "1,2,3"], ["--warp", "--lens", text.replace(",", ";")],
                ["--warp", "--lens", "0," + text.split(",", 1)[1]], ["--warp", "--lens", text + ",1"], ["--warp", "--lens", "nan," + text.split(",", 1)[1]]):
        r = subprocess.run([exe, pgm, str(tmp_path / "none")] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and not os.path.exists(str(tmp_path / "none_lines.csv")), bad
    r = subprocess.run([exe, pgm, str(tmp_path / "a"), "--warp", "--lens", text], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "a_warp.pgm")), ctx.rectify(img, lens=lens)[2])
    r = subprocess.run([exe, pgm, str(tmp_path / "b"), "--warp", "--cubic", "--border", "reflect101", "--lens", text], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "b_warp.pgm")), ctx.rectify(img, lens=lens, interp="cubic", border="reflect101")[2])
