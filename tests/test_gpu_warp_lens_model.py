"""LR_WARP_LENS_MODEL on the GPU against its NumPy second source (tests/numpy_warp_lens_model_ref.py), byte for byte (f32: bit
for bit): both models, three pixel formats, the plain, the packed and the ragged launch; both sampling rules, border rules and
LR_WARP_AREA over the lens; a mixed ragged batch; the dispatch to the nine-entry kernels and to the plain ones; what is
refused; and LensModel, lens_scale= and --fisheye of the Python paths and of the recipe."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_border_ref as RB
import numpy_warp_lens_model_ref as RM
from test_gpu_rectify_warp import BPP, assert_same, frame, read_pnm, synthetic_rgb
from test_gpu_warp_border import SENTINEL, check_outputs, gray_of, lay_sources
from test_gpu_warp_cubic import six_frames
from test_gpu_warp_lens import OH, OW, SOURCES, border_specs, source, the_maps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CUBIC, BORDER, PACKED, RAGGED, LENS, AREA, MODEL = 0x8000, 0x40000, 0x200, 0x800, 0x100000, 0x400000, 0x800000


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


def the_models(w, h):
    """two lenses of model 0, one with all twelve coefficients and one whose denominator 1 + k4 r2 is exactly zero one pixel
    from the integer centre (a focal length of half a pixel: r2 = 4 there; infinities, and NaN from 0 * inf), and two fisheyes (the second with a focal length of a few pixels: most of the view folded into the
    picture, r far above 1)"""
    f, cx, cy = 0.6 * max(w, h), (w - 1) / 2.0, (h - 1) / 2.0
    return [
        (f, f, cx, cy, -0.3, 0.1, 0.01, -0.02, 0.02, 0.1, -0.05, 0.01, 0.003, -0.001, 0.002, 0.0005, 0.0),
        (0.5, 0.5, float(w // 2), float(h // 2), 0.0, 0.0, 0.0, 0.0, 0.0, -0.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
        (f, f, cx, cy, 0.05, -0.01, 0.005, -0.001) + (0.0,) * 8 + (1.0,),
        (3.0, 2.5, float(w // 2), float(h // 2), -0.02, 0.0, 0.0, 0.001) + (0.0,) * 8 + (1.0,),
    ]


_REF = {}


def ref(fmt, si, mi, lens, bi=0, cubic=False, area=None):
    """the second source's picture, computed once and shared by the layouts; lens: seventeen entries or None"""
    key = (fmt, si, mi, lens, bi, cubic, area)
    if key not in _REF:
        w, h = SOURCES[si]
        _, mode, value = border_specs(fmt)[bi]
        _REF[key] = RM.warp(source(fmt, si), the_maps(w, h)[mi], OW, OH, lens, mode, value, cubic, area)
        _REF[key].setflags(write=False)
    return _REF[key]


def launch(L, ctx, fmt, layout, opts, srcs, Ms, out_sizes, lenses, borders=None, areas=None):
    """One launch in the given layout (0 plain, PACKED, RAGGED) with tables from the package's builders, align=1 (f32: 4), so
    that rows and frames start at odd addresses; sources at odd offsets with padded rows.  lenses: a list per frame of Lens,
    LensModel or None, and the lens bits follow from the table's width; or None: a call without either lens bit.  Returns
    (destination bytes, places)."""
    bpp, step = BPP[fmt], 4 if fmt == 2 else 1
    n = len(srcs)
    sbuf, splaces = lay_sources(fmt, srcs, layout != RAGGED)
    w, h, soff, srow = splaces[0]
    simg = splaces[1][2] - soff if n > 1 else h * srow
    lead = 3 * step  # the frames start here in the region, and 16 bytes of sentinel follow the last
    ptable, total = L.warp_table(np.stack(Ms), np.array(out_sizes), bpp, align=step, border=borders, lens=lenses, area=areas)
    lens_cols = ptable.shape[1] - 13 - (1 if borders is not None else 0) - (1 if areas is not None else 0)
    assert lens_cols == (0 if lenses is None else lens_cols) and lens_cols in (0, 9, 17)
    bits = opts | (LENS if lens_cols else 0) | (MODEL if lens_cols == 17 else 0) | (BORDER if borders is not None else 0) | (AREA if areas is not None else 0)
    if layout == 0:
        ow, oh = out_sizes[0]
        drow = ow * bpp + 3 * step
        dimg = oh * drow + 5 * step
        places = [(ow, oh, lead + b * dimg, drow) for b in range(n)]
        region = lead + n * dimg + 16
        table = np.concatenate([ptable[:, :9], ptable[:, 13:]], axis=1)  # (the map, then what lies behind the packed row)
    elif layout == PACKED:
        table = ptable
        places = [tuple(int(v) for v in table[b, 9:13]) for b in range(n)]
        region = lead + total + 16
    else:
        table, total = L.ragged_table(np.stack(Ms), np.array(out_sizes), np.array(splaces), bpp, align=step, border=borders, lens=lenses, area=areas)
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
    frames = [(mi, li) for mi in range(3) for li in range(4)]  # every map with both lenses of both models
    groups = [[(si,) + f for f in frames] for si in range(2)] if layout != RAGGED else [[(si,) + f for si in range(2) for f in frames]]
    for group in groups:  # plain and packed: a launch per source size; ragged: both sources' frames in one launch
        srcs = [source(fmt, si) for si, _, _ in group]
        Ms = [the_maps(*SOURCES[si])[mi] for si, mi, _ in group]
        models = [the_models(*SOURCES[si])[li] for si, _, li in group]
        got, places = launch(L, ctx, fmt, layout, 0, srcs, Ms, [(OW, OH)] * len(group), [L.LensModel(*m) for m in models])
        check_outputs(got, fmt, places, [ref(fmt, si, mi, m) for (si, mi, _), m in zip(group, models)])


def test_the_models_change_the_pictures_and_the_odd_ones_are_odd():
    """(the comparisons above are not of equal pictures; the second lens of model 0 makes infinities and NaN inside the picture,
    the second fisheye has r far above 1)"""
    w, h = SOURCES[0]
    none = ref(0, 0, 0, None)
    assert all((ref(0, 0, 0, m) != none).mean() > 0.3 for m in the_models(w, h))
    U, V = RM.unrounded_coords(the_maps(w, h)[0], OW, OH, the_models(w, h)[1])
    assert np.isinf(U).any() and np.isnan(V).any() and np.isfinite(U).any()
    m = the_models(w, h)[3]
    r2 = ((np.arange(OW) - m[2]) / m[0]) ** 2
    assert r2.max() > 100.0 and (r2 < 1.0).any()  # (both branches of ATAN)


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_cubic_border_and_area_on_the_ragged_layout(L, ctx, fmt):
    specs = border_specs(fmt)
    for cubic in (False, True):
        for bi in (4, 1):  # reflect-101, the constant 200
            for area in (None, 2):
                group = [(si, (si + li) % 3, li) for si in range(2) for li in range(4)]
                srcs = [source(fmt, si) for si, _, _ in group]
                Ms = [the_maps(*SOURCES[si])[mi] for si, mi, _ in group]
                models = [the_models(*SOURCES[si])[li] for si, _, li in group]
                got, places = launch(L, ctx, fmt, RAGGED, CUBIC if cubic else 0, srcs, Ms, [(OW, OH)] * len(group), [L.LensModel(*m) for m in models],
                                     [specs[bi][0]] * len(group), None if area is None else [area] * len(group))
                check_outputs(got, fmt, places, [ref(fmt, si, mi, m, bi, cubic, area) for (si, mi, _), m in zip(group, models)])


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ragged_batch_of_six_mixed_frames(L, ctx, fmt):
    """no lens (a model-0 row of zeros), a model-0 lens that fits the nine entries, one with twelve coefficients, two different
    fisheyes and a None, in one launch"""
    frames, Ms, out_sizes = six_frames(fmt, False)
    lenses = []
    for b, f in enumerate(frames):
        h, w = f.shape[:2]
        m = the_models(w, h)
        lenses.append([L.LensModel(30.0, 30.0, 1.0, 2.0), L.Lens(*m[0][:9]), L.LensModel(*m[0]), L.LensModel(*m[2]), L.LensModel.fisheye(*m[3][:8]), None][b])
    seventeen = [None if v is None else tuple(v) + (0.0,) * (17 - len(v)) for v in lenses]
    for cubic in (False, True):
        got, places = launch(L, ctx, fmt, RAGGED, CUBIC if cubic else 0, frames, Ms, out_sizes, lenses)
        check_outputs(got, fmt, places, [RM.warp(f, M, size[0], size[1], lens, cubic=cubic) for f, M, size, lens in zip(frames, Ms, out_sizes, seventeen)])
        interp = "cubic" if cubic else "linear"
        for b in (0, 5):  # (the frames without a lens are the frames of the call without the bits)
            assert_same(RM.warp(frames[b], Ms[b], out_sizes[b][0], out_sizes[b][1], None, cubic=cubic), ctx.warp_perspective(frames[b], Ms[b], out_sizes[b], interp=interp))
        for b in (1, 3):  # (and the single-frame path gives the same frames)
            assert_same(ctx.warp_perspective(frames[b], Ms[b], out_sizes[b], interp=interp, lens=lenses[b]),
                        RM.warp(frames[b], Ms[b], out_sizes[b][0], out_sizes[b][1], seventeen[b], cubic=cubic))


@pytest.mark.parametrize("layout", [0, PACKED, RAGGED], ids=["plain", "packed", "ragged"])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_rows_that_fit_nine_entries_and_rows_of_zeros(L, ctx, fmt, layout):
    """a call with the bit whose rows all fit the nine entries gives the bytes of the same call with LR_WARP_LENS alone; rows of
    zeros give the call without either bit"""
    si = 0
    w, h = SOURCES[si]
    n = 3
    Ms = the_maps(w, h)
    f = 0.6 * max(w, h)
    nine = [L.Lens(f, f, w / 2.0, h / 2.0, -0.3, 0.1), None, L.Lens(f, 1.1 * f, w / 2.0 + 1.5, h / 2.0, 0.25, 0.05, 0.01, -0.02, 0.02)]
    as_models = [None if v is None else L.LensModel(*(tuple(v) + (-0.0, 0.0) * 4)[:17]) for v in nine]
    zeros = [L.LensModel(40.0, 41.0, 3.0, 5.0), None, L.LensModel(*((1e-3, 1e6, -7.0, 1e9) + (-0.0, 0.0) * 6 + (0.0,)))]
    srcs = [source(fmt, si)] * n
    for cubic in (False, True):
        opts = CUBIC if cubic else 0
        for borders, areas in ((None, None), ([None, "reflect", ("constant", border_specs(fmt)[1][0][1])], None), (None, [2, 1, 3])):
            with_lens, places = launch(L, ctx, fmt, layout, opts, srcs, Ms, [(OW, OH)] * n, nine, borders, areas)
            with_model, places_m = launch(L, ctx, fmt, layout, opts, srcs, Ms, [(OW, OH)] * n, as_models, borders, areas)
            assert places == places_m and with_lens.tobytes() == with_model.tobytes()
            assert (with_lens != SENTINEL).any()
            no_lens, places_n = launch(L, ctx, fmt, layout, opts, srcs, Ms, [(OW, OH)] * n, None, borders, areas)
            of_zeros, places_z = launch(L, ctx, fmt, layout, opts, srcs, Ms, [(OW, OH)] * n, zeros, borders, areas)
            assert places_n == places_z and no_lens.tobytes() == of_zeros.tobytes() and no_lens.tobytes() != with_lens.tobytes()
            if borders is None and areas is None:
                check_outputs(of_zeros, fmt, places_z, [ref(fmt, si, mi, None, 0, cubic) for mi in range(3)])


def test_refusals_leave_the_destination_as_it_was(L, ctx):
    lib = L.lib()
    w, h = 64, 48
    n = w * h * 4
    d_src = ctx.device_upload(np.zeros(n, np.uint8))
    d_dst = ctx.device_upload(np.full(n, SENTINEL, np.uint8))
    M = np.eye(3).reshape(-1)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = L.JpegArgs()  # (never read: the combination is refused first)
    good = np.array([50.0, 50.0, 31.5, 23.5, -0.2, 0.05, 0.001, -0.001, 0.0, 0.01, 0.0, 0.002, 0.0, 0.001, 0.0, 0.0, 0.0])
    fish = np.array([50.0, 50.0, 31.5, 23.5, 0.05, 0.01, 0.0, 0.001] + [0.0] * 8 + [1.0])

    def tables(lens, bpp, word=None, area=None):
        """the same frame in the three layouts, the lens entries at the end of its row (behind the border word, if any)"""
        tail = np.concatenate([[] if word is None else [word], lens, [] if area is None else [area]])
        plain = np.concatenate([M, tail])
        packed = np.concatenate([M, [w, h, 0, w * bpp], tail])
        ragged = np.concatenate([M, [w, h, 0, w * bpp, w, h, 0, w * bpp, 0.0 if word is None else word], tail[(0 if word is None else 1):]])
        return [(0, plain, w * bpp, w * bpp), (PACKED, packed, w * bpp, 0), (RAGGED, ragged, 0, 0)]

    def call(fmt_word, table, srow, drow):
        rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), n, 1, w, h, srow, fmt_word, P(table), C.c_void_p(d_dst), n, w, h, drow)
        return rc, lib.lr_last_error().decode()

    untouched = lambda: (ctx.device_download(d_dst, (n,), np.uint8) == SENTINEL).all()  # noqa: E731
    try:
        # the bit together with the calls that are no warp, and without LR_WARP_LENS
        behind = C.cast(C.byref(args), C.c_void_p)
        for name, bit in (("LR_WARP_PREPARE", L.WARP_PREPARE), ("LR_WARP_LINES", L.WARP_LINES), ("LR_WARP_JPEG", L.WARP_JPEG),
                          ("LR_WARP_JPEG_DECODE", L.WARP_JPEG_DECODE)):
            for lens_bit in (LENS, 0):
                rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), n, 1, 0, 0, 0, 1 | bit | lens_bit | MODEL, behind, C.c_void_p(d_dst), n, 0, 0, 0)
                err = lib.lr_last_error().decode()
                assert rc != 0 and "LR_WARP_LENS_MODEL" in err and name in err, (name, err)
        for layout, table, srow, drow in tables(good, 3):
            rc, err = call(1 | layout | MODEL, table, srow, drow)
            assert rc != 0 and "LR_WARP_LENS_MODEL without LR_WARP_LENS" in err, err
        assert untouched()
        # entry by entry: non-finite values, fx and fy, the model, a fisheye's entries [8..15]
        bad = []
        for base, i, v in [(good, 0, 0.0), (good, 0, -0.0), (good, 1, -3.0), (fish, 0, -1.0), (good, 16, 2.0), (good, 16, -1.0), (good, 16, 0.5), (fish, 16, 1.5),
                           (good, 16, float("nan")), (fish, 16, float("inf"))] + [(good, i, float("nan")) for i in range(16)] + \
                          [(fish, i, -float("inf")) for i in (2, 7, 9, 15)] + [(fish, i, 1e-300) for i in range(8, 16)] + [(fish, 12, -0.5)]:
            lens = base.copy()
            lens[i] = v
            bad.append(lens)
        for k, lens in enumerate(bad):
            for fmt in (0, 1, 2):
                for word, area in ((None, None), (1.0, None), (None, 2.0), (4.0, 3.0)):
                    for layout, table, srow, drow in tables(lens, BPP[fmt], word, area):
                        rule = CUBIC if (k + fmt) % 2 else 0
                        rc, err = call(fmt | layout | LENS | MODEL | rule | (BORDER if word is not None else 0) | (AREA if area is not None else 0), table, srow, drow)
                        assert rc != 0, (lens, fmt, layout)
                        assert err.startswith("lr_warp_perspective_device") and "LR_WARP_LENS_MODEL" in err and "frame 0" in err and "seventeen" in err, err
        assert untouched()
        # the second frame's lens names the second frame
        two = np.concatenate([M, good, M, bad[0]])
        rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), w * h, 2, w, h, w, 0 | LENS | MODEL, P(two), C.c_void_p(d_dst), w * h, w, h, w)
        assert rc != 0 and "frame 1" in lib.lr_last_error().decode()
        # what the call without the bit rejects, it rejects with it; unknown option bits stay unknown
        for layout, table, srow, drow in tables(good, 3):
            rc, err = call(3 | layout | LENS | MODEL, table, srow, drow)
            assert rc != 0 and "unknown pixel format" in err
            nan_map = table.copy()
            nan_map[4] = np.nan
            rc, err = call(1 | layout | LENS | MODEL, nan_map, srow, drow)
            assert rc != 0 and "not finite" in err
            for unknown in (0x400, 0x10000, 0x200000, 0x1000000, 1 << 30):
                rc, err = call(1 | layout | unknown | LENS | MODEL, table, srow, drow)
                assert rc != 0 and "unknown option" in err, (hex(unknown), layout, err)
        assert untouched()
        # and the next calls on the same context are right
        src = frame(1, w, h, 2)
        L._check(lib.lr_memcpy_h2d(ctx._h, C.c_void_p(d_src), P(src), src.nbytes))
        for lens in (good, fish):
            for layout, table, srow, drow in tables(lens, 3):
                rc, err = call(1 | layout | LENS | MODEL, table, srow, drow)
                assert rc == 0, err
                assert_same(ctx.device_download(d_dst, (h, w, 3), np.uint8), RM.warp(src, np.eye(3), w, h, tuple(lens)))
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


# ---- the Python level ----

def test_python_refusals(L, ctx):
    img = source(0, 0)
    fish = L.LensModel.fisheye(40.0, 40.0, 33.0, 17.0, 0.05)
    with pytest.raises(ValueError, match="warp_perspective"):
        ctx.undistort(img, fish._replace(k3=0.1))
    with pytest.raises(ValueError, match="warp_perspective"):
        ctx.warp_perspective(img, np.eye(3), (8, 8), lens=fish._replace(model=3))
    for s in (0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lens_scale"):
            ctx.undistort(img, fish, lens_scale=s)
        with pytest.raises(ValueError, match="lens_scale"):
            ctx.rectify(img, lens=fish, lens_scale=s)
        with pytest.raises(ValueError, match="lens_scale"):
            ctx.rectify_batch([img], lens=fish, lens_scale=s)
    with pytest.raises(ValueError, match="lens_scale"):
        ctx.rectify(img, lens_scale=0.5)
    with pytest.raises(ValueError, match="lens_scale"):
        ctx.rectify_batch([img], lens_scale=0.5)
    with pytest.raises(ValueError, match="crop"):
        ctx.rectify(img, lens=fish, crop=True)
    with pytest.raises(ValueError, match="crop"):
        ctx.rectify_batch([img], lens=[fish], crop=True)
    with pytest.raises(ValueError, match=r"rectify_batch.*frame 1"):
        ctx.rectify_batch([img, img], lens=[fish, fish._replace(s1=1.0)])


def straight_edges(w, h):
    """a pattern of straight edges: bars of 7 pixels, upright and slanted"""
    y, x = np.mgrid[0:h, 0:w]
    return (((x // 7) % 2) * 120 + (((x + 2 * y) // 9) % 2) * 100 + 20).astype(np.uint8)


def test_undistort_with_lens_scale(L, ctx):
    w, h = 70, 45
    fish = L.LensModel.fisheye(0.5 * w, 0.5 * w, (w - 1) / 2.0, (h - 1) / 2.0, 0.05, -0.01, 0.005, -0.001)
    # the pattern as this fisheye's rule shows it: what stands in the ideal picture at p is read at distort(p)
    stored = RM.warp(straight_edges(w, h), np.eye(3), w, h, tuple(fish))
    assert (stored != straight_edges(w, h)).mean() > 0.2
    outs = {}
    for s in (0.5, 1):
        S = L.lens_scale_map(fish, s)
        q = 1.0 / s
        np.testing.assert_array_equal(S, [[q, 0.0, fish.cx * (1.0 - q)], [0.0, q, fish.cy * (1.0 - q)], [0.0, 0.0, 1.0]])
        for interp in ("linear", "cubic"):
            for spec, mode, value in border_specs(0)[:3]:
                got = ctx.undistort(stored, fish, interp=interp, border=spec, lens_scale=s)
                assert got.shape == stored.shape
                assert_same(got, RM.warp(stored, S, w, h, tuple(fish), mode, value, interp == "cubic"))
        outs[s] = ctx.undistort(stored, fish, lens_scale=s)
        rgb = np.stack([stored, 255 - stored, stored // 2], axis=-1)
        assert_same(ctx.undistort(rgb, fish, lens_scale=s), RM.warp(rgb, S, w, h, tuple(fish)))
    assert_same(outs[1], ctx.undistort(stored, fish))
    assert (outs[0.5] != outs[1]).mean() > 0.2
    # a nine-entry Lens takes lens_scale as well
    nine = L.Lens(0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0, -0.2, 0.05)
    assert_same(ctx.undistort(stored, nine, lens_scale=0.5), ctx.warp_perspective(stored, L.lens_scale_map(nine, 0.5), (w, h), lens=nine))
    # the points that lens_distort names are where the undistorted picture was read
    X, Y = RM.fixed_coords(np.eye(3), w, h, tuple(fish))
    d = L.lens_distort(fish, np.stack(np.meshgrid(np.arange(float(w)), np.arange(float(h))), axis=-1))
    assert np.array_equal(np.rint(d[..., 0] * 32).astype(np.int64), X) and np.array_equal(np.rint(d[..., 1] * 32).astype(np.int64), Y)


@pytest.fixture(scope="module")
def photograph():
    """the golden photograph's luma at half size"""
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    return np.ascontiguousarray(gray[::2, ::2])


def fisheye_of(img, k1=0.03, k2=-0.005):
    h, w = img.shape[:2]
    return (1.5 * max(w, h), 1.5 * max(w, h), (w - 1) / 2.0, (h - 1) / 2.0, k1, k2, 0.001, -0.0005)


def compose(S, M):
    """lens_scale_map @ M with every product and sum rounded on its own (the zeros of S add nothing)"""
    return np.stack([S[0, 0] * M[0] + S[0, 2] * M[2], S[1, 1] * M[1] + S[1, 2] * M[2], M[2]])


def test_rectify_with_a_fisheye_and_lens_scale_is_the_hand_made_sequence(L, ctx, photograph):
    img = photograph
    lens = L.LensModel.fisheye(*fisheye_of(img))
    for s, kwargs in ((0.6, {}), (0.6, {"interp": "cubic", "border": "replicate"}), (1, {"max_size": 300}), (1.25, {"out_max_size": 200})):
        ideal = ctx.undistort(img, lens, lens_scale=s)
        assert (ideal != img).mean() > 0.3
        lines0, t0, _ = ctx.rectify(ideal, **{k: v for k, v in kwargs.items() if k == "max_size"})
        lines, t, warped = ctx.rectify(img, lens=lens, lens_scale=s, **kwargs)
        assert len(lines) > 10 and lines.tobytes() == lines0.tobytes()
        np.testing.assert_array_equal(t.as_array(), t0.as_array())
        _, M, size = L.rectification_homography(t, 3.0)
        area = None
        if "out_max_size" in kwargs:
            _, M, size, area = L.shrink_homography(None, M, size, kwargs["out_max_size"])
        M = compose(L.lens_scale_map(lens, s), np.asarray(M, np.float64).reshape(3, 3))
        np.testing.assert_array_equal(warped, ctx.warp_perspective(img, M, size, interp=kwargs.get("interp", "linear"), border=kwargs.get("border"), lens=lens, area=area))
        if not kwargs:
            np.testing.assert_array_equal(warped, RM.warp(img, M, size[0], size[1], tuple(lens)))
    # a file goes the same way: decoded once, the lens refers to the decoded frame
    data = ctx.encode_jpeg(img, 95)
    decoded = ctx.decode_jpeg(data, L.PIX_U8)
    got = ctx.rectify(data, lens=lens, lens_scale=0.6)
    exp = ctx.rectify(decoded, lens=lens, lens_scale=0.6)
    assert got[0].tobytes() == exp[0].tobytes()
    np.testing.assert_array_equal(got[2], exp[2])


def test_rectify_batch_with_mixed_lens_types_is_a_loop_of_rectify(L, ctx, photograph):
    frames = [photograph, np.ascontiguousarray(photograph[::-1]), gray_of(synthetic_rgb(333, 250, 4)), np.ascontiguousarray(photograph[:, ::-1])]  # (two shapes)
    h, w = photograph.shape
    nine = L.Lens(0.8 * max(w, h), 0.8 * max(w, h), (w - 1) / 2.0, (h - 1) / 2.0, -0.12, 0.02, 0.001, -0.0005)
    full = L.LensModel(*(tuple(nine) + (0.01, -0.002, 0.0003, 0.0005, 0.0, -0.0004, 0.0001)))
    lenses = [nine, None, L.LensModel.fisheye(*fisheye_of(frames[2], 0.02, 0.001)), full]
    for kwargs in ({}, {"interp": "cubic", "border": "reflect", "lens_scale": 0.8}, {"max_size": 300}):
        single = [ctx.rectify(f, lens=lens, **{k: v for k, v in kwargs.items() if k != "lens_scale" or lens is not None}) for f, lens in zip(frames, lenses)]
        batch = ctx.rectify_batch(frames, lens=lenses, **kwargs)
        for got, exp in zip(batch, single):
            assert len(got) == len(exp) == 3
            assert got[0].tobytes() == exp[0].tobytes()
            np.testing.assert_array_equal(got[1].as_array(), exp[1].as_array())
            np.testing.assert_array_equal(got[2], exp[2])
    # (the frame whose lens is None is the frame of the call without lens=; a Lens in the mixed list is the Lens alone)
    np.testing.assert_array_equal(single[1][2], ctx.rectify(frames[1], max_size=300)[2])
    np.testing.assert_array_equal(single[0][2], ctx.rectify_batch([frames[0]], lens=[nine], max_size=300)[0][2])
    same = ctx.rectify_batch(np.stack(frames[:2]), lens=lenses[3])  # (one LensModel serves every frame)
    for got, f in zip(same, frames[:2]):
        np.testing.assert_array_equal(got[2], ctx.rectify(f, lens=lenses[3])[2])


def test_recipe_fisheye_writes_what_the_library_computes(L, ctx, tmp_path, photograph):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    img = photograph
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    eight = fisheye_of(img)
    lens = L.LensModel.fisheye(*eight)
    text = ",".join(repr(float(v)) for v in eight)
    text17 = ",".join(repr(float(v)) for v in lens)
    h, w = img.shape
    full = L.LensModel(0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0, -0.12, 0.02, 0.001, -0.0005, 0.0, 0.01, -0.002, 0.0003, 0.0005, 0.0, -0.0004, 0.0001)
    for bad in (["--fisheye", text], ["--warp", "--crop", "--fisheye", text], ["--warp", "--fisheye", text + ",0"], ["--warp", "--fisheye", "0," + text.split(",", 1)[1]],
                ["--warp", "--fisheye", text17], ["--warp", "--lens", text17 + ",0"], ["--warp", "--lens", text17[:-3] + "2.0"], ["--warp", "--lens", text17.replace(",0.0,1.0", ",0.5,1.0")],
                ["--warp", "--lens-scale", "0.5"], ["--warp", "--fisheye", text, "--lens-scale", "0"], ["--warp", "--fisheye", text, "--lens-scale", "nan"]):
        r = subprocess.run([exe, pgm, str(tmp_path / "none")] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and not os.path.exists(str(tmp_path / "none_lines.csv")), bad
    r = subprocess.run([exe, pgm, str(tmp_path / "a"), "--warp", "--fisheye", text], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "a_warp.pgm")), ctx.rectify(img, lens=lens)[2])
    r = subprocess.run([exe, pgm, str(tmp_path / "b"), "--warp", "--cubic", "--border", "reflect101", "--lens", text17, "--lens-scale", "0.6"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "b_warp.pgm")), ctx.rectify(img, lens=lens, lens_scale=0.6, interp="cubic", border="reflect101")[2])
    r = subprocess.run([exe, pgm, str(tmp_path / "c"), "--warp", "--lens", ",".join(repr(float(v)) for v in full), "--out-max", "200"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_pnm(str(tmp_path / "c_warp.pgm")), ctx.rectify(img, lens=full, out_max_size=200)[2])
