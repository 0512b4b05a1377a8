"""Mixed-size batches: lr_warp_perspective_device with LR_WARP_RAGGED (the warp and the prepare step on frames that each
have their own source size and place) against tests/numpy_warp_ref.py, tests/numpy_prepare_ref.py and the single-frame
launches, bit for bit; their clean failures; the batch detector with a frame table against the single-frame call; and
Context.rectify_batch on a list of frames of different shapes against a loop of Context.rectify."""
import ctypes as C

import numpy as np
import pytest

import numpy_prepare_ref as PR
import numpy_warp_ref as R
from test_gpu_rectify_batch import EDGE_BATCHES, EDGE_KINDS, EDGE_SIZES, KINDS, SENTINEL, SETTINGS, SIZES, _kw, cut, gray_frame, edge_table, same_results, seven_frames_table, written_mask
from test_gpu_rectify_warp import BPP, DTYPE, assert_same, frame, maps, synthetic_rgb

pytestmark = pytest.mark.gpu

PREFIX = "lr_warp_perspective_device: "


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


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def source_region(frames, fmt, whole_pixels=False, odd_stride=True):
    """The frames in one region, one after the other, with padded rows, gaps and (8-bit) odd offsets and strides
    (whole_pixels: strides that the detector takes, too; odd_stride=False: a list too short to hold an odd stride for
    sure).  Returns (the region's bytes, [(width, height, byte_offset, row_bytes)])."""
    bpp = BPP[fmt]
    cursor = 8 if fmt == 2 else 5
    sources = []
    for k, f in enumerate(frames):
        h, w = f.shape[:2]
        row = w * bpp + ((4, 12, 0)[k % 3] if fmt == 2 else (1, 4, 0, 7)[k % 4])
        if whole_pixels:
            row = (w + (1, 4, 0, 7)[k % 4]) * bpp
        sources.append((w, h, cursor, row))
        cursor += (h - 1) * row + w * bpp + ((4, 0, 20)[k % 3] if fmt == 2 else (3, 0, 10)[k % 3])
    buf = np.full(cursor + (4 if fmt == 2 else 9), 0x5A, np.uint8)
    for f, (w, h, off, row) in zip(frames, sources):
        rows = np.lib.stride_tricks.as_strided(buf[off:], (h, w * bpp), (row, 1))
        rows[:] = np.ascontiguousarray(f).reshape(h, -1).view(np.uint8)
    if fmt != 2:
        assert any(s[2] % 2 for s in sources) and (whole_pixels or not odd_stride or any(s[3] % 2 for s in sources))
    return buf, sources


# ---- the ragged warp ---------------------------------------------------------------------------------------------

SRC_SIZES = [(257, 131), (64, 16), (65, 17), (5, 7), (1, 1), (130, 40)]  # and the first once more, with another map


def seven_ragged_frames(fmt):
    """Seven frames on six sources (the seventh reads the first's), with the output sizes, map kinds and out-of-order
    places of seven_frames_table.  Returns (frames per table row, region bytes, table, destination bytes)."""
    srcs = [frame(fmt, w, h, 200 + k) for k, (w, h) in enumerate(SRC_SIZES)]
    buf, sources = source_region(srcs, fmt)
    srcs.append(srcs[0])
    sources.append(sources[0])
    packed, region = seven_frames_table(fmt)
    table = np.zeros((7, 18))
    table[:, 9:13] = packed[:, 9:]
    for b, (w, h, _, _) in enumerate(sources):
        table[b, :9] = maps(w, h, *SIZES[b])[KINDS[b]].reshape(-1)
    table[:, 13:17] = sources
    assert not np.array_equal(table[0, :9], table[6, :9])
    assert (np.diff(table[:, 11]) < 0).any(), "the outputs are placed out of frame order"
    return srcs, buf, table, region


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ragged_warp_bit_exact_and_writes_nothing_else(L, ctx, fmt):
    srcs, buf, table, region = seven_ragged_frames(fmt)
    bpp = BPP[fmt]
    d_src = ctx.device_upload(buf)
    d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    singles = []
    try:
        ctx.warp_perspective_ragged_device(d_src, len(buf), fmt, table, d_dst, region)
        got = ctx.device_download(d_dst, (region,), np.uint8)
        for b in range(7):  # the single-frame launch on the frame's own source
            ow, oh = SIZES[b]
            w, h, off, row = (int(v) for v in table[b, 13:17])
            d_one = ctx.device_upload(np.zeros(ow * oh * bpp, np.uint8))
            try:
                ctx.warp_perspective_device(d_src + off, 0, 1, w, h, row, fmt, table[b, :9].copy(), d_one, ow * oh * bpp, ow, oh, ow * bpp)
                singles.append(ctx.device_download(d_one, (oh, ow * bpp), np.uint8))
            finally:
                ctx.device_free(d_one)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    mask = written_mask(region, table[:, :13], bpp)
    assert (got[~mask] == SENTINEL).all(), "bytes outside the frames' pixel rows were written"
    for b in range(7):
        ow, oh = SIZES[b]
        out = cut(got, table[b, :13], fmt)
        assert_same(out, R.warp(srcs[b], table[b, :9], ow, oh)), KINDS[b]
        assert_same(out, np.ascontiguousarray(singles[b]).view(DTYPE[fmt]).reshape(out.shape))
    assert_same(cut(got, table[0, :13], fmt), srcs[0][:1, :1])  # (identity)


@pytest.mark.parametrize("which", EDGE_BATCHES)
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ragged_warp_of_a_few_tiles(L, ctx, fmt, which):
    """EDGE_SIZES (six tiles in all: some XCDs' runs are empty), every frame from a source of its own size"""
    srcs = [frame(fmt, *[(70, 20), (5, 7), (64, 16)][s], 200 + s) for s in which]
    buf, sources = source_region(srcs, fmt, odd_stride=len(which) > 1)
    packed, region = edge_table(fmt, which)
    table = np.zeros((len(which), 18))
    table[:, 9:13] = packed[:, 9:]
    for k, s in enumerate(which):
        table[k, :9] = maps(*sources[k][:2], *EDGE_SIZES[s])[EDGE_KINDS[s]].reshape(-1)
        table[k, 13:17] = sources[k]
    d_src = ctx.device_upload(buf)
    d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    try:
        ctx.warp_perspective_ragged_device(d_src, len(buf), fmt, table, d_dst, region)
        got = ctx.device_download(d_dst, (region,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    assert (got[~written_mask(region, table[:, :13], BPP[fmt])] == SENTINEL).all(), "bytes outside the frames' pixel rows were written"
    for k, s in enumerate(which):
        assert_same(cut(got, table[k, :13], fmt), R.warp(srcs[k], table[k, :9], *EDGE_SIZES[s])), EDGE_KINDS[s]


# ---- the ragged prepare step -------------------------------------------------------------------------------------

PREPARE_SIZES = [  # source width, height -> output width, height
    (120, 80, 120, 80),    # pure conversion
    (257, 131, 100, 51),   # non-integral scale
    (1300, 40, 100, 4),    # more than 512 source columns under one tile
    (40, 1300, 3, 100),    # portrait, 13 source rows per destination row
    (9, 9, 1, 1),
    (300, 200, 299, 199),  # scale just above 1
    (70, 70, 64, 64),
]


def prepare_table(sources):
    """f32 outputs placed out of frame order, with gaps and padded rows (all multiples of 4); NaN in the map columns"""
    table = np.full((len(sources), 18), np.nan)
    cursor = 8
    for k, b in enumerate([4, 0, 6, 2, 5, 1, 3]):
        ow, oh = PREPARE_SIZES[b][2:]
        row = ow * 4 + (4, 12, 0)[k % 3]
        table[b, 9:13] = (ow, oh, cursor, row)
        cursor += (oh - 1) * row + ow * 4 + (4, 0, 20)[k % 3]
    table[:, 13:17] = sources
    table[:, 17] = 0
    return table, cursor + 12


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ragged_prepare_bit_exact_and_writes_nothing_else(L, ctx, fmt):
    srcs = [frame(fmt, w, h, 300 + k) for k, (w, h, _, _) in enumerate(PREPARE_SIZES)]
    buf, sources = source_region(srcs, fmt)
    table, region = prepare_table(sources)
    d_src = ctx.device_upload(buf)
    d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    singles = []
    try:
        ctx.prepare_ragged_device(d_src, len(buf), fmt, table, d_dst, region)
        got = ctx.device_download(d_dst, (region,), np.uint8)
        for b, (w, h, ow, oh) in enumerate(PREPARE_SIZES):  # the single-frame LR_WARP_PREPARE call
            d_one = ctx.device_upload(np.zeros(ow * oh * 4, np.uint8))
            try:
                ctx.prepare_device(d_src + sources[b][2], 0, 1, w, h, sources[b][3], fmt, d_one, ow * oh * 4, ow, oh, ow * 4)
                singles.append(ctx.device_download(d_one, (oh, ow), np.float32))
            finally:
                ctx.device_free(d_one)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    mask = written_mask(region, table[:, :13], 4)
    assert (got[~mask] == SENTINEL).all(), "bytes outside the frames' pixel rows were written"
    for b, (w, h, ow, oh) in enumerate(PREPARE_SIZES):
        out = cut(got, table[b, :13], 2)
        assert_same(out, PR.prepare(srcs[b], ow, oh))
        assert_same(out, singles[b])
    if fmt != 2:  # the pure conversion is exactly luma / 256
        c = srcs[0].astype(np.int64)
        lum = c if fmt == 0 else (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
        assert_same(cut(got, table[0, :13], 2), lum.astype(np.float32) / np.float32(256))


EDGE_PREPARE = [  # source width, height -> output width, height
    (130, 10, 65, 5),   # a partial tile in both directions
    (1100, 20, 2, 2),   # a pixel's 550 column taps cross the 512-pixel chunk, its 10 row taps the 8-row chunk
    (1, 1, 1, 1),
]


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ragged_prepare_edge_shapes(L, ctx, fmt):
    srcs = [frame(fmt, w, h, 400 + k) for k, (w, h, _, _) in enumerate(EDGE_PREPARE)]
    buf, sources = source_region(srcs, fmt)
    if fmt == 1:
        assert all(s[2] % 2 for s in sources[:2]), "u8x3 sources whose first byte is at an odd offset"
    table = np.full((3, 18), np.nan)
    cursor = 8
    for b in (2, 0, 1):  # placed out of frame order, with gaps and padded rows
        ow, oh = EDGE_PREPARE[b][2:]
        row = ow * 4 + 4 * b
        table[b, 9:13] = (ow, oh, cursor, row)
        cursor += (oh - 1) * row + ow * 4 + 12
    table[:, 13:17] = sources
    table[:, 17] = 0
    region = cursor + 12
    d_src = ctx.device_upload(buf)
    d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    try:
        ctx.prepare_ragged_device(d_src, len(buf), fmt, table, d_dst, region)
        got = ctx.device_download(d_dst, (region,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    assert (got[~written_mask(region, table[:, :13], 4)] == SENTINEL).all(), "bytes outside the frames' pixel rows were written"
    for b, (w, h, ow, oh) in enumerate(EDGE_PREPARE):
        assert_same(cut(got, table[b, :13], 2), PR.prepare(srcs[b], ow, oh))


# ---- failures are clean ------------------------------------------------------------------------------------------

def test_ragged_failures_are_clean(L, ctx):
    lib = L.lib()
    srcs = [frame(1, w, h, 400 + k) for k, (w, h) in enumerate([(64, 48), (33, 50), (80, 20)])]
    buf, sources = source_region(srcs, 1)
    sizes = [(70, 20), (9, 33), (64, 48)]
    Ms = np.stack([maps(s[0], s[1], ow, oh)[k] for s, (ow, oh), k in zip(sources, sizes, ("shift", "rotation", "identity"))])
    good, total = L.ragged_table(Ms, sizes, sources, 3, align=1)
    src_end = max(off + (h - 1) * row + w * 3 for w, h, off, row in sources)
    region = 1 << 16
    assert total + 100 < region
    d_src = ctx.device_upload(buf)
    d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    fmt = L.PIX_U8X3 | L.WARP_RAGGED
    # the same source bytes read as f32 frames (16 x 20, 8 x 30, 16 x 10 at offsets and strides that are multiples of 4)
    f32_src = [(16, 20, 8, 64), (8, 30, 4000, 32), (16, 10, 6000, 64)]
    assert max(o + (h - 1) * r + 4 * w for w, h, o, r in f32_src) <= len(buf)
    f32, f32_total = L.ragged_table(np.stack([np.eye(3)] * 3), [(16, 20), (9, 33), (16, 10)], f32_src, 4)
    f32_call = dict(fmt=L.PIX_F32 | L.WARP_RAGGED, table=f32)
    # the prepare step on the u8x3 sources
    prep, prep_total = L.ragged_table(None, [(32, 24), (33, 50), (8, 2)], sources, 3, out_bpp=4)
    prep[:, :9] = np.nan
    prep_call = dict(fmt=fmt | L.WARP_PREPARE, table=prep)
    assert max(f32_total, prep_total) <= region

    def call(table=good, fmt=fmt, dst=None, dst_bytes=region, src=None, src_bytes=len(buf), sw=80, sh=50, ow=70, oh=50, srow=0, drow=0):
        t = np.ascontiguousarray(table, np.float64)
        return lib.lr_warp_perspective_device(ctx._h, C.c_void_p(src or d_src), src_bytes, len(t), sw, sh, srow, fmt, P(t),
                                              C.c_void_p(dst or d_dst), dst_bytes, ow, oh, drow)

    def changed(k, v, b=1, base=good):
        t = base.copy()
        t[b, k] = v
        return t

    overlap = good.copy()
    overlap[1, 11] = good[0, 11] + good[0, 12] * 3  # inside frame 0's rows
    many = np.zeros((17, 18))
    many[:, :9] = np.eye(3).reshape(-1)
    many[:, 9], many[:, 10], many[:, 12] = 1, 2**31 - 1, 1
    many[:, 11] = np.arange(17) * 2.0**31
    many[:, 13:17] = (8, 8, 0, 24)
    cases = {
        "ragged and packed": dict(fmt=fmt | L.WARP_PACKED),
        "ragged, packed and prepare": dict(fmt=fmt | L.WARP_PACKED | L.WARP_PREPARE),
        "another option bit": dict(fmt=fmt | 0x400),
        "a high option bit": dict(fmt=fmt | 0x10000),
        "entry 17 not 0": dict(table=changed(17, 1)),
        "entry 17 NaN": dict(table=changed(17, np.nan)),
        "output width not integral": dict(table=changed(9, 8.5)),
        "source height 0": dict(table=changed(14, 0)),
        "source width above the bound": dict(sw=79),
        "output height above the bound": dict(oh=47),
        "source offset negative": dict(table=changed(15, -1)),
        "source stride infinite": dict(table=changed(16, np.inf)),
        "source stride shorter than a row": dict(table=changed(16, 33 * 3 - 1)),
        "output stride NaN": dict(table=changed(12, np.nan)),
        "source outside the region": dict(src_bytes=src_end - 1),
        "output outside the region": dict(dst_bytes=total - 1),
        "outputs overlap": dict(table=overlap),
        "map NaN": dict(table=changed(4, np.nan)),
        "map infinite": dict(table=changed(8, -np.inf)),
        "src_row_bytes not 0": dict(srow=80 * 3),
        "dst_row_bytes not 0": dict(drow=70 * 3),
        "more than 2^31 tiles": dict(table=many, fmt=L.PIX_U8 | L.WARP_RAGGED, sw=8, sh=8, dst_bytes=2**36, ow=1, oh=2**31 - 1),
        "batch 0": dict(table=good[:0]),
        "unknown pixel format": dict(fmt=3 | L.WARP_RAGGED),
        "f32 source offset not a multiple of 4": dict(f32_call, table=changed(15, 4002, base=f32)),
        "f32 source stride not a multiple of 4": dict(f32_call, table=changed(16, 34, base=f32)),
        "f32 output offset not a multiple of 4": dict(f32_call, table=changed(11, f32[1, 11] + 2, base=f32)),
        "f32 destination misaligned": dict(f32_call, dst="odd"),
        "f32 source misaligned": dict(f32_call, src="odd"),
        "prepare: output offset not a multiple of 4": dict(prep_call, table=changed(11, prep[1, 11] + 1, base=prep)),
        "prepare: output stride not a multiple of 4": dict(prep_call, table=changed(12, prep[1, 12] + 2, base=prep)),
        "prepare: destination misaligned": dict(prep_call, dst="odd"),
        "prepare: output wider than the source": dict(prep_call, table=changed(9, 34, base=prep)),
        "prepare: stride of a u8 row (outputs are f32)": dict(prep_call, table=changed(12, 36, base=prep)),
    }
    try:
        for name, kw in cases.items():
            kw = dict(kw)
            for side, base in (("dst", d_dst), ("src", d_src)):
                if kw.get(side) == "odd":
                    kw[side] = base + 2
            rc = call(**kw)
            msg = lib.lr_last_error().decode()
            assert rc != 0, name
            assert msg.startswith(PREFIX) and len(msg) > len(PREFIX), (name, msg)
            assert (ctx.device_download(d_dst, (region,), np.uint8) == SENTINEL).all(), name
        rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), len(buf), 3, 80, 50, 0, fmt, P(good), None, region, 70, 50, 0)
        assert rc != 0 and lib.lr_last_error().decode().startswith(PREFIX)

        def fresh():
            ctx.synchronize()
            assert lib.lr_memcpy_h2d(ctx._h, C.c_void_p(d_dst), P(np.full(region, SENTINEL, np.uint8)), region) == 0

        # the tables the f32 and prepare cases start from are themselves accepted, NaN maps and all
        assert call(**f32_call) == 0, lib.lr_last_error()
        fresh()
        assert call(**prep_call) == 0, lib.lr_last_error()
        got = ctx.device_download(d_dst, (region,), np.uint8)
        for b, (ow, oh) in enumerate([(32, 24), (33, 50), (8, 2)]):
            assert_same(cut(got, prep[b, :13], 2), PR.prepare(srcs[b], ow, oh))
        assert (got[~written_mask(region, prep[:, :13], 4)] == SENTINEL).all()
        fresh()

        def valid():
            assert call() == 0, lib.lr_last_error()
            got = ctx.device_download(d_dst, (region,), np.uint8)
            for b, (ow, oh) in enumerate(sizes):
                np.testing.assert_array_equal(cut(got, good[b, :13], 1), R.warp(srcs[b], Ms[b], ow, oh))
            assert (got[~written_mask(region, good[:, :13], 3)] == SENTINEL).all()

        assert call(table=overlap) != 0
        valid()  # the next valid call on the same context
        ctx.trim()
        valid()
        # ... and the calls that existed before: the plain warp, the packed warp and the single-size prepare
        w, h, off, row = sources[0]
        ctx.warp_perspective_device(d_src + off, 0, 1, w, h, row, 1, np.eye(3), d_dst, region, w, h, w * 3)
        np.testing.assert_array_equal(ctx.device_download(d_dst, (h, w, 3), np.uint8), srcs[0])
        ptable, ptotal = L.warp_table(Ms[:1], sizes[:1], 3)
        ctx.warp_perspective_packed_device(d_src + off, 0, 1, w, h, row, 1, ptable, d_dst, region)
        np.testing.assert_array_equal(cut(ctx.device_download(d_dst, (region,), np.uint8), ptable[0], 1), R.warp(srcs[0], Ms[0], *sizes[0]))
        ctx.prepare_device(d_src + off, 0, 1, w, h, row, 1, d_dst, region, 32, 24, 32 * 4)
        assert_same(ctx.device_download(d_dst, (24, 32), np.float32), PR.prepare(srcs[0], 32, 24))
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


# ---- the batch detector with a frame table -----------------------------------------------------------------------

LONG = [(640, 480)] + [(160, 120)] * 10 + [(257, 131)]  # small frames in a row after a large one: the shrink counter rests
MIXED = [(320, 240), (96, 64), (777, 401), (4, 4)] * 2  # lanes that change size every frame, and the answer below 5 x 5
MIN_LENGTH = 3.0


def detector_frame(fmt, w, h, seed):
    from librectify_amd import synth

    if fmt == 0:
        return gray_frame(w, h, seed)
    if fmt == 1:
        return synthetic_rgb(w, h, seed)
    return np.ascontiguousarray(synth.frame(w, h, seed), np.float32)


@pytest.fixture(scope="module")
def lists(ctx):
    """the detector lists that the tests below have put on the device, freed when the module is done"""
    made = {}
    yield made
    for lst in made.values():
        ctx.device_free(lst["d"])


def detector_list(_lists, ctx, which, fmt):
    """The frames of a list on the device (one allocation, padded strides, left there for the module) and, per refine
    flag, what the single-frame call gives for each"""
    key = (which, fmt)
    if key not in _lists:
        sizes = LONG if which == "long" else MIXED
        frames = [detector_frame(fmt, w, h, 500 + 7 * k) for k, (w, h) in enumerate(sizes)]
        bpp = BPP[fmt]
        sources, cursor = [], 0
        for k, (w, h) in enumerate(sizes):
            row = (w + (3, 0, 8, 1)[k % 4]) * bpp  # (the detector's strides are whole pixels)
            sources.append((w, h, cursor, row))
            cursor += (h * row + 15) // 16 * 16
        buf = np.full(cursor, 0x5A, np.uint8)
        for f, (w, h, off, row) in zip(frames, sources):
            np.lib.stride_tricks.as_strided(buf[off:], (h, w * bpp), (row, 1))[:] = np.ascontiguousarray(f).reshape(h, -1).view(np.uint8)
        _lists[key] = dict(d=ctx.device_upload(buf), sources=sources, ref={})
    return _lists[key]


def frames_word(L, fmt, refine):
    return ((fmt + 1) << 8) | int(refine)  # (a format word for f32 too: frames below 5 x 5 are then answered, not refused)


def single_frames(L, ctx, lst, fmt, refine, min_lengths):
    """per frame: lr_find_line_segment_groups_device and compute_rectification_transform for its own size"""
    key = (refine, tuple(min_lengths))
    if key not in lst["ref"]:
        lib, bpp, res = L.lib(), BPP[fmt], []
        cfg = L.RectificationConfig()
        for (w, h, off, row), ml in zip(lst["sources"], min_lengths):
            out, n = np.zeros(4096, L.LINE_DTYPE), C.c_int(-1)
            rc = lib.lr_find_line_segment_groups_device(ctx._h, C.c_void_p(lst["d"] + off), w, h, row // bpp, ml, frames_word(L, fmt, refine), -1, P(out), 4096, C.byref(n))
            assert rc == 0, lib.lr_last_error()
            assert n.value <= 4096
            lines = out[: n.value].copy()
            res.append((lines, L.compute_rectification_transform(lines, w, h, cfg)))
        lst["ref"][key] = res
    return lst["ref"][key]


def frame_table(L, lst, fmt, min_lengths=None):
    bpp = BPP[fmt]
    rows = [L.Frame(lst["d"] + off, w, h, row // bpp, -1.0 if min_lengths is None else min_lengths[b])
            for b, (w, h, off, row) in enumerate(lst["sources"])]
    return (L.Frame * len(rows))(*rows)


def table_call(L, ctx, table, word, min_length=MIN_LENGTH, capacity=4096, image_stride=24, stride=0, batch=None):
    batch = len(table) if batch is None else batch
    out = np.zeros((len(table), capacity), L.LINE_DTYPE)
    n = np.full(len(table), -1, np.int32)
    tf = (L.ImageTransform * len(table))()
    cfg = L.RectificationConfig()
    rc = L.lib().lr_find_line_segment_groups_batch_device(ctx._h, C.cast(table, C.c_void_p), image_stride, batch, 0, 0, stride, min_length, word, -1, P(out), capacity, P(n), C.byref(cfg), C.byref(tf))
    return rc, out, n, tf


def assert_table_result(out, n, tf, want, capacity=4096):
    for b, (lines, t) in enumerate(want):
        assert n[b] == len(lines), "frame %d: count" % b
        k = min(len(lines), capacity)
        assert out[b][:k].tobytes() == lines[:k].tobytes(), "frame %d: lines" % b
        if len(lines) <= capacity:
            assert bytes(tf[b]) == bytes(t), "frame %d: transform" % b


@pytest.fixture
def streams(ctx):
    yield ctx.set_batch_streams
    ctx.set_batch_streams(5)


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("lanes", [1, 2, 5])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_frame_table_equals_the_single_frame_calls(L, ctx, lists, streams, fmt, lanes, refine):
    word = frames_word(L, fmt, refine)
    for which in ("long", "mixed"):
        lst = detector_list(lists, ctx, which, fmt)
        B = len(lst["sources"])
        want = single_frames(L, ctx, lst, fmt, refine, [MIN_LENGTH] * B)
        print(which, fmt, refine, "lines per frame:", [len(x[0]) for x in want])
        assert max(len(x[0]) for x in want) > 10, "the frames have lines to compare"
        if which == "mixed":
            assert len(want[3][0]) == 0 and want[3][1].width == 4  # (below 5 x 5: no lines, the transform of its size)
        streams(lanes)
        rc, out, n, tf = table_call(L, ctx, frame_table(L, lst, fmt), word)
        assert rc == 0, L.lib().lr_last_error()
        assert_table_result(out, n, tf, want)


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_frame_table_capacity_and_min_length(L, ctx, lists, streams, fmt):
    lst = detector_list(lists, ctx, "long", fmt)
    B = len(lst["sources"])
    word = frames_word(L, fmt, False)
    want = single_frames(L, ctx, lst, fmt, False, [MIN_LENGTH] * B)
    streams(5)
    # capacity 8: the full counts, eight records each, and nothing behind them
    assert max(len(x[0]) for x in want) > 8
    rc, out, n, tf = table_call(L, ctx, frame_table(L, lst, fmt), word, capacity=8)
    assert rc == 0, L.lib().lr_last_error()
    assert_table_result(out, n, tf, want, capacity=8)
    # a frame's own min_length is honoured; -1 takes the call's
    own = [25.0 if b % 2 else -1.0 for b in range(B)]
    mixed = single_frames(L, ctx, lst, fmt, False, [MIN_LENGTH if v < 0 else v for v in own])
    assert any(len(a[0]) != len(b[0]) for a, b in zip(want, mixed)), "the longer min_length drops lines"
    rc, out, n, tf = table_call(L, ctx, frame_table(L, lst, fmt, own), word)
    assert rc == 0, L.lib().lr_last_error()
    assert_table_result(out, n, tf, mixed)
    # the Python entry
    bpp = BPP[fmt]
    rows = [(lst["d"] + off, w, h, row // bpp) for w, h, off, row in lst["sources"]]
    for table in (frame_table(L, lst, fmt), rows):
        lines, tfs = ctx.find_line_segment_groups_frames_device(table, fmt, MIN_LENGTH)
        for b in range(B):
            assert lines[b].tobytes() == want[b][0].tobytes() and bytes(tfs[b]) == bytes(want[b][1])


def test_frame_table_refusals_leave_the_uniform_batch_as_it_was(L, ctx, lists, streams):
    lib = L.lib()
    fmt = 0
    lst = detector_list(lists, ctx, "long", fmt)
    word = frames_word(L, fmt, False)
    streams(5)
    # a uniform batch: the ten 160 x 120 frames are not equally strided, so two of one stride
    (w, h, off1, row), (_, _, off5, row5) = lst["sources"][1], lst["sources"][5]
    assert row == row5
    uniform = lambda: ctx.find_line_segment_groups_batch_device(lst["d"] + off1, off5 - off1, 2, w, h, MIN_LENGTH, fmt=fmt, stride=row)  # noqa: E731
    out0, n0, tf0 = uniform()
    assert n0.min() > 0

    def row_changed(b, **kw):
        t = frame_table(L, lst, fmt)
        for k, v in kw.items():
            setattr(t[b], k, v)
        return t

    good = frame_table(L, lst, fmt)
    cases = {
        "image_stride not 24": dict(table=good, image_stride=32),
        "stride not 0": dict(table=good, stride=640),
        "null data": dict(table=row_changed(3, data=None)),
        "width 0": dict(table=row_changed(11, width=0)),
        "stride below the width": dict(table=row_changed(0, stride=639)),
    }
    for name, kw in cases.items():
        rc, out, n, tf = table_call(L, ctx, word=word, **kw)
        assert rc != 0 and lib.lr_last_error(), name
        assert (n == -1).all() and not out.view(np.uint8).any(), name + ": nothing was written"
    # a misaligned f32 address, and a frame below 5 x 5 under the plain flag
    odd = row_changed(2, data=lst["d"] + lst["sources"][2][2] + 2)
    assert table_call(L, ctx, odd, frames_word(L, 2, False))[0] != 0
    tiny = row_changed(2, width=4, height=4, stride=4)
    assert table_call(L, ctx, tiny, 0)[0] != 0 and table_call(L, ctx, tiny, 1)[0] != 0
    # the 0 x 0 mode exists on this one entry only
    outh, nh = np.zeros((12, 64), L.LINE_DTYPE), np.zeros(12, np.int32)
    rc = lib.lr_find_line_segment_groups_batch_host(ctx._h, C.cast(good, C.c_void_p), 24, 12, 0, 0, 0, MIN_LENGTH, word, -1, P(outh), 64, P(nh), None, None)
    assert rc != 0 and lib.lr_last_error()
    out1, n1, tf1 = uniform()
    assert n1.tolist() == n0.tolist() and out1.tobytes() == out0.tobytes() and bytes(tf1) == bytes(tf0)
    # ... and a table call after them is right
    want = single_frames(L, ctx, lst, fmt, False, [MIN_LENGTH] * 12)
    rc, out, n, tf = table_call(L, ctx, good, word)
    assert rc == 0, lib.lr_last_error()
    assert_table_result(out, n, tf, want)


# ---- rectify_batch on a mixed list -------------------------------------------------------------------------------

MIXED_SHAPES = [(480, 360), (360, 480), (777, 401), (320, 240), (640, 480)]


def mixed_frames(colour):
    return [(synthetic_rgb if colour else gray_frame)(w, h, 3 + b) for b, (w, h) in enumerate(MIXED_SHAPES)]


@pytest.mark.parametrize("colour", [True, False])
def test_rectify_batch_on_a_mixed_list_equals_a_loop_of_rectify(L, ctx, colour):
    frames = mixed_frames(colour)
    for s in SETTINGS + [dict(max_size=400)]:
        kw = _kw(L, s)
        want = [ctx.rectify(f, **kw) for f in frames]
        assert all(len(x[0]) > 10 for x in want)
        same_results(ctx.rectify_batch(frames, **kw), want, str(s))
        if s == dict(max_size=400):
            scaled = [L.prepared_size(w, h, 400)[2] != 1 for w, h in MIXED_SHAPES]
            assert scaled[1] and not scaled[3], "360 x 480 is prescaled, 320 x 240 is not"
        if not s:
            # a first detector pass with too small a capacity still returns every line
            assert max(len(x[0]) for x in want) > 8
            same_results(ctx.rectify_batch(frames, capacity=8), want, "capacity 8")


def test_rectify_batch_mixed_list_rules(L, ctx):
    gray, rgb = mixed_frames(False), mixed_frames(True)
    two = ctx.rectify_batch([gray[3], gray[0]])  # (two shapes: the mixed-size pipeline)
    assert len(two) == 2 and two[0][2].ndim == 2 and two[0][0].tobytes() == ctx.rectify(gray[3])[0].tobytes()
    with pytest.raises(ValueError):
        ctx.rectify_batch([gray[0], rgb[1]])
    with pytest.raises(ValueError):
        ctx.rectify_batch([gray[0], gray[1].astype(np.float32)])
    # a list of one shape is the array call
    same = [gray_frame(320, 240, 20 + b) for b in range(3)]
    same_results(ctx.rectify_batch(same), ctx.rectify_batch(np.stack(same)), "a list of one shape")


def test_rectify_frames_device_on_a_resident_region(L, ctx):
    frames = mixed_frames(True)
    buf, sources = source_region(frames, 1, whole_pixels=True)
    for kw in (dict(), dict(max_size=300, refine=True)):
        want = ctx.rectify_batch(frames, **kw)
        d = ctx.device_upload(buf)
        d_out = None
        try:
            lines, tfs, table, d_out, total = ctx.rectify_frames_device(d, sources, L.PIX_U8X3, **kw)
            got = ctx.device_download(d_out, (total,), np.uint8)
        finally:
            ctx.device_free(d)
            if d_out:
                ctx.device_free(d_out)
        assert table.shape == (5, 18) and total == int(table[4, 11] + (table[4, 10] - 1) * table[4, 12] + table[4, 9] * 3)
        np.testing.assert_array_equal(table[:, 13:17], sources)
        for b in range(5):
            assert lines[b].tobytes() == want[b][0].tobytes() and bytes(tfs[b]) == bytes(want[b][1])
            np.testing.assert_array_equal(cut(got, table[b, :13], 1), want[b][2])
