"""Baseline JPEG streams on the GPU: lr_encode_jpeg_device (kernels_jpeg.hip) against tests/numpy_jpeg_ref.py, byte for byte:
the shapes at which the transform and the entropy coder take another path (less than a block, partial MCUs, 4:2:0 blocks
wholly outside the frame, more than eight restart intervals, a partial last interval, many workgroups), the contents that
reach the longest codes, byte stuffing, category 11 and ZRL runs, a batch at unordered places with guard bytes, a capacity
below a stream's need, the pipeline (rectify_batch and draw_lines_batch with jpeg=), trim, and the clean failures (each
refused on the host before anything is launched: the tests provoke nothing on the device)."""
import ctypes as C

import numpy as np
import pytest

import numpy_jpeg_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
PREFIX = "lr_encode_jpeg_device: "
KINDS = ["u8", "420", "444"]  # one component; colour 4:2:0; colour 4:4:4
SHAPES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (203, 117), (256, 200), (300, 150), (640, 360)]


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


def layout_of(kind):
    return 1 if kind == "444" else 0


def as_kind(gray, kind):
    """a gray picture as a frame of the kind (three equal channels for colour)"""
    return gray if kind == "u8" else np.ascontiguousarray(np.stack([gray, gray, gray], axis=-1))


def textured(w, h, seed, kind):
    """a ramp under noise of +-20: every coefficient class occurs, and the reference stays quick"""
    rng = np.random.default_rng(seed)
    shape = (h, w) if kind == "u8" else (h, w, 3)
    y, x = np.mgrid[0:h, 0:w]
    ramp = (3 * x + 2 * y) % 256
    if kind != "u8":
        ramp = np.stack([ramp, (ramp + 85) % 256, (2 * ramp) % 256], axis=-1)
    return np.clip(ramp + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)


def check(ctx, img, quality, kind):
    got = ctx.encode_jpeg(img, quality, layout_of(kind))
    want = R.encode(img, quality, layout_of(kind))
    assert isinstance(got, bytes)
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError("%d bytes, want %d; the first difference at byte %d" % (len(got), len(want), first))
    return want


def test_the_shapes_cover_the_marker_wrap_and_a_partial_interval():
    for kind in KINDS:
        comps = 1 if kind == "u8" else 3
        n = {s: R.intervals(s[0], s[1], layout_of(kind), comps) for s in SHAPES}
        assert max(n.values()) > 8, kind
        mcu = 16 if kind == "420" else 8
        ri = R.restart_interval(0, layout_of(kind), comps)
        assert any((-(-w // mcu)) * (-(-h // mcu)) % ri for w, h in SHAPES), kind


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_shapes(ctx, kind, shape):
    w, h = shape
    check(ctx, textured(w, h, 7 + w, kind), 85, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_constant_frames(ctx, kind):
    for value in (0, 128, 255):
        img = as_kind(np.full((24, 40), value, np.uint8), kind)
        check(ctx, img, 75, kind)
    coefs, _ = R.coefficients(as_kind(np.full((16, 16), 128, np.uint8), kind), 75, layout_of(kind))
    assert not coefs.any(), "constant 128 is all-zero coefficients"


@pytest.mark.parametrize("kind", KINDS)
def test_noise_at_quality_100_stuffs_bytes(ctx, kind):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (40, 48) if kind == "u8" else (40, 48, 3), dtype=np.uint8)
    want = check(ctx, img, 100, kind)
    scan = want[want.index(b"\xFF\xDA"):]
    assert b"\xFF\x00" in scan, "the case has stuffed bytes"


@pytest.mark.parametrize("kind", KINDS)
def test_alternating_blocks_reach_category_11(ctx, kind):
    by, bx = np.mgrid[0:8, 0:8]
    gray = np.kron(((by + bx) & 1) * 255, np.ones((8, 8), np.int64)).astype(np.uint8)
    img = as_kind(gray, kind)
    coefs, _ = R.coefficients(img, 100, layout_of(kind))
    dc = coefs[:, 0, 0] if kind != "420" else coefs[:, :4, 0].reshape(-1)
    assert np.abs(np.diff(dc)).max() >= 1024, "a DC difference of category 11"
    check(ctx, img, 100, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_one_late_coefficient_gives_zrl_and_no_eob(ctx, kind):
    i = np.arange(8)
    wave = np.cos((2 * i + 1) * 7 * np.pi / 16)
    tile = 128 + 100 * np.outer(wave, wave)
    gray = np.tile(np.round(tile), (3, 5)).astype(np.uint8)
    img = as_kind(gray, kind)
    coefs, _ = R.coefficients(img, 95, layout_of(kind))
    blocks = coefs.reshape(-1, 64)
    late = blocks[(blocks[:, 63] != 0) & ~blocks[:, 1:63].any(axis=1)]
    assert len(late), "a block whose only AC coefficient is index 63: three ZRL, a run of 14, and no EOB"
    check(ctx, img, 95, kind)
    check(ctx, img, 100, kind)  # (rounding adds a few +-1 in front of it: runs of every length)


@pytest.mark.parametrize("quality", [1, 50, 95])
@pytest.mark.parametrize("kind", KINDS)
def test_synth_frame(ctx, kind, quality):
    check(ctx, R.synth_u8(203, 117, 21, kind != "u8"), quality, kind)


# ---- the raw call: a batch at places of its own, guard bytes, capacity, failures ----

def raw_call(L, ctx, fmt, frames, rows, src_pad=0, dst_bytes=None, **kw):
    """frames: arrays; rows: per frame (stream offset, capacity, quality, layout).  Returns (rc, sizes, destination)."""
    bpp = 3 if fmt == L.PIX_U8X3 else 1
    sources, end = [], src_pad
    for f in frames:
        h, w = f.shape[:2]
        sources.append((end, w * bpp))
        end += f.nbytes + 5  # (odd places: nothing needs alignment)
    region = np.full(end, 0x11, np.uint8)
    for f, (off, _) in zip(frames, sources):
        region[off:off + f.nbytes] = f.reshape(-1)
    table = np.array([[f.shape[1], f.shape[0], s[0], s[1], r[0], r[1], r[2], r[3]] for f, s, r in zip(frames, sources, rows)], np.float64)
    for b, col, v in kw.get("poke", []):
        table[b, col] = v
    if dst_bytes is None:
        dst_bytes = int(max(r[0] + r[1] for r in rows)) + 64
    dst = np.full(dst_bytes, SENTINEL, np.uint8)
    sizes = np.full(len(frames), 0xDEADBEEF, np.uint64)
    d_src, d_dst = ctx.device_upload(region), ctx.device_upload(dst)
    try:
        args = L.JpegArgs(table.ctypes.data, None if kw.get("null_sizes") else sizes.ctypes.data)
        word = kw.get("word", fmt | L.WARP_JPEG)
        extra = kw.get("extra", (0, 0, 0, 0, 0, 0))  # width, height, src_row_bytes, out_width, out_height, dst_row_bytes
        rc = L.lib().lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), end, len(frames), extra[0], extra[1], extra[2], word,
                                                C.cast(C.byref(args), C.c_void_p), C.c_void_p(d_dst), dst_bytes, extra[3], extra[4], extra[5])
        return rc, sizes, ctx.device_download(d_dst, (dst_bytes,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def assert_only_extents_written(dst, extents):
    mask = np.ones(len(dst), bool)
    for off, n in extents:
        mask[off:off + n] = False
    assert (dst[mask] == SENTINEL).all(), "a byte outside the frames' extents was written"


def test_batch_of_five_at_unordered_places(L, ctx):
    shapes = [(203, 117), (17, 33), (64, 48), (9, 7), (130, 90)]
    frames = [textured(w, h, 30 + b, "420") for b, (w, h) in enumerate(shapes)]
    quals, layouts = [95, 10, 50, 100, 75], [0, 1, 1, 0, 0]
    want = [R.encode(f, q, l) for f, q, l in zip(frames, quals, layouts)]
    singles = [ctx.encode_jpeg(f, q, l) for f, q, l in zip(frames, quals, layouts)]
    assert singles == want
    order, at, offs = [3, 0, 4, 1, 2], 13, {}
    for b in order:  # (unordered, with gaps of odd sizes; capacities a little above the need)
        offs[b] = at
        at += len(want[b]) + 7 + 3 * b
    rows = [(offs[b], len(want[b]) + 7, quals[b], layouts[b]) for b in range(5)]
    rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, frames, rows)
    assert rc == 0, L.lib().lr_last_error()
    assert sizes.tolist() == [len(s) for s in want]
    for b in range(5):
        assert dst[offs[b]:offs[b] + len(want[b])].tobytes() == want[b], "frame %d" % b
    assert_only_extents_written(dst, [(offs[b], len(want[b])) for b in range(5)])
    # one-component frames in one call, too
    gray = [textured(w, h, 40 + b, "u8") for b, (w, h) in enumerate(shapes[:3])]
    gwant = [R.encode(f, 80, 0) for f in gray]
    rows = [(20000 * b + 1, 19999, 80, 0) for b in range(3)]
    assert max(len(s) for s in gwant) < 19999
    rc, sizes, dst = raw_call(L, ctx, L.PIX_U8, gray, rows, src_pad=3)
    assert rc == 0 and sizes.tolist() == [len(s) for s in gwant]
    for b in range(3):
        assert dst[rows[b][0]:rows[b][0] + len(gwant[b])].tobytes() == gwant[b]
    assert_only_extents_written(dst, [(rows[b][0], len(gwant[b])) for b in range(3)])


def test_a_capacity_below_the_need(L, ctx):
    frames = [textured(64, 48, 50 + b, "444") for b in range(3)]
    want = [R.encode(f, 90, 1) for f in frames]
    for short in (len(want[1]) - 1, 700, 100, 1, 0):  # the EOI, an interval, the header cut; nothing at all
        rows = [(10, len(want[0]), 90, 1), (10000, short, 90, 1), (20000, len(want[2]) + 50, 90, 1)]
        rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, frames, rows)
        assert rc == 0, L.lib().lr_last_error()
        assert sizes.tolist() == [len(s) for s in want], "sizes report the need"
        assert dst[10:10 + len(want[0])].tobytes() == want[0] and dst[20000:20000 + len(want[2])].tobytes() == want[2]
        assert_only_extents_written(dst, [(10, len(want[0])), (10000, short), (20000, len(want[2]))])


def test_clean_failures(L, ctx):
    frames = [textured(40, 24, 60, "420"), textured(24, 40, 61, "420")]
    rows = [(0, 4000, 90, 0), (5000, 4000, 90, 0)]
    gray = [f[..., 0].copy() for f in frames]
    J = L.WARP_JPEG
    cases = [
        ("LR_PIX_F32", dict(word=L.PIX_F32 | J)),
        ("a second option bit", dict(word=L.PIX_U8X3 | J | L.WARP_RAGGED)),
        ("with LR_WARP_LINES", dict(word=L.PIX_U8X3 | J | L.WARP_LINES)),
        ("an unknown bit", dict(word=L.PIX_U8X3 | J | 0x400)),
        ("a width", dict(extra=(40, 0, 0, 0, 0, 0))),
        ("a height", dict(extra=(0, 24, 0, 0, 0, 0))),
        ("a source stride", dict(extra=(0, 0, 120, 0, 0, 0))),
        ("an output size", dict(extra=(0, 0, 0, 40, 24, 0))),
        ("an output stride", dict(extra=(0, 0, 0, 0, 0, 120))),
        ("null sizes", dict(null_sizes=True)),
        ("overlapping extents", dict(poke=[(1, 4, 3999)])),
        ("quality 0", dict(poke=[(1, 6, 0)])),
        ("quality 101", dict(poke=[(0, 6, 101)])),
        ("quality 50.5", dict(poke=[(0, 6, 50.5)])),
        ("layout 2", dict(poke=[(1, 7, 2)])),
        ("width 65536", dict(poke=[(1, 0, 65536)])),
        ("height 65536", dict(poke=[(0, 1, 65536)])),
        ("width 0", dict(poke=[(0, 0, 0)])),
        ("a stride below a row", dict(poke=[(0, 3, 119)])),
        ("a source beyond the region", dict(poke=[(1, 2, 1e9)])),
        ("an extent beyond the region", dict(poke=[(1, 5, 1e9)])),
        ("a NaN", dict(poke=[(0, 4, float("nan"))])),
    ]
    for name, kw in cases:
        rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, frames, rows, **kw)
        msg = L.lib().lr_last_error().decode()
        assert rc != 0 and msg, name
        assert (dst == SENTINEL).all(), name + ": nothing is written"
        assert (sizes == 0xDEADBEEF).all(), name + ": sizes are untouched"
    rc, sizes, dst = raw_call(L, ctx, L.PIX_U8, gray, rows, poke=[(1, 7, 1)])
    assert rc != 0 and (dst == SENTINEL).all() and (sizes == 0xDEADBEEF).all(), "layout 1 on u8"
    assert L.lib().lr_last_error().decode().startswith(PREFIX + "frame 1: entry [7]")
    # ... and the call after them is right
    rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, frames, rows)
    assert rc == 0 and dst[5000:5000 + int(sizes[1])].tobytes() == R.encode(frames[1], 90, 0)


def test_trim_and_the_next_call(L, ctx):
    img = textured(130, 90, 70, "420")
    want = R.encode(img, 92, 0)
    assert ctx.encode_jpeg(img, 92, 0) == want
    ctx.trim()
    assert ctx.encode_jpeg(img, 92, 0) == want
    assert ctx.encode_jpeg_batch([img, img[:50, :60]], 92, 1) == [R.encode(img, 92, 1), R.encode(img[:50, :60], 92, 1)]


# ---- the pipeline ----

def detector_frame(w, h, seed):
    from librectify_amd import synth

    g = np.clip(synth.frame(w, h, seed, bars=40) * 255.0, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))


def test_rectify_batch_with_jpeg(L, ctx):
    frames = [detector_frame(w, h, 3 + b) for b, (w, h) in enumerate([(160, 120), (120, 160), (160, 120), (120, 160)])]
    raw = ctx.rectify_batch(frames)
    assert sum(r[2] is not None for r in raw) >= 2, "the case has pictures to encode"
    want = [None if r[2] is None else R.encode(r[2], 90, 0) for r in raw]
    for first in (None, 600):  # (600: every frame's first extent is too small)
        ctx.jpeg_first_capacity = first
        try:
            got = ctx.rectify_batch(frames, jpeg=90)
        finally:
            ctx.jpeg_first_capacity = None
        for b, (g, r) in enumerate(zip(got, raw)):
            assert g[0].tobytes() == r[0].tobytes() and bytes(g[1]) == bytes(r[1]), "frame %d: lines and transform" % b
            assert g[2] == want[b], "frame %d (first capacity %s)" % (b, first)
    # one shape (the uniform batch), one frame, and gray
    same = [frames[0], frames[2]]
    for g, r in zip(ctx.rectify_batch(same, jpeg=75), ctx.rectify_batch(same)):
        assert g[0].tobytes() == r[0].tobytes() and g[2] == (None if r[2] is None else R.encode(r[2], 75, 0))
    b = next(i for i, r in enumerate(raw) if r[2] is not None)
    one = ctx.rectify(frames[b], jpeg=90)
    assert one[0].tobytes() == raw[b][0].tobytes() and one[2] == want[b]
    g = frames[b][..., 0].copy()
    lines, t, warped = ctx.rectify(g)
    assert ctx.rectify(g, jpeg=60)[2] == R.encode(warped, 60, 0)


def test_draw_lines_batch_with_jpeg(L, ctx):
    frames = [detector_frame(w, h, 3 + b) for b, (w, h) in enumerate([(160, 120), (120, 160)])]
    lines = [ctx.rectify(f)[0] for f in frames]
    pictures = ctx.draw_lines_batch(frames, lines)
    want = [R.encode(p, 90, 0) for p in pictures]
    assert ctx.draw_lines_batch(frames, lines, jpeg=90) == want
    ctx.jpeg_first_capacity = 300
    try:
        assert ctx.draw_lines_batch(frames, lines, jpeg=90) == want
    finally:
        ctx.jpeg_first_capacity = None
