"""LR_JPEG_OPTIMIZE on the GPU: lr_encode_jpeg_device with a frame's own Huffman tables (kernels_jpeg.hip: the count mode of the
block coder, jpeg_tables_kernel, the per-frame-table entropy coder) against tests/numpy_jpeg_optimize_ref.py, byte for byte,
through the C ABI: the shapes of test_gpu_jpeg's small end, a frame whose luminance AC table needs the K.3 limiter, a batch
that mixes frames with and without the option in any order, the decoder's round trip, capacities and guard bytes, a second
call on the same context, the table check (refused on the host: nothing is provoked on the device), the Python keywords, and
a flat 16384 x 16384 frame on either side of the count at which the tables kernel goes from 32-bit to 64-bit keys."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import numpy_jpeg_optimize_ref as O
import numpy_jpeg_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
PREFIX = "lr_encode_jpeg_device: "
OPT = 0x10  # LR_JPEG_OPTIMIZE
KINDS = ["u8", "420", "444"]
SHAPES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (203, 117)]
HERE = os.path.dirname(os.path.abspath(__file__))


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


def textured(w, h, seed, kind):
    """a ramp under noise of +-20: every coefficient class occurs, and the reference stays quick"""
    rng = np.random.default_rng(seed)
    shape = (h, w) if kind == "u8" else (h, w, 3)
    y, x = np.mgrid[0:h, 0:w]
    ramp = (3 * x + 2 * y) % 256
    if kind != "u8":
        ramp = np.stack([ramp, (ramp + 85) % 256, (2 * ramp) % 256], axis=-1)
    return np.clip(ramp + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def doc_half():
    """the 500 x 282 decimation of the doc image: its luminance AC table reaches 17 bits before the limit
    (test_jpeg_optimize_cpu asserts it)"""
    from PIL import Image

    img = np.asarray(Image.open(os.path.join(HERE, "golden", "doc_image.jpg")).convert("RGB"))
    return np.ascontiguousarray(img[::2, ::2])


def raw_call(L, ctx, fmt, frames, rows, dst_bytes=None, poke=()):
    """frames: arrays; rows: per frame (stream offset, capacity, quality, [7]).  Returns (rc, sizes, destination)."""
    bpp = 3 if fmt == L.PIX_U8X3 else 1
    sources, end = [], 3
    for f in frames:
        sources.append((end, f.shape[1] * bpp))
        end += f.nbytes + 5  # (odd places: nothing needs alignment)
    region = np.full(end, 0x11, np.uint8)
    for f, (off, _) in zip(frames, sources):
        region[off:off + f.nbytes] = f.reshape(-1)
    table = np.array([[f.shape[1], f.shape[0], s[0], s[1], r[0], r[1], r[2], r[3]] for f, s, r in zip(frames, sources, rows)], np.float64)
    for b, col, v in poke:
        table[b, col] = v
    if dst_bytes is None:
        dst_bytes = int(max(r[0] + r[1] for r in rows)) + 64
    dst = np.full(dst_bytes, SENTINEL, np.uint8)
    sizes = np.full(len(frames), 0xDEADBEEF, np.uint64)
    d_src, d_dst = ctx.device_upload(region), ctx.device_upload(dst)
    try:
        args = L.JpegArgs(table.ctypes.data, sizes.ctypes.data)
        rc = L.lib().lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), end, len(frames), 0, 0, 0, fmt | L.WARP_JPEG,
                                                C.cast(C.byref(args), C.c_void_p), C.c_void_p(d_dst), dst_bytes, 0, 0, 0)
        return rc, sizes, ctx.device_download(d_dst, (dst_bytes,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def assert_only_extents_written(dst, extents):
    mask = np.ones(len(dst), bool)
    for off, n in extents:
        mask[off:off + n] = False
    assert (dst[mask] == SENTINEL).all(), "a byte outside the frames' extents was written"


def same(got, want, what=""):
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError("%s%d bytes, want %d; the first difference at byte %d" % (what, len(got), len(want), first))


def one(L, ctx, img, quality, kind, optimize=True):
    """the stream of one frame through the C ABI, the capacity lr_jpeg_bound's"""
    fmt = L.PIX_U8 if kind == "u8" else L.PIX_U8X3
    cap = L.jpeg_bound(img.shape[1], img.shape[0], fmt, layout_of(kind), optimize=optimize)
    rc, sizes, dst = raw_call(L, ctx, fmt, [img], [(16, cap, quality, layout_of(kind) + (OPT if optimize else 0))])
    assert rc == 0, L.lib().lr_last_error()
    assert int(sizes[0]) <= cap
    assert_only_extents_written(dst, [(16, int(sizes[0]))])
    return dst[16:16 + int(sizes[0])].tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_shapes_byte_for_byte(L, ctx, kind, shape):
    w, h = shape
    img = textured(w, h, 7 + w, kind)
    same(one(L, ctx, img, 95, kind), O.encode(img, 95, layout_of(kind)))


@pytest.mark.parametrize("quality", [1, 100])
@pytest.mark.parametrize("kind", KINDS)
def test_qualities_byte_for_byte(L, ctx, kind, quality):
    img = textured(17, 33, 24, kind)
    same(one(L, ctx, img, quality, kind), O.encode(img, quality, layout_of(kind)))


@pytest.mark.parametrize("kind", KINDS)
def test_the_limiter_frame_byte_for_byte(L, ctx, kind):
    img = doc_half() if kind != "u8" else np.ascontiguousarray(doc_half()[..., 1])
    same(one(L, ctx, img, 95, kind), O.encode(img, 95, layout_of(kind)))


def test_mixed_batch_in_any_order(L, ctx):
    shapes = [(203, 117), (17, 33), (64, 48), (9, 7), (130, 90), (33, 200)]
    frames = [textured(w, h, 30 + b, "420") for b, (w, h) in enumerate(shapes)]
    quals, layouts = [95, 10, 50, 100, 75, 95], [0, 1, 1, 0, 0, 1]
    plain = [R.encode(f, q, l) for f, q, l in zip(frames, quals, layouts)]
    optimised = [O.encode(f, q, l) for f, q, l in zip(frames, quals, layouts)]
    cap = [L.jpeg_bound(w, h, L.PIX_U8X3, l, optimize=True) for (w, h), l in zip(shapes, layouts)]
    big = max(cap) + 7  # (every place takes the largest capacity, gaps of 7 between)
    # a call without any optimised frame gives numpy_jpeg_ref's streams ...
    rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, frames, [(13 + b * big, cap[b], quals[b], layouts[b]) for b in range(6)])
    assert rc == 0, L.lib().lr_last_error()
    for b in range(6):
        same(dst[13 + b * big:13 + b * big + int(sizes[b])].tobytes(), plain[b], "frame %d without: " % b)
    # ... and so do those frames among optimised ones, whichever way the two kinds are arranged
    for flags, order in (([1, 0, 1, 1, 0, 0], [0, 1, 2, 3, 4, 5]), ([0, 1, 0, 0, 1, 1], [5, 3, 0, 4, 2, 1]), ([1] * 6, [2, 0, 1, 5, 4, 3])):
        fr = [frames[b] for b in order]
        rows = [(13 + i * big, cap[b], quals[b], layouts[b] + OPT * flags[b]) for i, b in enumerate(order)]
        rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, fr, rows)
        assert rc == 0, L.lib().lr_last_error()
        for i, b in enumerate(order):
            want = optimised[b] if flags[b] else plain[b]
            same(dst[rows[i][0]:rows[i][0] + int(sizes[i])].tobytes(), want, "frame %d (%s): " % (b, "with" if flags[b] else "without"))
        assert_only_extents_written(dst, [(rows[i][0], int(sizes[i])) for i in range(6)])
    # one-component frames, mixed
    gray = [textured(w, h, 40 + b, "u8") for b, (w, h) in enumerate(shapes[:3])]
    rows = [(30000 * b + 1, 29999, 80, OPT * (b != 1)) for b in range(3)]
    rc, sizes, dst = raw_call(L, ctx, L.PIX_U8, gray, rows)
    assert rc == 0, L.lib().lr_last_error()
    for b in range(3):
        want = R.encode(gray[b], 80, 0) if b == 1 else O.encode(gray[b], 80, 0)
        same(dst[rows[b][0]:rows[b][0] + int(sizes[b])].tobytes(), want, "gray frame %d: " % b)


@pytest.mark.parametrize("kind", KINDS)
def test_the_decoder_gets_the_same_pixels(L, ctx, kind):
    img = textured(203, 117, 51, kind)
    optimised, plain = one(L, ctx, img, 95, kind), one(L, ctx, img, 95, kind, optimize=False)
    assert len(optimised) < len(plain)
    a, b = ctx.decode_jpeg(optimised), ctx.decode_jpeg(plain)
    assert a.shape == b.shape and a.tobytes() == b.tobytes()


def test_sizes_capacity_and_guard_bytes(L, ctx):
    frames = [textured(64, 48, 50 + b, "444") for b in range(3)]
    want = [O.encode(f, 90, 1) for f in frames]
    for short in (len(want[1]) - 1, 500, 100, 1, 0):  # the EOI, an interval, the header cut; nothing at all
        rows = [(10, len(want[0]), 90, 1 + OPT), (10000, short, 90, 1 + OPT), (20000, len(want[2]) + 50, 90, 1 + OPT)]
        rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, frames, rows)
        assert rc == 0, L.lib().lr_last_error()
        assert sizes.tolist() == [len(s) for s in want], "sizes report the need"
        assert dst[10:10 + len(want[0])].tobytes() == want[0] and dst[20000:20000 + len(want[2])].tobytes() == want[2]
        assert_only_extents_written(dst, [(10, len(want[0])), (10000, short), (20000, len(want[2]))])


@pytest.mark.parametrize("kind", KINDS)
def test_the_bound_suffices_for_noise_at_quality_100(L, ctx, kind):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (40, 48) if kind == "u8" else (40, 48, 3), dtype=np.uint8)
    got = one(L, ctx, img, 100, kind)  # (asserts the length against jpeg_bound(optimize=True))
    same(got, O.encode(img, 100, layout_of(kind)))
    assert b"\xFF\x00" in got[got.index(b"\xFF\xDA"):], "the case has stuffed bytes"


def test_a_second_call_counts_from_zero(L, ctx):
    a, b = textured(130, 90, 70, "420"), textured(90, 130, 71, "420")
    same(one(L, ctx, a, 92, "420"), O.encode(a, 92, 0))
    same(one(L, ctx, b, 92, "420"), O.encode(b, 92, 0))
    same(one(L, ctx, a, 92, "420"), O.encode(a, 92, 0))
    ctx.trim()
    same(one(L, ctx, b, 92, "420"), O.encode(b, 92, 0))


def test_the_table_check(L, ctx):
    frames = [textured(40, 24, 60, "420"), textured(24, 40, 61, "420")]
    rows = [(0, 4000, 90, OPT), (5000, 4000, 90, 0)]
    for value in (2, 32, 18, 16.5, 15):
        rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, frames, rows, poke=[(1, 7, value)])
        assert rc != 0 and (dst == SENTINEL).all() and (sizes == 0xDEADBEEF).all(), value
        assert L.lib().lr_last_error().decode().startswith(PREFIX + "frame 1: entry [7]"), value
    gray = [f[..., 0].copy() for f in frames]
    for value in (17, 1, 2, 32):
        rc, sizes, dst = raw_call(L, ctx, L.PIX_U8, gray, rows, poke=[(1, 7, value)])
        assert rc != 0 and (dst == SENTINEL).all() and (sizes == 0xDEADBEEF).all(), value
        assert L.lib().lr_last_error().decode().startswith(PREFIX + "frame 1: entry [7]"), value
    # ... and the call after them is right
    rc, sizes, dst = raw_call(L, ctx, L.PIX_U8X3, frames, rows, poke=[(1, 7, 17)])
    assert rc == 0, L.lib().lr_last_error()
    same(dst[:int(sizes[0])].tobytes(), O.encode(frames[0], 90, 0))
    same(dst[5000:5000 + int(sizes[1])].tobytes(), O.encode(frames[1], 90, 1))


def detector_frame(w, h, seed):
    from librectify_amd import synth

    g = np.clip(synth.frame(w, h, seed, bars=40) * 255.0, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))


def test_python_keywords(L, ctx):
    from PIL import Image

    pixels = lambda s: np.asarray(Image.open(io.BytesIO(s)))  # noqa: E731
    frames = [textured(130, 90, 80, "420"), textured(17, 33, 81, "420")]
    got, plain = ctx.encode_jpeg_batch(frames, 95, optimize=True), ctx.encode_jpeg_batch(frames, 95)
    for f, g, p in zip(frames, got, plain):
        same(g, O.encode(f, 95, 0))
        assert len(g) < len(p) and (pixels(g) == pixels(p)).all()
    assert ctx.encode_jpeg(frames[0][..., 0].copy(), 80, optimize=True) == O.encode(frames[0][..., 0], 80, 0)
    ctx.jpeg_first_capacity = 300  # (every frame's first extent is too small: the second pass keeps the option)
    try:
        assert ctx.encode_jpeg_batch(frames, 95, optimize=True) == got
    finally:
        ctx.jpeg_first_capacity = None
    frame = next(f for f in (detector_frame(160, 120, 3 + b) for b in range(4)) if ctx.rectify(f)[2] is not None)
    lines, t, warped = ctx.rectify(frame)
    a, b = ctx.rectify(frame, jpeg=95, jpeg_optimize=True), ctx.rectify(frame, jpeg=95)
    assert a[0].tobytes() == lines.tobytes() and bytes(a[1]) == bytes(t)
    same(a[2], O.encode(warped, 95, 0))
    assert len(a[2]) < len(b[2]) and (pixels(a[2]) == pixels(b[2])).all()
    batch = ctx.rectify_batch([frame, frame[:100].copy()], jpeg=95, jpeg_optimize=True)
    assert batch[0][2] == a[2]
    drawn = ctx.draw_lines_batch([frame], [lines], jpeg=90, jpeg_optimize=True)
    assert drawn == [O.encode(ctx.draw_lines_batch([frame], [lines])[0], 90, 0)]
    for call in (lambda: ctx.rectify(frame, jpeg_optimize=True), lambda: ctx.rectify_batch([frame], jpeg_optimize=True),
                 lambda: ctx.draw_lines_batch([frame], [lines], jpeg_optimize=True)):
        with pytest.raises(ValueError):
            call()


def flat_stream(w, h):
    """the optimised stream of a one-component frame of 128s, put together by hand: every table has one symbol (DC category 0,
    EOB) and the code 0 of one bit, a block is the two bits 00, an interval of 96 blocks 24 zero bytes"""
    one = ([1] + [0] * 15, [0])
    n_blocks = (-(-w // 8)) * (-(-h // 8))
    n_int = -(-n_blocks // 96)
    out = [O.header(w, h, 95, 0, 1, [(one, one)])]
    for i in range(n_int):
        bits = 2 * min(96, n_blocks - 96 * i)
        padn = -bits % 8
        out.append((((1 << padn) - 1)).to_bytes((bits + padn) // 8, "big"))
        if i != n_int - 1:
            out.append(bytes([0xFF, 0xD0 + (i & 7)]))
    return b"".join(out + [b"\xFF\xD9"])


@pytest.mark.parametrize("height", [16376, 16384], ids=["below_2^22_symbols", "2^22_symbols"])
def test_the_key_width_threshold_of_the_tables_kernel(L, ctx, height):
    """jpeg_tables_kernel merges with 32-bit keys while a table's counts (the pseudo-symbol's 1 among them) sum below 2^22
    and with 64-bit keys from there: a flat 16384 x 16384 frame has exactly 2^22 blocks, so 2^22 + 1 in both of its tables;
    eight rows fewer stay below.  The expected stream is written down by hand (flat_stream, checked here against the
    reference on a small frame): the reference's Python loop over four million blocks would take minutes."""
    small = np.full((104, 200), 128, np.uint8)
    assert flat_stream(200, 104) == O.encode(small, 95, 0)
    w = 16384
    assert ((w // 8) * (height // 8) + 1 >= 1 << 22) == (height == 16384)
    want = flat_stream(w, height)
    cap = len(want) + 100  # (lr_jpeg_bound would be 1.7 GB; the need is reported whatever the capacity)
    rc, sizes, dst = raw_call(L, ctx, L.PIX_U8, [np.full((height, w), 128, np.uint8)], [(16, cap, 95, OPT)])
    assert rc == 0, L.lib().lr_last_error()
    assert int(sizes[0]) == len(want)
    same(dst[16:16 + len(want)].tobytes(), want)
    assert_only_extents_written(dst, [(16, len(want))])
    ctx.trim()  # (the coefficients of 268 M samples go back)
