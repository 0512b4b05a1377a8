"""The packed warp (lr_warp_perspective_device with LR_WARP_PACKED: every frame its own output size and place, one
launch) against tests/numpy_warp_ref.py, bit for bit, and against the uniform launch that existed before it; its clean
failures; Context.rectify_batch against a loop of Context.rectify; rectify_batch_device on resident frames."""
import ctypes as C
import os

import numpy as np
import pytest

import numpy_warp_ref as R
from test_gpu_rectify_warp import BPP, DTYPE, assert_same, frame, maps, synthetic_rgb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SENTINEL = 0xAB


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


def upload_frames(ctx, frames, fmt, pad, gap):
    """frames of one shape with rows `pad` bytes longer than their pixels and `gap` bytes between frames"""
    bpp = BPP[fmt]
    h, w = frames[0].shape[:2]
    srow = w * bpp + pad
    simg = h * srow + gap
    buf = np.full(len(frames) * simg, 0x5A, np.uint8)
    for b, f in enumerate(frames):
        buf[b * simg: b * simg + h * srow].reshape(h, srow)[:, : w * bpp] = np.ascontiguousarray(f).reshape(h, -1).view(np.uint8)
    return ctx.device_upload(buf), simg, srow


def cut(buf, row, fmt):
    """frame of table row `row` out of the downloaded region"""
    bpp = BPP[fmt]
    ow, oh, off, stride = (int(v) for v in row[9:])
    rows = np.lib.stride_tricks.as_strided(buf[off:], (oh, ow * bpp), (stride, 1))
    return np.ascontiguousarray(rows).view(DTYPE[fmt]).reshape((oh, ow, 3) if fmt == 1 else (oh, ow))


def written_mask(n, table, bpp):
    m = np.zeros(n, bool)
    for row in table:
        ow, oh, off, stride = (int(v) for v in row[9:])
        for y in range(oh):
            m[off + y * stride: off + y * stride + ow * bpp] = True
    return m


W, H = 257, 131
SIZES = [(1, 1), (63, 17), (64, 16), (65, 17), (400, 300), (200, 150), (130, 40)]
KINDS = ["identity", "horizon", "tiny_w0_nan", "perspective", "rotation", "scale_up", "w0_zero_row"]
ORDER = [4, 0, 6, 2, 5, 1, 3]  # the frames' places in the region, first to last


def seven_frames_table(fmt):
    """Seven frames with their own maps and sizes, placed out of frame order, with gaps, padded strides and (8-bit) odd
    offsets and strides.  Returns (table, region bytes)."""
    bpp = BPP[fmt]
    table = np.zeros((7, 13))
    cursor = 8 if fmt == 2 else 5
    for k, b in enumerate(ORDER):
        ow, oh = SIZES[b]
        pad = (4, 12, 0)[k % 3] if fmt == 2 else (1, 4, 0, 7)[k % 4]
        stride = ow * bpp + pad
        table[b, :9] = maps(W, H, ow, oh)[KINDS[b]].reshape(-1)
        table[b, 9:] = (ow, oh, cursor, stride)
        cursor += (oh - 1) * stride + ow * bpp + ((4, 0, 20)[k % 3] if fmt == 2 else (3, 0, 10)[k % 3])
    if fmt != 2:
        assert (table[:, 11] % 2 == 1).any() and (table[:, 12] % 2 == 1).any()
    return table, cursor + 9


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_packed_warp_bit_exact_and_writes_nothing_else(L, ctx, fmt):
    frames = [frame(fmt, W, H, 100 + b) for b in range(7)]
    table, region = seven_frames_table(fmt)
    d_src, simg, srow = upload_frames(ctx, frames, fmt, 4 if fmt == 2 else 1, 4 if fmt == 2 else 7)
    d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    d_uni = None
    try:
        ctx.warp_perspective_packed_device(d_src, simg, 7, W, H, srow, fmt, table, d_dst, region)
        got = ctx.device_download(d_dst, (region,), np.uint8)
        # the way that existed before: one launch at the largest size, cropped
        mw, mh = max(s[0] for s in SIZES), max(s[1] for s in SIZES)
        bpp = BPP[fmt]
        d_uni = ctx.device_upload(np.zeros(7 * mw * mh * bpp, np.uint8))
        ctx.warp_perspective_device(d_src, simg, 7, W, H, srow, fmt, table[:, :9].copy(), d_uni, mw * mh * bpp, mw, mh, mw * bpp)
        uni = ctx.device_download(d_uni, (7, mh, mw * bpp), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
        if d_uni:
            ctx.device_free(d_uni)
    mask = written_mask(region, table, BPP[fmt])
    assert (got[~mask] == SENTINEL).all(), "bytes outside the frames' pixel rows were written"
    for b in range(7):
        ow, oh = SIZES[b]
        out = cut(got, table[b], fmt)
        assert_same(out, R.warp(frames[b], table[b, :9], ow, oh)), KINDS[b]
        crop = np.ascontiguousarray(uni[b, :oh, : ow * bpp]).view(DTYPE[fmt]).reshape(out.shape)
        assert_same(out, crop)
    assert_same(cut(got, table[0], fmt), frames[0][:1, :1])  # (identity)


# one tile, exactly one tile, one pixel over in each direction (four tiles, a partial lane at the right edge): six tiles in
# all, so some XCDs' runs are empty; together and each as a batch of one
EDGE_SIZES = [(1, 1), (64, 16), (65, 17)]
EDGE_KINDS = ["identity", "perspective", "rotation"]
EDGE_BATCHES = [(0, 1, 2), (0,), (1,), (2,)]


def edge_table(fmt, which, w=W, h=H):
    """the frames `which` of EDGE_SIZES one after the other, with gaps, padded strides and (8-bit) an odd offset"""
    bpp = BPP[fmt]
    table = np.zeros((len(which), 13))
    cursor = 8 if fmt == 2 else 5
    for k, s in enumerate(which):
        ow, oh = EDGE_SIZES[s]
        stride = ow * bpp + ((4, 12, 0)[k] if fmt == 2 else (1, 4, 0)[k])
        table[k, :9] = maps(w, h, ow, oh)[EDGE_KINDS[s]].reshape(-1)
        table[k, 9:] = (ow, oh, cursor, stride)
        cursor += (oh - 1) * stride + ow * bpp + (4 if fmt == 2 else 3)
    return table, cursor + 9


@pytest.mark.parametrize("which", EDGE_BATCHES)
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_packed_warp_of_a_few_tiles(L, ctx, fmt, which):
    w, h = 70, 20
    frames = [frame(fmt, w, h, 100 + b) for b in which]
    table, region = edge_table(fmt, which, w, h)
    d_src, simg, srow = upload_frames(ctx, frames, fmt, 4 if fmt == 2 else 1, 4 if fmt == 2 else 7)
    d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    try:
        ctx.warp_perspective_packed_device(d_src, simg, len(which), w, h, srow, fmt, table, d_dst, region)
        got = ctx.device_download(d_dst, (region,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    assert (got[~written_mask(region, table, BPP[fmt])] == SENTINEL).all(), "bytes outside the frames' pixel rows were written"
    for k, s in enumerate(which):
        assert_same(cut(got, table[k], fmt), R.warp(frames[k], table[k, :9], *EDGE_SIZES[s])), EDGE_KINDS[s]


def test_packed_warp_large_frames(L, ctx):
    """Three 3840 x 2160 u8x3 frames, one of them at the full 3w x 3h: the whole images against the single-frame launch,
    bands of rows against the second source."""
    w, h = 3840, 2160
    frames = [frame(1, w, h, 50 + b) for b in range(3)]
    sizes = [(3840, 2160), (3 * w, 3 * h), (5001, 3001)]
    Ms = np.stack([maps(w, h, ow, oh)[k] for (ow, oh), k in zip(sizes, ("rotation", "scale_up", "perspective"))])
    Ms[1] = np.array([[1 / 3.0, 0.01, 0.0], [0.0, 1 / 3.0, 0.0], [0.0, 0.0, 1.0]])
    table, total = L.warp_table(Ms, sizes, 3, align=4)
    d_src = ctx.device_upload(np.stack(frames))
    p = C.c_void_p()
    assert L.lib().lr_device_malloc(ctx._h, total, C.byref(p)) == 0, L.lib().lr_last_error()
    d_dst = p.value
    d_one = None
    try:
        ctx.warp_perspective_packed_device(d_src, w * h * 3, 3, w, h, w * 3, 1, table, d_dst, total)
        got = ctx.device_download(d_dst, (total,), np.uint8)
        for b, (ow, oh) in enumerate(sizes):
            d_one = ctx.device_upload(np.zeros(ow * oh * 3, np.uint8))
            ctx.warp_perspective_device(d_src + b * w * h * 3, w * h * 3, 1, w, h, w * 3, 1, Ms[b], d_one, ow * oh * 3, ow, oh, ow * 3)
            one = ctx.device_download(d_one, (oh, ow, 3), np.uint8)
            ctx.device_free(d_one)
            d_one = None
            out = cut(got, table[b], 1)
            np.testing.assert_array_equal(out, one)
            rows = np.concatenate([np.arange(0, 17), np.arange(oh // 2 - 8, oh // 2 + 9), np.arange(oh - 17, oh)])
            exp = R.warp(frames[b], Ms[b], ow, oh, rows=rows)
            assert exp.any()
            np.testing.assert_array_equal(out[rows], exp)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
        if d_one:
            ctx.device_free(d_one)


def test_packed_frame_beyond_4_gib(L, ctx):
    """The second frame's output starts past 4 GiB from the destination pointer."""
    w, h = 300, 200
    frames = [frame(1, w, h, 70 + b) for b in range(2)]
    sizes = [(333, 77), (401, 203)]
    table = np.zeros((2, 13))
    far = 2**32 + 12345
    for b, (ow, oh) in enumerate(sizes):
        table[b, :9] = maps(w, h, ow, oh)["perspective" if b else "rotation"].reshape(-1)
        table[b, 9:] = (ow, oh, far if b else 3, ow * 3 + 5)
    n_near, n_far = 3 + 77 * (333 * 3 + 5) + 64, 64 + 203 * (401 * 3 + 5) + 64  # the frames' rows and 64 bytes around them
    total = far - 64 + n_far
    p = C.c_void_p()
    assert L.lib().lr_device_malloc(ctx._h, total, C.byref(p)) == 0, L.lib().lr_last_error()
    d_dst = p.value
    d_src = ctx.device_upload(np.stack(frames))
    try:
        for base, n in ((d_dst, n_near), (d_dst + far - 64, n_far)):  # a sentinel around the two frames
            assert L.lib().lr_memcpy_h2d(ctx._h, C.c_void_p(base), P(np.full(n, SENTINEL, np.uint8)), n) == 0
        ctx.warp_perspective_packed_device(d_src, w * h * 3, 2, w, h, w * 3, 1, table, d_dst, total)
        near = ctx.device_download(d_dst, (n_near,), np.uint8)
        blk = ctx.device_download(d_dst + far - 64, (n_far,), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    local = table.copy()
    local[1, 11] = 64  # (the far block starts 64 bytes before the frame)
    for b, buf in enumerate((near, blk)):
        ow, oh = sizes[b]
        np.testing.assert_array_equal(cut(buf, local[b], 1), R.warp(frames[b], table[b, :9], ow, oh))
        mask = written_mask(len(buf), local[b: b + 1], 3)
        assert (buf[~mask] == SENTINEL).all()


def test_packed_failures_are_clean(L, ctx):
    lib = L.lib()
    w, h, B = 64, 48, 3
    src = [frame(1, w, h, 30 + b) for b in range(B)]
    d_src = ctx.device_upload(np.stack(src))
    sizes = [(70, 20), (9, 33), (64, 48)]
    Ms = np.stack([maps(w, h, ow, oh)[k] for (ow, oh), k in zip(sizes, ("shift", "rotation", "identity"))])
    good, total = L.warp_table(Ms, sizes, 3, align=1)
    region = 1 << 16
    assert total + 100 < region
    d_dst = ctx.device_upload(np.full(region, SENTINEL, np.uint8))
    d_many = ctx.device_upload(np.zeros(17 * 64, np.uint8))
    fmt = L.PIX_U8X3 | L.WARP_PACKED

    def call(table=good, batch=B, fmt=fmt, dst=None, dst_bytes=region, ow=70, oh=48, drow=0, src=None, sib=w * h * 3, srow=w * 3, sw=w, sh=h):
        t = np.ascontiguousarray(table, np.float64)
        return lib.lr_warp_perspective_device(ctx._h, C.c_void_p(src or d_src), sib, batch, sw, sh, srow, fmt, P(t),
                                              C.c_void_p(dst or d_dst), dst_bytes, ow, oh, drow)

    def changed(b, k, v):
        t = good.copy()
        t[b, k] = v
        return t

    overlap = good.copy()
    overlap[1, 11] = good[0, 11] + good[0, 12] * 3  # inside frame 0's rows
    interleaved = good.copy()  # frame 1 in the row padding of a wide-strided frame 0: extents overlap all the same
    interleaved[0, 12], interleaved[0, 11] = 400, 0
    interleaved[1, 11], interleaved[1, 12] = 250, 400
    interleaved[2, 11] = 400 * 40
    many = np.zeros((17, 13))
    many[:, :9] = np.eye(3).reshape(-1)
    many[:, 9], many[:, 10], many[:, 12] = 1, 2**31 - 1, 1
    many[:, 11] = np.arange(17) * 2.0**31
    # the same bytes read as 16 x 48 f32 frames, with a table that is right for them
    f32, f32_total = L.warp_table(Ms, [(16, 20), (9, 33), (16, 48)], 4, align=4)
    assert f32_total <= region
    f32_call = dict(fmt=L.PIX_F32 | L.WARP_PACKED, sw=16, srow=w * 3, ow=16)

    def changed_f32(k):
        t = f32.copy()
        t[1, k] += 2
        return t

    cases = {
        "width not integral": dict(table=changed(0, 9, 10.5)),
        "height 0": dict(table=changed(1, 10, 0)),
        "width NaN": dict(table=changed(1, 9, np.nan)),
        "width above the bound": dict(ow=69),
        "height above the bound": dict(oh=47),
        "offset negative": dict(table=changed(0, 11, -1)),
        "offset not integral": dict(table=changed(2, 11, good[2, 11] + 0.5)),
        "offset infinite": dict(table=changed(2, 11, np.inf)),
        "offset beyond 2^53": dict(table=changed(2, 11, 2.0**60), dst_bytes=2**62),
        "stride shorter than a row": dict(table=changed(0, 12, 70 * 3 - 1)),
        "stride not integral": dict(table=changed(1, 12, 27.25)),
        "stride NaN": dict(table=changed(1, 12, np.nan)),
        "map NaN": dict(table=changed(1, 4, np.nan)),
        "map infinite": dict(table=changed(2, 8, -np.inf)),
        "frame outside the region": dict(dst_bytes=total - 1),
        "frames overlap": dict(table=overlap),
        "frames interleaved": dict(table=interleaved),
        "more than 2^31 tiles": dict(table=many, batch=17, fmt=L.PIX_U8 | L.WARP_PACKED, src=d_many, sib=64, srow=8, sw=8, sh=8,
                                     dst_bytes=2**36, ow=1, oh=2**31 - 1),
        "packed and prepare": dict(fmt=fmt | L.WARP_PREPARE),
        "another option bit": dict(fmt=fmt | 0x400),
        "a high option bit": dict(fmt=fmt | 0x10000),
        "dst_row_bytes not 0": dict(drow=70 * 3),
        "batch 0": dict(batch=0),
        "null destination": dict(dst=-1),
        "unknown pixel format": dict(fmt=3 | L.WARP_PACKED),
        "f32 offset not a multiple of 4": dict(table=changed_f32(11), **f32_call),
        "f32 stride not a multiple of 4": dict(table=changed_f32(12), **f32_call),
        "f32 destination misaligned": dict(table=f32, dst="odd", **f32_call),
    }
    try:
        for name, kw in cases.items():
            kw = dict(kw)
            if kw.get("dst") == -1:
                rc = lib.lr_warp_perspective_device(ctx._h, C.c_void_p(d_src), w * h * 3, B, w, h, w * 3, fmt, P(good), None, region, 70, 48, 0)
            else:
                if kw.get("dst") == "odd":
                    kw["dst"] = d_dst + 2
                rc = call(**kw)
            msg = lib.lr_last_error().decode()
            assert rc != 0, name
            assert msg.startswith("lr_warp_perspective_device") and len(msg) > len("lr_warp_perspective_device: "), (name, msg)
            assert (ctx.device_download(d_dst, (region,), np.uint8) == SENTINEL).all(), name
        # the f32 table the three f32 cases start from is itself accepted
        assert call(table=f32, **f32_call) == 0, lib.lr_last_error()
        ctx.synchronize()
        assert L.lib().lr_memcpy_h2d(ctx._h, C.c_void_p(d_dst), P(np.full(region, SENTINEL, np.uint8)), region) == 0

        def valid():
            assert call() == 0, lib.lr_last_error()
            got = ctx.device_download(d_dst, (region,), np.uint8)
            for b, (ow, oh) in enumerate(sizes):
                np.testing.assert_array_equal(cut(got, good[b], 1), R.warp(src[b], Ms[b], ow, oh))
            assert (got[~written_mask(region, good, 3)] == SENTINEL).all()

        assert call(table=overlap) != 0
        valid()  # the next valid call on the same context
        ctx.trim()
        valid()
        ctx.trim()
        ctx.warp_perspective_device(d_src, w * h * 3, 1, w, h, w * 3, 1, np.eye(3), d_dst, region, w, h, w * 3)  # and the plain warp
        np.testing.assert_array_equal(ctx.device_download(d_dst, (h, w, 3), np.uint8), src[0])
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
        ctx.device_free(d_many)


# ---- rectify_batch ---------------------------------------------------------------------------------------------

def gray_frame(w, h, seed):
    from librectify_amd import synth

    return np.clip(synth.frame(w, h, seed) * 255.0, 0, 255).astype(np.uint8)


def same_results(got, want, what):
    assert len(got) == len(want)
    for b, (g, w_) in enumerate(zip(got, want)):
        assert len(g[0]) == len(w_[0]) and g[0].tobytes() == w_[0].tobytes(), "%s: frame %d: lines" % (what, b)
        np.testing.assert_array_equal(g[1].as_array(), w_[1].as_array(), "%s: frame %d: transform" % (what, b))
        assert bytes(g[1]) == bytes(w_[1]), "%s: frame %d: transform" % (what, b)
        assert g[2] is not None and g[2].shape == w_[2].shape and g[2].dtype == np.uint8, "%s: frame %d" % (what, b)
        np.testing.assert_array_equal(g[2], w_[2], "%s: frame %d: image" % (what, b))


SETTINGS = [
    dict(), dict(max_size=300), dict(refine=True), dict(max_size=300, refine=True),
    dict(clip=1.5, cfg="other"), dict(max_size=300, clip=1.5, cfg="other"),
]


def _kw(L, kw):
    kw = dict(kw)
    if kw.get("cfg") == "other":
        kw["cfg"] = L.RectificationConfig(tol=30.0, vmin=2.5, v_strategy=L.RECTIFY, hmin=3.0, h_strategy=L.ROTATE_H)
    return kw


@pytest.mark.parametrize("colour", [True, False])
def test_rectify_batch_equals_a_loop_of_rectify(L, ctx, colour):
    if colour:
        frames = np.stack([synthetic_rgb(480, 360, 3 + b) for b in range(5)])
    else:
        frames = np.stack([gray_frame(777, 401, 4 + b) for b in range(5)])
    for s in SETTINGS:
        kw = _kw(L, s)
        want = [ctx.rectify(f, **kw) for f in frames]
        assert all(len(x[0]) > 10 for x in want)
        same_results(ctx.rectify_batch(frames, **kw), want, str(s))
        if not s:
            assert len({x[2].shape for x in want}) > 1, "the frames' output sizes differ"
            same_results(ctx.rectify_batch([np.array(f) for f in frames]), want, "a list of frames")
            # a first detector pass with too small a capacity still returns every line
            assert max(len(x[0]) for x in want) > 8
            same_results(ctx.rectify_batch(frames, capacity=8), want, "capacity 8")


def test_rectify_batch_golden_picture_with_copies_of_itself(L, ctx):
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    for kw in (dict(), dict(max_size=300)):
        one = ctx.rectify(gray, **kw)
        same_results(ctx.rectify_batch(np.stack([gray] * 3), **kw), [one] * 3, str(kw))


def test_rectify_batch_device_on_resident_frames(L, ctx, monkeypatch):
    frames = np.stack([synthetic_rgb(480, 360, 3 + b) for b in range(4)])
    lib = L.lib()
    live = {}
    real_malloc, real_free = lib.lr_device_malloc, lib.lr_device_free

    def malloc(h, n, ref):
        rc = real_malloc(h, n, ref)
        if rc == 0:
            live[ref._obj.value] = n
        return rc

    def free(h, p):
        live.pop(p.value, None)
        return real_free(h, p)

    for kw in (dict(), dict(max_size=300, refine=True)):
        want = ctx.rectify_batch(frames, **kw)
        d = ctx.device_upload(frames)
        monkeypatch.setattr(lib, "lr_device_malloc", malloc)
        monkeypatch.setattr(lib, "lr_device_free", free)
        try:
            live.clear()
            lines, tfs, table, d_out, total = ctx.rectify_batch_device(d, 4, 480, 360, L.PIX_U8X3, **kw)
            assert list(live) == [d_out] and live[d_out] == total, "nothing but d_out is left allocated"
            for _ in range(20):
                r = ctx.rectify_batch_device(d, 4, 480, 360, L.PIX_U8X3, **kw)
                ctx.device_free(r[3])
            assert list(live) == [d_out]
            got = ctx.device_download(d_out, (total,), np.uint8)
            ctx.device_free(d_out)
            assert not live
        finally:
            monkeypatch.undo()
            ctx.device_free(d)
        assert table.shape == (4, 13) and total == int(table[3, 11] + (table[3, 10] - 1) * table[3, 12] + table[3, 9] * 3)
        for b in range(4):
            assert lines[b].tobytes() == want[b][0].tobytes() and bytes(tfs[b]) == bytes(want[b][1])
            np.testing.assert_array_equal(cut(got, table[b], 1), want[b][2])


def test_a_frame_without_a_rectification_gets_none(L, ctx, monkeypatch):
    """Frame 2's transform is replaced by one with three collinear corners (built and tried on the CPU first), as both
    rectify and rectify_batch get it from compute_rectification_transform: rectify raises for that frame, the batch gives
    None for it and the others' images are what they were.  With a clip that leaves no pixel, every frame is None."""
    frames = np.stack([gray_frame(640, 480, 40 + b) for b in range(4)])
    plain = [ctx.rectify(f) for f in frames]
    assert len({x[0].tobytes() for x in plain}) == 4
    flat = L.ImageTransform()
    flat.width, flat.height = 640, 480
    flat.top_left, flat.top_right, flat.bottom_left, flat.bottom_right = [L.Point(x, y, 0.0) for x, y in ((0, 0), (320, 240), (640, 480), (640, 0))]
    with pytest.raises(L.LibrectifyError):
        L.rectification_homography(flat, 3.0)
    real = L.compute_rectification_transform
    marked = plain[2][0].tobytes()

    def transform(lines, width, height, cfg=None):
        return flat if np.ascontiguousarray(lines, L.LINE_DTYPE).tobytes() == marked else real(lines, width, height, cfg)

    monkeypatch.setattr(L, "compute_rectification_transform", transform)
    with pytest.raises(L.LibrectifyError):
        ctx.rectify(frames[2])
    got = ctx.rectify_batch(frames)
    assert got[2][2] is None and got[2][0].tobytes() == marked and bytes(got[2][1]) == bytes(flat)
    same_results([got[b] for b in (0, 1, 3)], [plain[b] for b in (0, 1, 3)], "the frames beside it")
    d = ctx.device_upload(frames)
    try:
        _, _, table, d_out, total = ctx.rectify_batch_device(d, 4, 640, 480, L.PIX_U8)
        packed = ctx.device_download(d_out, (total,), np.uint8)
        ctx.device_free(d_out)
    finally:
        ctx.device_free(d)
    assert not table[2].any() and (table[[0, 1, 3], 9] >= 1).all()
    for b in (0, 1, 3):
        np.testing.assert_array_equal(cut(packed, table[b], 0), plain[b][2])
    monkeypatch.undo()
    # a size below 1: no frame has an image, the lines and transforms are returned all the same
    with pytest.raises(L.LibrectifyError):
        L.rectification_homography(plain[0][1], 1e-4)
    none = ctx.rectify_batch(frames, clip=1e-4)
    assert all(x[2] is None for x in none)
    for b in range(4):
        assert none[b][0].tobytes() == plain[b][0].tobytes() and bytes(none[b][1]) == bytes(plain[b][1])


def test_rectify_batch_prescaled_frames_are_ready_before_the_detector_reads_them(L, ctx):
    """Sixteen 1920 x 1080 frames with max_size=900: the batched prepare writes 16 frames of 900 x 507 on the context's stream
    and the batch detector reads them on its lanes' streams, so it must not start before the prepare has ended (at this
    size a detector that started early saw a frame half written and reported other lines for it)."""
    base = [gray_frame(1920, 1080, 60 + b) for b in range(2)]
    frames = np.stack([np.roll(base[b % 2], (7 * b, 13 * b), (0, 1)) for b in range(16)])
    want = [ctx.rectify(f, max_size=900) for f in frames]
    for _ in range(3):
        same_results(ctx.rectify_batch(frames, max_size=900), want, "max_size=900")
