"""8-bit frames in the detector (u8 gray, u8x3 interleaved; host or HBM) against the fp32 path.

The definition is p = float(luma) * (1/256.f), exact, then the detector on p.  So the
expected value of every test here is what the fp32 path gives on the fp32 frame p, computed IN THE SAME TEST through
the fp32 twin of the entry under test (and, for the doc image, the oracle on p), and the comparison is equality:
records as raw bytes, counts, transforms, lr_stage_counters [0, 1, 3] and -- after single-frame calls -- the dx, dy
and label planes and the seed lists that lr_download serves.  No tolerance anywhere.

Every test reaches the C ABI through what the feature added to the mirror (FRAMES_*, frames_word, fmt=, uint8
arrays): without the feature they fail in Python, before any device call could read a quarter-sized buffer as fp32.
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L

    # the feature's own names, before anything touches the device: an AttributeError here is "the library has no 8-bit frames"
    assert (L.FRAMES_U8, L.FRAMES_U8X3, L.FRAMES_F32) == (0x100, 0x200, 0x300)
    assert L.frames_word(L.PIX_U8, True) == 0x101
    L.lib()
    assert L.device_count() > 0, "GPU tests need a GPU"
    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.set_seed(0)
    yield c
    c.close()


# ---- frames ----------------------------------------------------------------------------------

def unit(frame):
    """p of an 8-bit frame: float32(luma) * float32(1 / 256)"""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8
    if frame.ndim == 3:
        c = frame.astype(np.uint32)
        luma = (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
    else:
        luma = frame
    return np.ascontiguousarray(luma.astype(np.float32) * np.float32(1.0 / 256.0))


def quantise(img):
    return np.clip(np.floor(np.asarray(img, np.float64) * 256.0 + 0.5), 0, 255).astype(np.uint8)


def gray_frame(w, h, seed):
    from librectify_amd import synth

    return quantise(synth.frame(w, h, seed, bars=max(2, (w * h) // 1500)))


def colour_frame(w, h, seed):
    """three different channels: bars of one seed, of another, and the first one shifted"""
    a, b = gray_frame(w, h, seed), gray_frame(w, h, seed + 1)
    return np.ascontiguousarray(np.stack([a, b, np.roll(a, 2, axis=1)], axis=2))


def make_frame(w, h, seed, colour):
    return colour_frame(w, h, seed) if colour else gray_frame(w, h, seed)


def fmt_of(L, frame):
    return L.PIX_U8X3 if frame.ndim == 3 else L.PIX_U8


def bpp_of(frame):
    return 3 if frame.ndim == 3 else 1


# ---- what a call leaves behind ------------------------------------------------------------------

def snapshot(L, ctx, lines, planes=True):
    """everything the last whole-path call on ctx left: records, counters [0, 1, 3] and, if asked, the planes behind them"""
    cnt = ctx.stage_counters()
    snap = dict(lines=np.ascontiguousarray(lines).tobytes(), n=len(lines),
                counters=(cnt["seeds"], cnt["components"], cnt["labelled_px"]))
    if planes:
        ctx.n_seeds = cnt["seeds"]
        for name, buf in (("dx", L.BUF_DX), ("dy", L.BUF_DY), ("label", L.BUF_LABEL), ("seed_idx", L.BUF_SEED_IDX),
                          ("seed_bin", L.BUF_SEED_BIN), ("seed_thr", L.BUF_SEED_THR)):
            snap[name] = ctx.download(buf).tobytes()
    return snap


def same(got, want, what):
    assert got["n"] == want["n"], "[%s] n_lines %d, the fp32 path's %d" % (what, got["n"], want["n"])
    assert got["counters"] == want["counters"], "[%s] counters %s, the fp32 path's %s" % (what, got["counters"], want["counters"])
    for k in want:
        if k not in ("n", "counters"):
            assert k in got and got[k] == want[k], "[%s] %s differs from the fp32 path's" % (what, k)


def upload_padded(ctx, frame, stride, base, pad=7):
    """the frame's rows `stride` pixels apart, `base` bytes into a device buffer full of `pad`: (allocation, frame address)"""
    h, w = frame.shape[:2]
    bpp = bpp_of(frame)
    buf = np.full(base + h * stride * bpp + 8, pad, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf[base:], (h, w * bpp), (stride * bpp, 1))
    rows[:] = frame.reshape(h, w * bpp)
    d = ctx.device_upload(buf)
    return d, d + base


def fp32_device(L, ctx, p, ml, refine=False, planes=True):
    h, w = p.shape
    d = ctx.device_upload(p)
    try:
        return snapshot(L, ctx, ctx.find_line_segment_groups_device(d, w, h, ml, refine=refine).copy(), planes)
    finally:
        ctx.device_free(d)


def min_len(w, h):
    return max(2.0, max(w, h) / 50.0)


# ---- 1 / 5: the device entry ---------------------------------------------------------------------

EDGE_SHAPES = list(itertools.product((5, 55, 56, 57, 113), (5, 29, 30, 31, 61)))


def _device_variants(L, ctx, frame, what):
    h, w = frame.shape[:2]
    ml = min_len(w, h)
    want = fp32_device(L, ctx, unit(frame), ml)
    for stride, base in ((w, 0), (w + 1, 1), (w + 3, 3), (w, 1)):
        d, at = upload_padded(ctx, frame, stride, base)
        try:
            got = ctx.find_line_segment_groups_device(at, w, h, ml, stride=stride, fmt=fmt_of(L, frame)).copy()
            same(snapshot(L, ctx, got), want, "%s stride %d base +%d" % (what, stride, base))
        finally:
            ctx.device_free(d)
    return want


def test_device_u8_at_the_tile_and_band_edges(L, ctx):
    assert len(EDGE_SHAPES) == 25
    found = 0
    for k, (w, h) in enumerate(EDGE_SHAPES):
        found += _device_variants(L, ctx, gray_frame(w, h, 900 + k), "u8 %dx%d" % (w, h))["counters"][0]
    assert found > 0, "no frame had a seed"


def test_device_u8_frame_inside_a_mosaic(L, ctx):
    mosaic = gray_frame(300, 200, 77)
    d = ctx.device_upload(mosaic)
    try:
        for (x, y, w, h) in ((37, 23, 113, 61), (1, 0, 57, 31), (187, 139, 113, 61)):
            frame = np.ascontiguousarray(mosaic[y:y + h, x:x + w])
            want = fp32_device(L, ctx, unit(frame), min_len(w, h))
            got = ctx.find_line_segment_groups_device(d + y * 300 + x, w, h, min_len(w, h), stride=300, fmt=L.PIX_U8).copy()
            same(snapshot(L, ctx, got), want, "u8 %dx%d at (%d, %d) of a 300x200 mosaic" % (w, h, x, y))
    finally:
        ctx.device_free(d)


def test_device_u8x3(L, ctx):
    for k, (w, h) in enumerate(((5, 5), (57, 31), (113, 61), (56, 30), (320, 240))):
        _device_variants(L, ctx, colour_frame(w, h, 940 + k), "u8x3 %dx%d" % (w, h))


# ---- 2 / 5: the host entry -----------------------------------------------------------------------

def _host_variants(L, ctx, frame, what, threads=(-1, 8)):
    h, w = frame.shape[:2]
    ml = min_len(w, h)
    p = unit(frame)
    wants = {}
    for nt in threads:
        wants[nt] = snapshot(L, ctx, ctx.find_line_segment_groups(p, ml, num_threads=nt))
    same(wants[threads[-1]], wants[threads[0]], what + " fp32 by threads")
    pinned = ctx.host_alloc(frame.shape, np.uint8)
    try:
        pinned[...] = frame
        padded = np.full((h, w + 5) + frame.shape[2:], 9, np.uint8)
        padded[:, :w] = frame
        for nt in threads:
            for name, src in (("pageable", frame), ("page-locked", pinned), ("row stride w + 5", padded[:, :w]),
                              ("negative stride", frame[::-1])):
                got = ctx.find_line_segment_groups(src, ml, num_threads=nt)
                same(snapshot(L, ctx, got), wants[nt], "%s, %s, num_threads %d" % (what, name, nt))
        # (the fp32 entry on the same rows addressed from the other end: no flip there either)
        same(snapshot(L, ctx, ctx.find_line_segment_groups(p[::-1], ml)), wants[threads[0]], what + " fp32 negative stride")
    finally:
        ctx.host_free(pinned)


def test_host_u8(L, ctx):
    for k, (w, h) in enumerate(((5, 5), (57, 31), (113, 61), (641, 479))):
        _host_variants(L, ctx, gray_frame(w, h, 960 + k), "u8 %dx%d" % (w, h))


def test_host_u8_frame_of_three_upload_bands(L, ctx):
    """4000 x 3000 bytes are 12 MB: three bands of 4 MB, the filter behind each"""
    _host_variants(L, ctx, gray_frame(4000, 3000, 970), "u8 4000x3000")


def test_host_u8x3(L, ctx):
    for k, (w, h) in enumerate(((57, 31), (641, 479))):
        _host_variants(L, ctx, colour_frame(w, h, 980 + k), "u8x3 %dx%d" % (w, h))
    _host_variants(L, ctx, colour_frame(4000, 3000, 985), "u8x3 4000x3000", threads=(8,))


# ---- 3: the refine word ----------------------------------------------------------------------------

def test_refine_word(L, ctx):
    from librectify_amd import _check, _ptr

    w, h = 641, 479
    frame = gray_frame(w, h, 990)
    p = unit(frame)
    ml = min_len(w, h)
    plain = fp32_device(L, ctx, p, ml, refine=False, planes=False)
    refined = fp32_device(L, ctx, p, ml, refine=True, planes=False)
    d8, dp = ctx.device_upload(frame), ctx.device_upload(p)
    try:
        for refine, want in ((False, plain), (True, refined)):
            got = ctx.find_line_segment_groups_device(d8, w, h, ml, refine=refine, fmt=L.PIX_U8).copy()
            same(snapshot(L, ctx, got, False), want, "FRAMES_U8 | %d" % refine)
            same(snapshot(L, ctx, ctx.find_line_segment_groups(frame, ml, refine=refine), False), want, "host FRAMES_U8 | %d" % refine)
            # the explicit fp32 word on the fp32 frame
            cap = h * w // 6 + 16
            out = np.zeros(cap, L.LINE_DTYPE)
            n = C.c_int(0)
            _check(L.lib().lr_find_line_segment_groups_device(ctx._h, C.c_void_p(dp), w, h, w, ml, L.FRAMES_F32 | int(refine), -1,
                                                              _ptr(out), cap, C.byref(n)))
            same(snapshot(L, ctx, out[: n.value], False), want, "FRAMES_F32 | %d" % refine)
            _check(L.lib().lr_find_line_segment_groups_host(ctx._h, _ptr(p), w, h, w, ml, L.FRAMES_F32 | int(refine), 8,
                                                            _ptr(out), cap, C.byref(n)))
            same(snapshot(L, ctx, out[: n.value], False), want, "host FRAMES_F32 | %d" % refine)
    finally:
        ctx.device_free(d8)
        ctx.device_free(dp)


# ---- 4 / 5: batches ----------------------------------------------------------------------------------

def _batch_frames(n, w, h, seed, colour):
    base = [make_frame(w, h, seed + i, colour) for i in range(4)]
    return np.ascontiguousarray(np.stack([np.roll(base[i % 4], 37 * (i // 4), axis=1) for i in range(n)]))


def _batch_result(res, order=None):
    out, n, tf = res
    idx = range(len(n)) if order is None else order
    return [(int(n[i]), out[i][: n[i]].tobytes(), bytes(tf[i])) for i in idx]


def _same_batch(got, want, what):
    assert len(got) == len(want)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g[0] == w_[0], "[%s] frame %d: n_lines %d, the fp32 path's %d" % (what, i, g[0], w_[0])
        assert g[1] == w_[1], "[%s] frame %d: records differ from the fp32 path's" % (what, i)
        assert g[2] == w_[2], "[%s] frame %d: transform differs from the fp32 path's" % (what, i)


def _batches(L, ctx, B, w, h, seed, colour):
    frames = _batch_frames(B, w, h, seed, colour)
    tail = frames.shape[3:]
    bpp = 3 if colour else 1
    fmt = L.PIX_U8X3 if colour else L.PIX_U8
    what = "%d x %s %dx%d" % (B, "u8x3" if colour else "u8", w, h)
    ml = max(w, h) / 100.0
    cfg = L.RectificationConfig(hmin=2.0)
    p = np.ascontiguousarray(np.stack([unit(f) for f in frames]))
    want = _batch_result(ctx.find_line_segment_groups_batch_host(p, ml, num_threads=8, cfg=cfg))
    assert sum(x[0] for x in want) > 0
    dp = ctx.device_upload(p)
    try:
        _same_batch(_batch_result(ctx.find_line_segment_groups_batch_device(dp, w * h, B, w, h, ml, cfg=cfg)), want, what + " fp32 resident")
    finally:
        ctx.device_free(dp)
    del p

    # resident frames
    d = ctx.device_upload(frames)
    try:
        got = ctx.find_line_segment_groups_batch_device(d, w * h, B, w, h, ml, cfg=cfg, fmt=fmt)
        _same_batch(_batch_result(got), want, what + " _batch_device")
    finally:
        ctx.device_free(d)

    # one array whose frames are an odd number of bytes apart (_batch_host), pageable: registered where they lie
    gap = h * w * bpp + 3 * 4099
    flat = np.full(B * gap, 5, np.uint8)
    padded = np.lib.stride_tricks.as_strided(flat, (B, h, w) + tail, (gap, w * bpp, bpp) + ((1,) if colour else ()))
    padded[...] = frames
    _same_batch(_batch_result(ctx.find_line_segment_groups_batch_host(padded, ml, num_threads=8, cfg=cfg)), want, what + " _batch_host, padded frame stride")
    assert np.array_equal(padded, frames)

    # a list, one frame listed twice (_batch_host_ptrs)
    order = list(range(B)) + [2]
    listed = [np.array(frames[i]) for i in range(B)]
    got = ctx.find_line_segment_groups_batch_host([listed[i] for i in order], ml, num_threads=8, cfg=cfg)
    _same_batch(_batch_result(got), [want[i] for i in order], what + " _batch_host_ptrs, a frame listed twice")

    # two lane sets on one device (_batch_host_multi)
    got = ctx.find_line_segment_groups_batch_host(frames, ml, num_threads=8, cfg=cfg, devices=[0, 0])
    _same_batch(_batch_result(got), want, what + " _batch_host_multi")
    got = ctx.find_line_segment_groups_batch_host([listed[i] for i in order], ml, num_threads=8, cfg=cfg, devices=[0, 0])
    _same_batch(_batch_result(got), [want[i] for i in order], what + " _batch_host_multi, a frame in both blocks")

    # page-locked
    pinned = ctx.host_alloc(frames.shape, np.uint8)
    try:
        pinned[...] = frames
        _same_batch(_batch_result(ctx.find_line_segment_groups_batch_host(pinned, ml, num_threads=8, cfg=cfg)), want, what + " page-locked")
    finally:
        ctx.host_free(pinned)

    # One contiguous, unpadded array from pageable memory: neighbouring frames share the page at each end.  Twice: the
    # first call's release must leave the memory as it found it.
    before = frames.copy()
    for call in (1, 2):
        got = ctx.find_line_segment_groups_batch_host(frames, ml, num_threads=8, cfg=cfg)
        _same_batch(_batch_result(got), want, what + " contiguous pageable array, call %d" % call)
        assert np.array_equal(frames, before)
    frames[0, 0, 0] ^= 1  # (and it is ordinary writable memory still)
    # overlapping windows over one array (fp32 too: the same weakness): every window is its own frame
    rows = np.ascontiguousarray(np.concatenate([frames[0], frames[1]], axis=0))
    windows = [rows[k * 8:k * 8 + h] for k in range(4)]
    want_w = _batch_result(ctx.find_line_segment_groups_batch_host([np.ascontiguousarray(unit(x)) for x in windows], ml, cfg=cfg))
    _same_batch(_batch_result(ctx.find_line_segment_groups_batch_host(windows, ml, num_threads=8, cfg=cfg)), want_w, what + " overlapping windows")


def test_batches_u8(L, ctx):
    _batches(L, ctx, 16, 1920, 1080, 1100, False)


def test_batches_u8x3(L, ctx):
    _batches(L, ctx, 8, 1920, 1080, 1200, True)


# ---- 6: full sizes ---------------------------------------------------------------------------------

def test_bench_frame_quantised(L, ctx):
    from librectify_amd import synth

    w, h = 3840, 2160
    frame = quantise(synth.frame(w, h, 1))
    p = unit(frame)
    ml = max(w, h) / 100.0
    want = snapshot(L, ctx, ctx.find_line_segment_groups(p, ml, num_threads=8))
    assert want["n"] > 100
    same(snapshot(L, ctx, ctx.find_line_segment_groups(frame, ml, num_threads=8)), want, "u8 4K from the host")
    d = ctx.device_upload(frame)
    try:
        same(snapshot(L, ctx, ctx.find_line_segment_groups_device(d, w, h, ml, fmt=L.PIX_U8).copy()), want, "u8 4K resident")
    finally:
        ctx.device_free(d)
    rgb = np.ascontiguousarray(np.stack([frame] * 3, axis=2))  # (equal channels: the luma is the channel)
    same(snapshot(L, ctx, ctx.find_line_segment_groups(rgb, ml, num_threads=8)), want, "u8x3 4K from the host")


@pytest.mark.parametrize("scale", [1, 2])
def test_doc_image(L, ctx, scale):
    import scipy.ndimage as ndi

    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    assert gray.dtype == np.uint8
    if scale != 1:
        gray = quantise(ndi.zoom(gray.astype(np.float64) / 256.0, scale, order=3))
    h, w = gray.shape
    p = unit(gray)
    ml = max(w, h) / 100.0
    want = snapshot(L, ctx, ctx.find_line_segment_groups(p, ml))
    ref, _ = O.find_line_segment_groups(p, ml, seed=0)
    assert want["lines"] == np.ascontiguousarray(ref).tobytes() and len(ref) > 50, "the fp32 path differs from the oracle"
    got = ctx.find_line_segment_groups(gray, ml)
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(ref).tobytes(), "u8 doc image x%d differs from the oracle on p" % scale
    same(snapshot(L, ctx, got), want, "u8 doc image x%d" % scale)
    rgb = np.ascontiguousarray(np.stack([gray, np.roll(gray, 1, axis=1), np.roll(gray, 1, axis=0)], axis=2))
    pc = unit(rgb)
    refc, _ = O.find_line_segment_groups(pc, ml, seed=0)
    gotc = ctx.find_line_segment_groups(rgb, ml)
    assert np.ascontiguousarray(gotc).tobytes() == np.ascontiguousarray(refc).tobytes(), "u8x3 doc image x%d differs from the oracle on p" % scale
    snap = snapshot(L, ctx, gotc)
    same(snap, snapshot(L, ctx, ctx.find_line_segment_groups(pc, ml)), "u8x3 doc image x%d" % scale)


def test_frame_of_8192_squared(L, ctx):
    small = gray_frame(2048, 2048, 1300)
    frame = np.ascontiguousarray(np.tile(small, (4, 4)))
    assert frame.shape == (8192, 8192)
    ml = 81.92
    c2 = L.Context(0)  # (9 GB of workspace: given back with the context)
    try:
        c2.set_seed(0)
        p = unit(frame)
        want = snapshot(L, c2, c2.find_line_segment_groups(p, ml, num_threads=8, capacity=1 << 20), planes=False)
        del p
        assert want["n"] > 100
        same(snapshot(L, c2, c2.find_line_segment_groups(frame, ml, num_threads=8, capacity=1 << 20), planes=False), want, "u8 8192x8192")
    finally:
        c2.close()


# ---- 7: rows that span more than 4 GiB ----------------------------------------------------------

def test_device_u8_frame_whose_rows_span_more_than_4_gib(L, ctx):
    """A 256 x 1100 crop of a device mosaic 2^22 bytes wide: 4.6 GB from the first byte to the last, more than the filter
    kernel's 32-bit byte offsets reach -- the frame is packed first, as bytes.  (At the fp32 test's stride of 2^20 pixels a
    u8 frame spans 1.15 GB and is read where it lies: that is the second case.)"""
    from librectify_amd import _check, _ptr

    w, h = 256, 1100
    frame = gray_frame(w, h, 4242)
    ml = 5.0
    want = fp32_device(L, ctx, unit(frame), ml)
    lib = L.lib()
    for stride in (1 << 22, 1 << 20):
        nbytes = (h - 1) * stride + w
        assert (nbytes > (1 << 32)) == (stride == 1 << 22)
        p = C.c_void_p()
        _check(lib.lr_device_malloc(ctx._h, nbytes, C.byref(p)))
        try:
            for y in range(h):
                _check(lib.lr_memcpy_h2d(ctx._h, C.c_void_p(p.value + y * stride), _ptr(frame[y]), w))
            got = ctx.find_line_segment_groups_device(p.value, w, h, ml, stride=stride, fmt=L.PIX_U8).copy()
            same(snapshot(L, ctx, got), want, "u8 256x1100 stride %d" % stride)
            res = ctx.find_line_segment_groups_batch_device(p.value, nbytes, 1, w, h, ml, capacity=4096, fmt=L.PIX_U8, stride=stride)
            assert res[0][0][: res[1][0]].tobytes() == want["lines"], "_batch_device, stride %d" % stride
        finally:
            _check(lib.lr_device_free(ctx._h, p))


# ---- 8: one context, every format ------------------------------------------------------------------

def test_one_context_alternates_formats_and_sizes(L, ctx):
    sizes = ((320, 240), (641, 479), (1000, 563))
    items = []
    ref_ctx = L.Context(0)
    try:
        ref_ctx.set_seed(0)
        for k, ((w, h), kind) in enumerate(itertools.product(sizes, ("f32", "u8", "u8x3"))):
            frame = make_frame(w, h, 1400 + k, kind == "u8x3")
            p = unit(frame)
            ml = min_len(w, h)
            want = snapshot(L, ref_ctx, ref_ctx.find_line_segment_groups(p, ml))
            items.append((kind, p if kind == "f32" else frame, ml, want))
    finally:
        ref_ctx.close()
    order = [4, 0, 8, 2, 6, 1, 5, 7, 3, 3, 8, 0, 4]  # fixed, shuffled
    c = L.Context(0)
    try:
        c.set_seed(0)
        for lap in (1, 2):
            for i in order:
                kind, src, ml, want = items[i]
                same(snapshot(L, c, c.find_line_segment_groups(src, ml, num_threads=8)), want, "lap %d, item %d (%s), host" % (lap, i, kind))
                h, w = src.shape[:2]
                d = c.device_upload(src)
                try:
                    fmt = {"f32": L.PIX_F32, "u8": L.PIX_U8, "u8x3": L.PIX_U8X3}[kind]
                    got = c.find_line_segment_groups_device(d, w, h, ml, fmt=fmt).copy()
                    same(snapshot(L, c, got), want, "lap %d, item %d (%s), resident" % (lap, i, kind))
                finally:
                    c.device_free(d)
            c.trim()
    finally:
        c.close()


# ---- 9: clean failures --------------------------------------------------------------------------------

def test_clean_failures_with_an_8_bit_word(L, ctx):
    from librectify_amd import _check, _ptr

    w, h = 64, 48
    frame = gray_frame(w, h, 1500)
    rgb = colour_frame(w, h, 1501)
    lib = L.lib()
    out = np.zeros(64, L.LINE_DTYPE)
    n = C.c_int(-5)
    d = ctx.device_upload(frame)
    try:
        for word, src in ((L.FRAMES_U8, frame), (L.FRAMES_U8X3, rgb), (L.FRAMES_U8 | 1, frame)):
            # |stride| < width
            for stride in (w - 1, -(w - 1), 0):
                assert lib.lr_find_line_segment_groups_host(ctx._h, _ptr(src), w, h, stride, 2.0, word, 8, _ptr(out), 64, C.byref(n)) != 0
                assert lib.lr_last_error()
            assert lib.lr_find_line_segment_groups_device(ctx._h, C.c_void_p(d), w, h, w - 1, 2.0, word, -1, _ptr(out), 64, C.byref(n)) != 0
            assert lib.lr_last_error()
            # no frame
            assert lib.lr_find_line_segment_groups_host(ctx._h, None, w, h, w, 2.0, word, 8, _ptr(out), 64, C.byref(n)) != 0
            assert lib.lr_find_line_segment_groups_device(ctx._h, None, w, h, w, 2.0, word, -1, _ptr(out), 64, C.byref(n)) != 0
            ptrs = (C.c_void_p * 2)(src.ctypes.data, None)
            cfg = L.RectificationConfig()
            assert lib.lr_find_line_segment_groups_batch_host_ptrs(ctx._h, ptrs, 2, w, h, w, 2.0, word, 8, None, 0, None, C.byref(cfg), None) != 0
            # smaller than the filter: no lines, silently
            for (sw, sh) in ((4, 48), (64, 4), (1, 1)):
                n.value = -5
                _check(lib.lr_find_line_segment_groups_host(ctx._h, _ptr(src), sw, sh, sw, 2.0, word, 8, _ptr(out), 64, C.byref(n)))
                assert n.value == 0
                n.value = -5
                _check(lib.lr_find_line_segment_groups_device(ctx._h, C.c_void_p(d), sw, sh, sw, 2.0, word, -1, _ptr(out), 64, C.byref(n)))
                assert n.value == 0
        # the context is as good as before
        want = fp32_device(L, ctx, unit(frame), 2.0)
        same(snapshot(L, ctx, ctx.find_line_segment_groups_device(d, w, h, 2.0, fmt=L.PIX_U8).copy()), want, "after the failures")
    finally:
        ctx.device_free(d)


# ---- 10: rectify ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [False, True])
def test_rectify_without_a_prescale_equals_the_pipeline_from_its_parts(L, ctx, colour):
    """host luma -> fp32 detect -> transform -> homography -> warp_perspective, against rectify(img, max_size=None), which
    uploads the 8-bit frame once and detects on it in place"""
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    img = np.ascontiguousarray(np.stack([gray, np.roll(gray, 1, axis=1), np.roll(gray, 2, axis=0)], axis=2)) if colour else gray
    assert L.frames_word(fmt_of(L, img)) in (L.FRAMES_U8, L.FRAMES_U8X3)
    h, w = img.shape[:2]
    ml = max(w, h) / 100.0
    cfg = L.RectificationConfig(hmin=2.0)
    lines = ctx.find_line_segment_groups(unit(img), ml)
    t = L.compute_rectification_transform(lines, w, h, cfg)
    _, M, size = L.rectification_homography(t, 3.0)
    warped = ctx.warp_perspective(img, M, size)
    got_lines, got_t, got_warped = ctx.rectify(img, max_size=None)
    assert np.ascontiguousarray(got_lines).tobytes() == np.ascontiguousarray(lines).tobytes() and len(lines) > 50
    assert bytes(got_t) == bytes(t)
    assert got_warped.shape == warped.shape and got_warped.dtype == np.uint8 and np.array_equal(got_warped, warped)
