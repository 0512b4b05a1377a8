"""The detector kernels (filter, bins and dilated mask, seeds, flood, fit) against the float64 second source
tests/numpy_detector_ref.py, stage by stage: each stage is checked on the device's own fp32 output of the stage
before, with the three-valued rules of numpy_detector_ref (sure / ambiguous within EPS = 2^-20 / sure not).  Where
the kernels go wrong: ragged tiles (kLaneCols = 56 columns, 4-px halos) and bands (kBandRows = 30 rows), one-tile
frames, caller strides (one frame whose rows span more than 4 GiB), the size classes of the component fit, content
with exact ties.  test_gpu_parity.py holds the same kernels bit-exact against the oracle; this file does not use the
oracle at all."""
import ctypes as C

import numpy as np
import pytest

import numpy_detector_ref as N

pytestmark = pytest.mark.gpu

LANE_COLS, BAND_ROWS = 56, 30


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L

    L.lib()
    assert L.device_count() > 0, "GPU tests need a GPU"
    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def device_stages(L, ctx, img=None, dptr=None, shape=None, stride=None, mode=1):
    """the stage products of one frame (host array, or device pointer + shape + stride), dmask taken before the flood"""
    ctx.set_flood_mode(mode)
    try:
        if dptr is None:
            ctx.stage_filter_host(np.ascontiguousarray(img, np.float32))
        else:
            h, w = shape
            ctx.stage_filter_device(dptr, w, h, stride)
        st = dict(dx=ctx.download(L.BUF_DX), dy=ctx.download(L.BUF_DY), dmask=ctx.download(L.BUF_DMASK))
        ctx.stage_seeds()
        st.update(maxmag=ctx.download(L.BUF_MAXMAG)[0], seed_idx=ctx.download(L.BUF_SEED_IDX),
                  seed_bin=ctx.download(L.BUF_SEED_BIN), seed_thr=ctx.download(L.BUF_SEED_THR))
        ctx.stage_flood()
        st["label"] = ctx.download(L.BUF_LABEL)
        st["lines"] = ctx.stage_fit()
    finally:
        ctx.set_flood_mode(1)
    return st


def _same_bits(a, b, frame):
    for k in ("dx", "dy", "dmask", "seed_idx", "seed_bin", "seed_thr", "label"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "[%s] %s differs from the contiguous frame's" % (frame, k)
    assert np.float32(a["maxmag"]).tobytes() == np.float32(b["maxmag"]).tobytes(), "[%s] maxmag" % frame
    assert a["lines"].tobytes() == b["lines"].tobytes(), "[%s] segment records differ from the contiguous frame's" % frame


def _noisy_ok(frame, counts):
    """a noisy synthetic frame leaves no decision to the device"""
    assert counts["seeds_taken_from_device"] == 0 and counts["flood_px_taken_from_device"] == 0, (frame, counts)


# (w, h): n_tiles == 1, one column of tiles, one band, and every side of the 56-column tile and the 30-row band
SHAPES = [(5, 5), (55, 29), (56, 30), (6, 30), (5, 29),
          (5, 61), (6, 94), (55, 59), (56, 94),
          (57, 5), (112, 5), (116, 29), (171, 30),
          (57, 31), (60, 34), (111, 59), (112, 60), (113, 61), (116, 94), (171, 94),
          (55, 31), (56, 60), (57, 60), (60, 29), (111, 30), (113, 34), (116, 61), (171, 31), (171, 59), (112, 94)]


def _synth(w, h, seed, edge=False):
    from librectify_amd import synth

    img = synth.frame(w, h, seed, bars=max(2, (w * h) // 1500)).astype(np.float64)
    if edge:
        # the strongest edge of the frame in its last (ragged) band and column tile, where the filter's per-tile maximum
        # and the seed threshold it sets would miss it if a reduction skipped that tile
        r0 = min(max(BAND_ROWS * ((h - 1) // BAND_ROWS) + 1, 2), h - 3)
        c0 = min(max(LANE_COLS * ((w - 1) // LANE_COLS) + 1, 2), w - 3)
        img[r0:, c0:] += 3.0
    return img.astype(np.float32)


def test_shapes_at_the_tile_and_band_edges(L, ctx):
    assert len(SHAPES) == 30
    for k, (w, h) in enumerate(SHAPES):
        for edge in (False, True):
            img = _synth(w, h, 700 + k, edge)
            frame = "%dx%d%s" % (w, h, " +edge" if edge else "")
            st = device_stages(L, ctx, img)
            counts = N.check_stages(frame, img, st)
            _noisy_ok(frame, counts)


def _upload_strided(L, ctx, img, stride, pad_value=7.0):
    h, w = img.shape
    buf = np.full((h, stride), pad_value, np.float32)
    buf[:, :w] = img
    return ctx.device_upload(buf)


@pytest.mark.parametrize("shape", [(57, 31), (113, 61), (171, 94), (256, 120)])
def test_device_strides(L, ctx, shape):
    """stride = w + 1, w + 13, 2 w (the padding holds 7.0): bit-identical to the contiguous frame, and within the
    second source's bounds; lr_find_line_segment_groups_device too"""
    w, h = shape
    img = _synth(w, h, 31 + w)
    base = device_stages(L, ctx, img)
    ml = max(w, h) / 50.0
    ctx.set_seed(0)
    full = ctx.find_line_segment_groups(img, ml)
    for stride in (w + 1, w + 13, 2 * w):
        frame = "%dx%d stride %d" % (w, h, stride)
        d = _upload_strided(L, ctx, img, stride)
        try:
            st = device_stages(L, ctx, dptr=d, shape=(h, w), stride=stride)
            _same_bits(st, base, frame)
            _noisy_ok(frame, N.check_stages(frame, img, st))
            ctx.set_seed(0)
            got = ctx.find_line_segment_groups_device(d, w, h, ml, stride=stride).copy()
            assert got.tobytes() == full.tobytes(), "[%s] full path differs from the contiguous frame's" % frame
        finally:
            ctx.device_free(d)


def test_device_frame_whose_rows_span_more_than_4_gib(L, ctx):
    """A 256 x 1100 crop of a device mosaic 2^20 floats wide: its rows span 4.6 GB, more than the filter kernel's
    32-bit byte offsets reach.  Stage products, the single-frame and the batch device call must equal the contiguous
    frame's (once they came back wrong, without an error)."""
    from librectify_amd import _check, _ptr

    w, h, stride = 256, 1100, 1 << 20
    img = _synth(w, h, 4242)
    frame = "256x1100 stride 2^20"
    base = device_stages(L, ctx, img)
    ml = 5.0
    ctx.set_seed(0)
    full = ctx.find_line_segment_groups(img, ml)
    nbytes = ((h - 1) * stride + w) * 4
    assert nbytes > (1 << 32)
    lib = L.lib()
    p = C.c_void_p()
    _check(lib.lr_device_malloc(ctx._h, nbytes, C.byref(p)))
    try:
        rows = np.ascontiguousarray(img)
        for y in range(h):
            _check(lib.lr_memcpy_h2d(ctx._h, C.c_void_p(p.value + y * stride * 4), _ptr(rows[y]), w * 4))
        st = device_stages(L, ctx, dptr=p.value, shape=(h, w), stride=stride)
        _same_bits(st, base, frame)
        _noisy_ok(frame, N.check_stages(frame, img, st))
        ctx.set_seed(0)
        got = ctx.find_line_segment_groups_device(p.value, w, h, ml, stride=stride).copy()
        assert got.tobytes() == full.tobytes(), "[%s] lr_find_line_segment_groups_device differs" % frame
        cap = 4096
        out = np.zeros((1, cap), L.LINE_DTYPE)
        n = np.zeros(1, np.int32)
        tf = (L.ImageTransform * 1)()
        cfg = L.RectificationConfig()
        ctx.set_seed(0)
        _check(lib.lr_find_line_segment_groups_batch_device(ctx._h, p, (h - 1) * stride + w, 1, w, h, stride, ml, 0, -1,
                                                             _ptr(out), cap, _ptr(n), C.byref(cfg), C.byref(tf)))
        assert out[0][: n[0]].tobytes() == full.tobytes(), "[%s] lr_find_line_segment_groups_batch_device differs" % frame
    finally:
        _check(lib.lr_device_free(ctx._h, p))


def _bars(lengths, sigma, W, gap=30, seed=5):
    """soft horizontal bars of the given lengths, one above the other: each gives two floods of about
    (2 sigma + 0.5) * 2 * length pixels"""
    from librectify_amd import synth

    H = gap * (len(lengths) + 1)
    img = np.full((H, W), 0.3)
    for k, ln in enumerate(lengths):
        y = gap * (k + 1) - 5
        img[y: y + 10, 20: 20 + ln] += 0.4
    return (synth._gauss_blur(img, sigma) + np.random.RandomState(seed).normal(0, 0.002, img.shape)).astype(np.float32)


@pytest.mark.parametrize("mode", [0, 1])
def test_fit_size_classes_at_their_edges(L, ctx, mode):
    """Components on both sides of 64, 1024, 4096 and 16384 px (the fit's size classes: a wavefront, LDS, LDS, the
    huge-component path; flood mode 1 books the largest flood to decide whether the huge path runs).  The test asserts
    its own coverage: for each edge a component within 5 % below it and one within 5 % above it."""
    frames = {64: _bars(list(range(31, 38)), 1.0, 100), 1024: _bars(list(range(250, 271, 3)), 2.0, 300),
              4096: _bars(list(range(1000, 1061, 10)), 2.0, 1100), 16384: _bars(list(range(4000, 4201, 33)), 2.0, 4250)}
    for edge, img in frames.items():
        frame = "bars around %d px, mode %d" % (edge, mode)
        st = device_stages(L, ctx, img, mode=mode)
        N.check_stages(frame, img, st)  # (flat flanks with little noise: near-ties are allowed here)
        sizes = np.bincount(st["label"][st["label"] >= 0])
        assert ((sizes <= edge) & (sizes >= 0.95 * edge)).any(), (frame, "nothing just below")
        assert ((sizes > edge) & (sizes <= 1.05 * edge)).any(), (frame, "nothing just above")


def test_doc_image_at_1x_and_2x(L, ctx):
    import os

    import scipy.ndimage as ndi

    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "doc_image_gray.npy")
    img = np.load(g).astype(np.float32) / np.float32(256.0)
    for scale, im in ((1, img), (2, ndi.zoom(img.astype(np.float64), 2, order=3).astype(np.float32))):
        frame = "doc image %dx (%dx%d)" % (scale, im.shape[1], im.shape[0])
        counts = N.check_stages(frame, im, device_stages(L, ctx, im))
        print(frame, counts)


def test_unusual_content(L, ctx):
    """the 13 kinds of test_gpu_parity at 416 x 304; the noiseless ones have exact ties (seeds of one magnitude along
    a flank, responses equal in two bins), so they exercise the tie and ambiguity rules"""
    from test_gpu_parity import _unusual_frames

    for name, img in _unusual_frames(416, 304).items():
        img = np.ascontiguousarray(img)
        counts = N.check_stages(name, img, device_stages(L, ctx, img))
        print(name, counts)
