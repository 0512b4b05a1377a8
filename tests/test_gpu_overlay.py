"""The lines picture on the GPU: lr_draw_lines_device (kernels_overlay.hip) against tests/numpy_overlay_ref.py, byte for
byte: partial tiles, chunk boundaries of the walk, an LDS list that fills many times, the early stop, tiny frames, u8x3 and
in place, a batch with padded rows and gaps, H, far endpoints, the pipeline end to end, and the clean failures (each refused
on the host before anything is launched: the tests provoke nothing on the device)."""
import ctypes as C
import os

import numpy as np
import pytest

import numpy_overlay_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SENTINEL = 0xAB
PREFIX = "lr_draw_lines_device: "
LIST_CAPACITY = 256  # kernels_overlay.hip: kList, the records the LDS list holds (one chunk of the walk)


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


def make_lines(L, rows):
    out = np.zeros(len(rows), L.LINE_DTYPE)
    for i, r in enumerate(rows):
        out[i] = (r[0], r[1], r[2], r[3], 1.0, 0.0, r[4])
    return out


def gray(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def short_segments(L, n, seed, x_range, y_range, reach=9):
    """n seeded segments with both ends inside x_range x y_range, at most `reach` long per axis, groups -1 .. 13"""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(x_range[0], x_range[1], n)
    y1 = rng.uniform(y_range[0], y_range[1], n)
    x2 = np.clip(x1 + rng.uniform(-reach, reach, n), *x_range)
    y2 = np.clip(y1 + rng.uniform(-reach, reach, n), *y_range)
    return make_lines(L, list(zip(x1, y1, x2, y2, rng.integers(-1, 14, n))))


def forty_segments(L):
    """on a 130 x 37 frame: groups -1 .. 13, ends off the frame on every side, segments wholly outside, a zero-length one,
    two identical ones with different groups, the frame's diagonal"""
    rng = np.random.default_rng(40)
    rows = [(rng.uniform(-30, 160), rng.uniform(-20, 57), rng.uniform(-30, 160), rng.uniform(-20, 57), g)
            for g in list(range(-1, 14)) + [0, 1, 2, 3, 5, 8, 11, 12]]
    rows += [(-40.5, 10.2, 20.7, 30.1, 4), (100.0, 18.0, 190.0, 5.0, 6), (64.0, -30.0, 60.0, 12.0, 7), (10.0, 30.0, 14.0, 80.0, 9),  # off each side
             (-50.0, -50.0, -20.0, -9.0, 1), (140.0, 45.0, 170.0, 60.0, 2), (200.0, 5.0, 300.0, 9.0, 3), (20.0, 60.0, 90.0, 44.0, 10),  # wholly outside
             (77.3, 21.8, 77.3, 21.8, 5),  # zero length
             (30.0, 5.0, 95.0, 33.0, 2), (30.0, 5.0, 95.0, 33.0, 9),  # identical, different groups
             (0.0, 0.0, 129.0, 36.0, -1),  # the diagonal
             (63.9, 15.9, 64.0, 16.0, 13), (128.0, 0.0, 129.9, 36.9, 12), (0.0, 36.0, 64.0, 36.0, 11),
             (5.0, 5.0, 6.0, 5.0, 0), (60.0, 10.0, 70.0, 20.0, 3)]
    assert len(rows) == 40
    return make_lines(L, rows)


def check(ctx, img, lines, H=None):
    got = ctx.draw_lines(img, lines, H)
    want = R.draw(img, lines, H)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, "%d pixels differ, the first at (y, x) = %s: got %s, want %s" % (
        len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    return want


def test_partial_tiles_with_forty_segments(L, ctx):
    img = gray(130, 37, 1)
    lines = forty_segments(L)
    want, owner = R.draw(img, lines, with_owner=True)
    assert len(np.unique(owner)) > 25 and (owner == 33).any() and (owner[owner >= 0] != 32).all()  # of the identical pair the later one
    check(ctx, img, lines)


def test_more_than_one_chunk_of_the_walk(L, ctx):
    img = gray(130, 37, 2)
    lines = short_segments(L, 700, 7, (-8, 108), (-8, 45))
    lines[0] = (124.0, 30.0, 124.0, 30.0, 1.0, 0.0, 8)  # alone in its corner: found in the third chunk of the walk
    _, owner = R.draw(img, lines, with_owner=True)
    assert 700 > 2 * LIST_CAPACITY and (owner < 0).any() and (owner == 0).sum() == 81
    check(ctx, img, lines)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_segment_counts_around_a_wavefront_and_a_chunk(L, ctx, n):
    """all in the second tile of the first tile row (x 64 .. 127, y 0 .. 15); the first segment owns a pixel of its own"""
    img = gray(130, 37, 3)
    lines = short_segments(L, n, 100 + n, (70, 110), (6, 10), reach=4)
    lines[0] = (122.0, 9.0, 122.0, 9.0, 1.0, 0.0, 4)
    _, owner = R.draw(img, lines, with_owner=True)
    assert (owner == 0).any() and (owner == n - 1).any()
    check(ctx, img, lines)


@pytest.mark.parametrize("order", ["ascending", "reversed"])
def test_the_list_in_lds_fills_many_times(L, ctx, order):
    """5 000 segments through the one tile of a 64 x 16 frame: some twenty times the list's capacity (LIST_CAPACITY
    records, one chunk), so the list is filled, tested and emptied about twenty times.  The segments leave the right
    columns free, so the tile is never complete and every chunk is walked; the first segment alone owns pixels there."""
    n = 5000
    assert n > 19 * LIST_CAPACITY
    img = gray(64, 16, 4)
    lines = short_segments(L, n, 5, (0, 44), (0, 15), reach=6)
    lines[0] = (58.0, 8.0, 58.0, 8.0, 1.0, 0.0, 6)
    if order == "reversed":
        lines = lines[::-1].copy()
    want, owner = R.draw(img, lines, with_owner=True)
    assert (owner < 0).any() and (owner == (0 if order == "ascending" else n - 1)).sum() == 81
    assert len(np.unique(owner)) > 30
    check(ctx, img, lines)


def test_early_stop_on_a_tile_the_last_segments_cover(L, ctx):
    img = gray(130, 37, 5)
    beneath = short_segments(L, 300, 6, (0, 63), (0, 15))
    cover = make_lines(L, [(-10.0, float(y), 80.0, float(y), g) for g, y in enumerate(range(1, 17, 3))])
    lines = np.concatenate([beneath, cover])
    _, owner = R.draw(img, lines, with_owner=True)
    assert (owner[:16, :64] >= 300).all() and (owner[:, 100:] < 0).all()
    check(ctx, img, lines)


BIN = 256  # kernels_overlay.hip: kBin, the side of the host's bins


def bin_entries(lines, w, h):
    """(entries, bins touched): the (segment, bin) pairs the host's binning makes for a frame -- boxes grown by the disc's
    radius and cut to the frame -- restated here so that a test can say which of the two paths its frame takes: bins
    while entries <= 8 n, one list of all beyond that"""
    entries, touched = 0, set()
    for line in lines:
        seg = R.endpoints(line)
        if seg is None:
            continue
        x_lo, x_hi = max(min(seg[0], seg[2]) - R.REACH, 0), min(max(seg[0], seg[2]) + R.REACH, w - 1)
        y_lo, y_hi = max(min(seg[1], seg[3]) - R.REACH, 0), min(max(seg[1], seg[3]) + R.REACH, h - 1)
        if x_lo > x_hi or y_lo > y_hi:
            continue
        for by in range(y_lo // BIN, y_hi // BIN + 1):
            for bx in range(x_lo // BIN, x_hi // BIN + 1):
                entries += 1
                touched.add((bx, by))
    return entries, touched


def on_bin_borders(L):
    """dots and short strokes whose grown boxes straddle bin borders of an 1100 x 800 frame, in x, in y and at corners"""
    rows = []
    for k, v in enumerate((255, 256, 261, 250, 511, 512, 517, 767, 768, 773)):
        rows += [(float(v), 100.0 + 37 * k, float(v), 100.0 + 37 * k, k), (60.0 + 97 * k, float(v), 60.0 + 97 * k, float(v), k + 3)]
    rows += [(255.0, 255.0, 256.0, 256.0, 1), (261.0, 261.0, 261.0, 261.0, 2), (250.0, 511.0, 262.0, 513.0, 4), (512.0, 256.0, 512.0, 256.0, 5),
             (767.0, 511.0, 769.0, 512.0, 6), (1023.0, 767.0, 1025.0, 769.0, 7), (1029.0, 773.0, 1029.0, 773.0, 8),
             (240.0, 300.0, 530.0, 300.0, 9), (700.0, 240.0, 700.0, 530.0, 10)]
    return make_lines(L, rows)


def test_many_bins_in_rows_and_columns(L, ctx):
    """1100 x 800: 5 x 4 bins, 18 x 50 tiles.  A few hundred short segments all over the frame and the border set: the
    binned path, with every bin in use and segments that belong to two and to four bins."""
    w, h = 1100, 800
    lines = np.concatenate([short_segments(L, 200, 31, (-8, w + 8), (-8, h + 8), reach=30), on_bin_borders(L),
                            short_segments(L, 200, 32, (-8, w + 8), (-8, h + 8), reach=30)])
    entries, touched = bin_entries(lines, w, h)
    assert len(lines) < entries <= 8 * len(lines) and len(touched) == 20
    img = gray(w, h, 31)
    _, owner = R.draw(img, lines, with_owner=True)
    assert (owner < 0).any() and len(np.unique(owner)) > 350
    check(ctx, img, lines)


def test_one_list_of_all_when_long_segments_cross_the_bins(L, ctx):
    """The same frame with forty segments that cross it, beneath, between and above a few short ones and the border set:
    more than 8 entries a segment, so the frame keeps one list of all its records and every tile walks it."""
    w, h = 1100, 800
    rng = np.random.default_rng(33)
    long_rows = [(0.0, 0.0, w - 1.0, h - 1.0, 0), (0.0, h - 1.0, w - 1.0, 0.0, 1), (-40.0, 256.0, w + 40.0, 261.0, 2), (256.0, -40.0, 255.0, h + 40.0, 3)]
    for k in range(36):  # corner to corner, both ways: the grown box of each covers all twenty bins
        x1, y1, x2, y2 = rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(w - 50, w + 50), rng.uniform(h - 50, h + 50)
        long_rows.append((x1, y1, x2, y2, k % 15 - 1) if k % 2 else (x1, y2, x2, y1, k % 15 - 1))
    long_lines = make_lines(L, long_rows)
    lines = np.concatenate([long_lines[:14], short_segments(L, 12, 34, (0, w), (0, h), reach=30), long_lines[14:27], on_bin_borders(L),
                            long_lines[27:], short_segments(L, 8, 35, (0, w), (0, h), reach=30)])
    entries, touched = bin_entries(lines, w, h)
    assert entries > 8 * len(lines) and len(touched) == 20, (entries, len(lines))
    img = gray(w, h, 33)
    _, owner = R.draw(img, lines, with_owner=True)
    assert (owner < 0).any() and len(np.unique(owner)) > 60
    want = check(ctx, img, lines)
    # two frames in one call, the first on one list of all and the second binned: the second's records start behind the first's
    both = np.concatenate([lines, on_bin_borders(L)])
    table = L.draw_table([(w, h), (w, h)], [(0, w), (0, w)], [(0, w * 3), (w * h * 3, w * 3)], [(0, len(lines)), (len(lines), len(both) - len(lines))])
    d_src = ctx.device_upload(img)
    d_dst = ctx.device_upload(np.full(2 * w * h * 3, SENTINEL, np.uint8))
    try:
        ctx.draw_lines_device(d_src, img.size, L.PIX_U8, both, table, d_dst, 2 * w * h * 3)
        got = ctx.device_download(d_dst, (2, h, w, 3), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], R.draw(img, on_bin_borders(L)))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1)])
def test_tiny_frames(L, ctx, w, h):
    img = gray(w, h, 6)
    lines = make_lines(L, [(0.0, 0.0, 0.0, 0.0, 2), (-3.0, -3.0, float(w) + 2, float(h) + 2, 4), (0.0, float(h - 1), float(w - 1), 0.0, -1),
                           (float(w // 2), float(h // 2), float(w // 2), float(h // 2), 7)])
    check(ctx, img, lines[:1])
    check(ctx, img, lines)


def test_no_segments_gives_the_background(L, ctx):
    img = gray(130, 37, 7)
    got = ctx.draw_lines(img, np.zeros(0, L.LINE_DTYPE))
    np.testing.assert_array_equal(got, np.repeat(img[:, :, None], 3, axis=2))
    rgb = np.random.default_rng(8).integers(0, 256, (37, 130, 3), dtype=np.uint8)
    np.testing.assert_array_equal(ctx.draw_lines(rgb, np.zeros(0, L.LINE_DTYPE)), rgb)


def test_u8x3_source_and_in_place(L, ctx):
    rgb = np.random.default_rng(9).integers(0, 256, (37, 130, 3), dtype=np.uint8)
    lines = forty_segments(L)
    want = check(ctx, rgb, lines)
    # in place: the destination holds a seeded pattern with padded rows; only covered pixels change
    row = 130 * 3 + 7
    region = np.random.default_rng(10).integers(0, 256, 5 + 36 * row + 130 * 3 + 3, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(region[5:], (37, 130, 3), (row, 3, 1))
    before = region.copy()
    exp = R.draw(view.copy(), lines)
    d = ctx.device_upload(region)
    try:
        ctx.draw_lines_device(None, 0, L.PIX_U8X3, lines, L.draw_table([(130, 37)], None, [(5, row)], [(0, 40)]), d, len(region))
        got = ctx.device_download(d, (len(region),), np.uint8)
    finally:
        ctx.device_free(d)
    got_view = np.lib.stride_tricks.as_strided(got[5:], (37, 130, 3), (row, 3, 1))
    np.testing.assert_array_equal(got_view, exp)
    changed = got != before
    inside = np.zeros(len(region), bool)
    np.lib.stride_tricks.as_strided(inside[5:], (37, 130 * 3), (row, 1))[:] = True
    assert changed.any() and not (changed & ~inside).any()
    covered = (R.draw(np.zeros((37, 130), np.uint8), lines, with_owner=True)[1] >= 0)
    assert not (got_view != view)[~covered].any()
    assert want.shape == exp.shape


def batch_layout(L):
    """three frames with padded rows and gaps, outputs out of frame order, segments out of one array with unused rows between"""
    sizes = [(130, 37), (64, 16), (33, 200)]
    frames = [gray(w, h, 20 + k) for k, (w, h) in enumerate(sizes)]
    capacity = 64
    lines = np.zeros(3 * capacity, L.LINE_DTYPE)
    lines["x1"] = np.nan  # unused rows, as a detector's `capacity` leaves them (here poisoned: they must not be read as segments)
    counts = [40, 25, 33]
    per_frame = [forty_segments(L), short_segments(L, 25, 21, (-5, 70), (-5, 20)), short_segments(L, 33, 22, (-5, 40), (-5, 205), reach=30)]
    for b, ls in enumerate(per_frame):
        lines[b * capacity:b * capacity + counts[b]] = ls
    src_rows = [131, 64 + 5, 33 + 2]
    src_offs, cursor = [], 3
    for (w, h), row in zip(sizes, src_rows):
        src_offs.append(cursor)
        cursor += (h - 1) * row + w + 6
    src = np.full(cursor, 0x5A, np.uint8)
    for f, off, row, (w, h) in zip(frames, src_offs, src_rows, sizes):
        np.lib.stride_tricks.as_strided(src[off:], (h, w), (row, 1))[:] = f
    dst_rows = [130 * 3 + 5, 64 * 3, 33 * 3 + 1]
    spans = [(h - 1) * row + w * 3 for (w, h), row in zip(sizes, dst_rows)]
    dst_offs = [0, 0, 0]
    dst_offs[2] = 7
    dst_offs[0] = dst_offs[2] + spans[2] + 9
    dst_offs[1] = dst_offs[0] + spans[0] + 2
    dst_bytes = dst_offs[1] + spans[1] + 11
    assert dst_offs[0] > dst_offs[2] and any(o % 4 for o in dst_offs)
    table = L.draw_table(sizes, list(zip(src_offs, src_rows)), list(zip(dst_offs, dst_rows)), [(b * capacity, counts[b]) for b in range(3)])
    return sizes, frames, lines, per_frame, src, table, dst_bytes


def test_batch_is_exact_writes_nothing_else_and_equals_single_calls(L, ctx):
    sizes, frames, lines, per_frame, src, table, dst_bytes = batch_layout(L)
    d_src = ctx.device_upload(src)
    d_dst = ctx.device_upload(np.full(dst_bytes, SENTINEL, np.uint8))
    d_one = ctx.device_upload(np.full(dst_bytes, SENTINEL, np.uint8))
    try:
        ctx.draw_lines_device(d_src, len(src), L.PIX_U8, lines, table, d_dst, dst_bytes)
        got = ctx.device_download(d_dst, (dst_bytes,), np.uint8)
        for b in range(3):
            ctx.draw_lines_device(d_src, len(src), L.PIX_U8, lines, table[b:b + 1], d_one, dst_bytes)
        singles = ctx.device_download(d_one, (dst_bytes,), np.uint8)
    finally:
        for p in (d_src, d_dst, d_one):
            ctx.device_free(p)
    written = np.zeros(dst_bytes, bool)
    for b, (w, h) in enumerate(sizes):
        off, row = int(table[b, 4]), int(table[b, 5])
        view = np.lib.stride_tricks.as_strided(got[off:], (h, w, 3), (row, 3, 1))
        np.testing.assert_array_equal(view, R.draw(frames[b], per_frame[b]), err_msg="frame %d" % b)
        np.lib.stride_tricks.as_strided(written[off:], (h, w * 3), (row, 1))[:] = True
    assert (got[~written] == SENTINEL).all() and (~written).sum() > 200
    np.testing.assert_array_equal(got, singles)


def golden_h_at_an_eighth(L):
    rows = [[float(v) for v in line.split(",")] for line in open(os.path.join(G, "doc_warp_tform.csv"))]
    t = L.ImageTransform()
    t.width, t.height = 1000, 563
    t.top_left, t.top_right, t.bottom_left, t.bottom_right = [L.Point(r[0], r[1], 0.0) for r in rows[:4]]
    H, _, (w, h) = L.rectification_homography(t, 3.0)
    S = np.diag([0.125, 0.125, 1.0])
    lines = np.loadtxt(os.path.join(G, "doc_warp_lines.csv"), delimiter=",")
    lines[:, :4] *= 0.125
    return S @ H @ np.linalg.inv(S), (w + 7) // 8, (h + 7) // 8, make_lines(L, [tuple(r[:4]) + (int(r[6]),) for r in lines])


def test_lines_through_the_golden_homography(L, ctx):
    H, w, h, lines = golden_h_at_an_eighth(L)
    assert len(lines) == 848 and (w, h) == (142, 75)
    rgb = np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8)
    _, owner = R.draw(rgb, lines, H, with_owner=True)
    assert (owner >= 0).mean() > 0.3 and (owner < 0).any()
    check(ctx, rgb, lines, H)


def test_lines_through_a_homography_whose_horizon_crosses_the_frame(L, ctx):
    H = np.array([[1.1, 0.05, 3.0], [-0.04, 0.9, 2.0], [0.001, 0.02, -0.5]])  # the denominator changes sign near y = 24
    lines = short_segments(L, 200, 12, (0, 130), (0, 37), reach=25)
    drawn = [R.endpoints(l, H) is not None for l in lines]
    assert 20 < sum(drawn) < 180
    img = gray(130, 37, 12)
    Hs = -4.0 * np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1]])  # and a negative denominator throughout: drawn
    check(ctx, img, lines, H)
    np.testing.assert_array_equal(check(ctx, img, lines, Hs), R.draw(img, lines))


def test_far_endpoints_need_int64(L, ctx):
    img = gray(130, 37, 13)
    far = make_lines(L, [(-2.0 ** 24, -2.0 ** 24, 2.0 ** 24, 2.0 ** 24 - 7, 3), (2.0 ** 24, -2.0 ** 24, -2.0 ** 24, 2.0 ** 24, 5),
                         (-2.0 ** 24, 3.0, 2.0 ** 24, 30.0, 7), (2.0 ** 24 + 2, 3.0, 5.0, 5.0, 1), (np.nan, 3.0, 5.0, 5.0, 1),
                         (4.0, np.inf, 5.0, 5.0, 1)])
    _, owner = R.draw(img, far, with_owner=True)
    assert set(np.unique(owner)) == {-1, 0, 1, 2}
    check(ctx, img, far)


def test_end_to_end_with_rectify_and_the_batch_equals_the_loop(L, ctx):
    from librectify_amd import synth

    frames = [np.clip(synth.frame(w, h, 30 + k) * 255.0, 0, 255).astype(np.uint8) for k, (w, h) in enumerate([(320, 240), (257, 131)])]
    pictures, inputs = [], []
    for f in frames:
        lines, t, warped = ctx.rectify(f)
        H, _, (w, h) = L.rectification_homography(t, 3.0)
        assert warped.shape == (h, w) and len(lines) > 10
        pictures.append(check(ctx, warped, lines, H))
        inputs.append((warped, lines, H))
    got = ctx.draw_lines_batch([i[0] for i in inputs], [i[1] for i in inputs], [i[2] for i in inputs])
    for g, want in zip(got, pictures):
        np.testing.assert_array_equal(g, want)
    check(ctx, frames[0], inputs[0][1])  # and on the frame itself, as the demo draws


# ---- clean failures --------------------------------------------------------------------------------------------------


def _base(L):
    img = gray(130, 37, 14)
    lines = forty_segments(L)
    table = L.draw_table([(130, 37), (64, 16)], [(0, 130), (0, 130)], [(0, 390), (37 * 390, 192)], [(0, 40), (0, 20)])
    return img, lines, table, 37 * 390 + 16 * 192


def _edit(table, b, k, v):
    t = table.copy()
    t[b, k] = v
    return t


FAILURES = {
    "null_lines": (dict(lines=None, n_lines=40), "null lines"),
    "segments_beyond_n_lines": (dict(table=(1, 6, 25.0)), "frame 1: entry [7]"),
    "fractional": (dict(table=(0, 4, 0.5)), "frame 0: entry [4]"),
    "negative": (dict(table=(1, 2, -1.0)), "frame 1: entry [2]"),
    "beyond_2_53": (dict(table=(0, 5, 2.0 ** 53 + 2)), "frame 0: entry [5]"),
    "nan_entry": (dict(table=(0, 0, float("nan"))), "frame 0: entry [0]"),
    "short_output_stride": (dict(table=(0, 5, 389.0)), "frame 0: entry [5]"),
    "short_source_stride": (dict(table=(0, 3, 129.0)), "frame 0: entry [3]"),
    "output_beyond_region": (dict(table=(1, 4, 37 * 390 + 1.0)), "beyond dst_bytes"),
    "source_beyond_region": (dict(table=(0, 2, 1.0)), "beyond src_bytes"),
    "overlapping_outputs": (dict(table=(1, 4, 36 * 390.0)), "overlap"),
    "output_overlaps_source": (dict(dst_is_src=True), "overlaps the source"),
    "in_place_u8": (dict(in_place=True, fmt="u8"), "in place"),
    "in_place_src_bytes": (dict(in_place=True, src_bytes=4), "in place"),
    "in_place_source_entry": (dict(in_place=True, keep_sources=True), "frame 0: entry [3]"),
    "f32": (dict(fmt="f32"), "format"),
    "batch_0": (dict(batch=0), "batch < 1"),
    "H_inf": (dict(H=(1, 4, float("inf"))), "frame 1: H is not finite"),
    "H_nan": (dict(H=(0, 8, float("nan"))), "frame 0: H is not finite"),
}


@pytest.mark.parametrize("case", sorted(FAILURES))
def test_failures_leave_the_destination_untouched(L, ctx, case):
    spec, why = FAILURES[case]
    img, lines, table, dst_bytes = _base(L)
    if "table" in spec:
        table = _edit(table, *spec["table"])
    fmt = {"u8": L.PIX_U8, "f32": L.PIX_F32, "u8x3": L.PIX_U8X3}[spec.get("fmt", "u8x3" if spec.get("in_place") else "u8")]
    H = None
    if "H" in spec:
        H = np.tile(np.eye(3).reshape(-1), (2, 1))
        H[spec["H"][0], spec["H"][1]] = spec["H"][2]
    d_src = ctx.device_upload(np.concatenate([img.reshape(-1), np.full(dst_bytes, SENTINEL, np.uint8)]))
    d_dst = ctx.device_upload(np.full(dst_bytes, SENTINEL, np.uint8))
    try:
        src, src_bytes, dst = d_src, img.size, d_dst
        if spec.get("dst_is_src"):
            dst = d_src + img.size - 1  # the destination region starts on the source's last byte
        if spec.get("in_place"):
            src, src_bytes = None, spec.get("src_bytes", 0)
            if not spec.get("keep_sources"):
                table[:, 2:4] = 0
        args = L.DrawLinesArgs(None if spec.get("lines", 0) is None else lines.ctypes.data_as(C.c_void_p),
                               spec.get("n_lines", len(lines)), table.ctypes.data_as(C.c_void_p),
                               None if H is None else H.ctypes.data_as(C.c_void_p))
        rc = L.lib().lr_warp_perspective_device(ctx._h, C.c_void_p(src) if src else None, src_bytes, spec.get("batch", 2), 0, 0, 0,
                                                fmt | L.WARP_LINES, C.cast(C.byref(args), C.c_void_p), C.c_void_p(dst), dst_bytes, 0, 0, 0)
        msg = L.lib().lr_last_error().decode()
        assert rc != 0 and msg.startswith(PREFIX) and why in msg, msg
        ctx.synchronize()
        assert (ctx.device_download(d_dst, (dst_bytes,), np.uint8) == SENTINEL).all()
        assert (ctx.device_download(d_src + img.size, (dst_bytes,), np.uint8) == SENTINEL).all()
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def test_the_entry_rejects_other_option_bits_and_sizes_it_does_not_take(L, ctx):
    img, lines, table, dst_bytes = _base(L)
    d_src = ctx.device_upload(img)
    d_dst = ctx.device_upload(np.full(dst_bytes, SENTINEL, np.uint8))
    try:
        args = L.DrawLinesArgs(lines.ctypes.data_as(C.c_void_p), len(lines), table.ctypes.data_as(C.c_void_p), None)
        a = C.cast(C.byref(args), C.c_void_p)
        call = L.lib().lr_warp_perspective_device
        assert call(ctx._h, C.c_void_p(d_src), img.size, 2, 0, 0, 0, L.PIX_U8 | L.WARP_LINES | L.WARP_PACKED, a, C.c_void_p(d_dst), dst_bytes, 0, 0, 0) != 0
        assert "another option bit" in L.lib().lr_last_error().decode()
        assert call(ctx._h, C.c_void_p(d_src), img.size, 2, 130, 37, 0, L.PIX_U8 | L.WARP_LINES, a, C.c_void_p(d_dst), dst_bytes, 0, 0, 0) != 0
        assert "must be 0" in L.lib().lr_last_error().decode()
        assert call(ctx._h, C.c_void_p(d_src), img.size, 2, 0, 0, 0, L.PIX_U8 | L.WARP_LINES, None, C.c_void_p(d_dst), dst_bytes, 0, 0, 0) != 0
        ctx.synchronize()
        assert (ctx.device_download(d_dst, (dst_bytes,), np.uint8) == SENTINEL).all()
        # and the call that is in order draws both frames
        ctx.draw_lines_device(d_src, img.size, L.PIX_U8, lines, table, d_dst, dst_bytes)
        got = ctx.device_download(d_dst, (dst_bytes,), np.uint8)
        np.testing.assert_array_equal(got[:37 * 390].reshape(37, 130, 3), R.draw(img, lines))
        np.testing.assert_array_equal(got[37 * 390:].reshape(16, 64, 3), R.draw(img[:16, :64], lines[:20]))
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def test_trim_gives_the_records_back_and_the_next_call_still_draws(L, ctx):
    img = gray(130, 37, 15)
    lines = forty_segments(L)
    check(ctx, img, lines)
    ctx.trim()
    check(ctx, img, lines)
