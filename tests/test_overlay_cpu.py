"""The lines picture without a GPU: the second source (tests/numpy_overlay_ref.py) against the reference's own lines
picture (doc/image.jpg_warp_lines.jpg, as tests/golden/doc_lines_overlay.npz), the properties of the rule, draw_table, and
the recipe's --lines without a device.

The fixture was made once from the JPEG: `mask` the packed bits of the pixels whose max(R, G, B) - min(R, G, B) > 64
(62 034 of 1000 x 563), `dominant` the argmax channel of each marked pixel in row-major order, `strong` the packed bits,
over the marked pixels, of those whose chroma exceeds 128."""
import os
import subprocess

import numpy as np
import pytest

import numpy_overlay_ref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
LINE_DTYPE = O.LINE_DTYPE


def seg(x1, y1, x2, y2, g=0):
    out = np.zeros(1, LINE_DTYPE)
    out[0] = (x1, y1, x2, y2, 1.0, 0.0, g)
    return out


def segs(*rows):
    return np.concatenate([seg(*r) for r in rows])


def covered(w, h, lines, **kw):
    return R.draw(np.zeros((h, w), np.uint8), lines, with_owner=True, **kw)[1] >= 0


@pytest.fixture(scope="module")
def doc():
    lines = O.lines_from_rows(np.loadtxt(os.path.join(G, "doc_warp_lines.csv"), delimiter=","))
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    assert len(lines) == 848 and gray.shape == (563, 1000)
    picture, owner = R.draw(gray, lines, with_owner=True)
    return lines, gray, picture, owner


def test_second_source_covers_the_known_pixel_count(doc):
    """the rule's known answer on the golden lines: another count means the second source does not state the rule"""
    lines, gray, picture, owner = doc
    assert int((owner >= 0).sum()) == 130490
    bg = owner < 0
    assert (picture[bg] == gray[bg][:, None]).all()


def test_second_source_places_and_colours_as_the_reference_picture(doc):
    """That picture was drawn by an older demo (1-px strokes, smaller dots, another colour for group 3), so it pins
    placement and palette one-sidedly: everything it marks lies in what the rule covers, and what it marks strongly on
    groups 0, 1 and 2 is red, green and blue.  Measured: 10 marked pixels outside before the dilation, 0 after; shares
    0.936, 0.923, 0.918 on 17 258, 6 457 and 3 032 pixels."""
    lines, _, _, owner = doc
    fx = np.load(os.path.join(G, "doc_lines_overlay.npz"))
    h, w = (int(v) for v in fx["shape"])
    mask = np.unpackbits(fx["mask"])[: h * w].reshape(h, w).astype(bool)
    assert owner.shape == (h, w) and int(mask.sum()) == 62034 == len(fx["dominant"])
    cov = owner >= 0
    grown = cov.copy()
    grown[1:] |= cov[:-1]
    grown[:-1] |= cov[1:]
    grown[:, 1:] |= cov[:, :-1]
    grown[:, :-1] |= cov[:, 1:]
    assert int((mask & ~cov).sum()) == 10  # (the older demo's dots: all within one pixel of the rule's shapes)
    assert int((mask & ~grown).sum()) == 0
    strong = np.unpackbits(fx["strong"])[: len(fx["dominant"])].astype(bool)
    own = owner[mask]
    group = np.where(own >= 0, lines["group_id"][np.clip(own, 0, None)], -99)
    for g in (0, 1, 2):
        sel = strong & (group == g)
        share = float((fx["dominant"][sel] == g).mean())
        print("group", g, "pixels", int(sel.sum()), "share", share)
        assert sel.sum() > 1000 and share >= 0.90, (g, int(sel.sum()), share)


# ---- properties of the rule ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("L", [0, 1, 7, 40])
def test_horizontal_stroke_is_three_rows_with_a_round_cap_of_three_pixels_at_each_end(L):
    """Without the discs a horizontal segment of length L covers the three rows |y - Y1| <= 1 over the columns X1 - 1 ..
    X2 + 1: 3 (L + 1) pixels over the segment's own columns and 3 beyond each end, 3 (L + 1) + 6.  (Beyond an end the rule
    asks 4 |p|^2 <= 9, and the diagonal neighbours (+-1, +-1) have 4 |p|^2 = 8: the cap is the whole 3-pixel column, not
    its middle pixel alone -- the count 3 (L + 1) + 2 would need 4 |p|^2 <= 7.  With the discs, which the library always
    draws, the caps lie inside them either way.)"""
    m = covered(64, 21, seg(10, 10, 10 + L, 10), discs=False)
    exp = np.zeros((21, 64), bool)
    exp[9:12, 9:12 + L] = True
    np.testing.assert_array_equal(m, exp)
    assert int(m.sum()) == 3 * (L + 1) + 6
    np.testing.assert_array_equal(covered(64, 21, seg(10 + L, 10, 10, 10), discs=False), exp)  # either direction
    np.testing.assert_array_equal(covered(21, 64, seg(10, 10, 10, 10 + L), discs=False), exp.T)  # and vertical


def test_disc_has_81_pixels_and_a_zero_length_segment_is_the_disc():
    disc = covered(31, 31, seg(15, 15, 15, 15), stroke=False)
    assert int(disc.sum()) == 81
    ys, xs = np.nonzero(disc)
    assert ((xs - 15) ** 2 + (ys - 15) ** 2 <= 25).all()
    np.testing.assert_array_equal(covered(31, 31, seg(15.9, 15.2, 15.1, 15.7)), disc)  # truncation toward zero
    np.testing.assert_array_equal(covered(31, 31, seg(-0.9, -0.9, -0.2, -0.5)), covered(31, 31, seg(0, 0, 0, 0)))


def test_overlap_is_decided_by_index_not_by_group():
    a, b = (5, 8, 40, 8, 7), (20, 2, 20, 20, 1)
    for first, second in ((a, b), (b, a)):
        out, owner = R.draw(np.zeros((24, 48), np.uint8), segs(first, second), with_owner=True)
        both = covered(48, 24, seg(*first)) & covered(48, 24, seg(*second))
        assert both.sum() > 0 and (owner[both] == 1).all()
        assert (out[both] == R.colour(second[4])).all()


def test_colours_of_ungrouped_wrapped_and_last_palette_entry():
    assert R.colour(-1) == (255, 255, 255) and R.colour(-7) == (255, 255, 255)
    assert R.colour(13) == R.colour(1) == (0, 255, 0)
    assert R.colour(11) == (128, 128, 0) and R.colour(0) == (255, 0, 0)
    out = R.draw(np.full((12, 12), 9, np.uint8), seg(6, 6, 6, 6, 13))
    assert tuple(out[6, 6]) == (0, 255, 0) and tuple(out[0, 0]) == (9, 9, 9)
    # c0 is red: the u8x3 luma weights put 4899 on it
    assert (4899 * 255 + 8192) >> 14 == 76


FAR = [(-2 ** 24, -2 ** 24, 2 ** 24, 2 ** 24 - 7), (2 ** 24, -2 ** 24, -2 ** 24, 2 ** 24), (-2 ** 24, 3, 2 ** 24, 30),
       (-2 ** 24, -2 ** 24, 60, 17), (2 ** 24, 5, 2 ** 24 - 1, -2 ** 24)]


@pytest.mark.parametrize("ends", FAR)
def test_far_endpoints_agree_with_python_integers(ends):
    """int64 with the early reject against unbounded integers without it, over every pixel of a 130 x 37 frame"""
    w, h = 130, 37
    got = covered(w, h, seg(*ends))
    exp = np.array([[R.covered_python(x, y, ends) for x in range(w)] for y in range(h)])
    np.testing.assert_array_equal(got, exp)
    # and the products the reject keeps out of int64 really do not fit
    X1, Y1, X2, Y2 = ends
    c = (0 - X1) * (Y2 - Y1) - (36 - Y1) * (X2 - X1)
    if abs(X1) == abs(Y1) == 2 ** 24 and abs(c) > 2 ** 31:
        assert 4 * c * c > 2 ** 63


def test_the_segment_that_only_passes_through_the_frame_is_drawn():
    m = covered(130, 37, seg(*FAR[0]))
    # (y = x - 3.5 near the origin: in through the top row, out through the bottom one)
    assert m[0].any() and m[-1].any() and m.all(axis=1).sum() == 0 and m.any(axis=1).all()


@pytest.mark.parametrize("bad", [2.0 ** 24 + 2, -(2.0 ** 24) - 2, float("nan"), float("inf"), float("-inf")])
def test_coordinates_beyond_the_range_or_not_finite_are_skipped(bad):
    for k in range(4):
        ends = [3.0, 4.0, 20.0, 9.0]
        ends[k] = bad
        assert R.endpoints(seg(*ends)[0]) is None
        assert not covered(40, 20, seg(*ends)).any()
    assert R.endpoints(seg(2.0 ** 24, 0, -(2.0 ** 24), 0)[0]) == (2 ** 24, 0, -(2 ** 24), 0)
    # 2^24 + 1 is no float32; the first coordinate beyond the range that is one
    assert np.float32(2.0 ** 24 + 1) == np.float32(2.0 ** 24)


def test_under_H_a_segment_across_the_horizon_is_skipped():
    H = np.array([[1.0, 0, 0], [0, 1, 0], [0, 0.1, -1.0]])  # the denominator 0.1 y - 1 changes sign at y = 10
    assert R.endpoints(seg(5, 2, 9, 30)[0], H) is None
    assert R.endpoints(seg(5, 10, 9, 30)[0], H) is None  # a zero denominator
    assert R.endpoints(seg(5, 20, 9, 30)[0], H) == (5, 20, 4, 15)
    assert R.endpoints(seg(5, 2, 9, 4)[0], H) == (-6, -2, -15, -6)  # both negative: drawn
    # the skipped segment still counts in the painter's order
    lines = segs((5, 20, 9, 30, 0), (5, 2, 9, 30, 1), (5, 20, 9, 30, 2))
    _, owner = R.draw(np.zeros((40, 40), np.uint8), lines, H=H, with_owner=True)
    assert set(np.unique(owner)) == {-1, 2}


def test_rgb_background_is_copied_and_gray_is_replicated():
    rgb = np.random.default_rng(3).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    np.testing.assert_array_equal(R.draw(rgb, np.zeros(0, LINE_DTYPE)), rgb)
    gray = rgb[:, :, 0].copy()
    np.testing.assert_array_equal(R.draw(gray, np.zeros(0, LINE_DTYPE)), np.repeat(gray[:, :, None], 3, axis=2))


# ---- draw_table ------------------------------------------------------------------------------------------------------


def test_draw_table_shape_and_values():
    import librectify_amd as L

    t = L.draw_table([(130, 37), (64, 16)], [(5, 131), (9000, 64)], [(12, 400), (0, 192)], [(0, 40), (100, 0)])
    assert t.dtype == np.float64 and t.shape == (2, 8)
    np.testing.assert_array_equal(t, [[130, 37, 5, 131, 12, 400, 0, 40], [64, 16, 9000, 64, 0, 192, 100, 0]])
    np.testing.assert_array_equal(L.draw_table([(3, 2)], None, [(0, 9)], [(0, 0)]), [[3, 2, 0, 0, 0, 9, 0, 0]])
    for bad in (dict(sizes=[(0, 2)]), dict(sizes=[(3.5, 2)]), dict(outputs=[(-1, 9)]), dict(segments=[(0, 1), (1, 1)]),
                dict(sources=[(0, 2 ** 53 + 2)])):
        kw = dict(sizes=[(3, 2)], sources=[(0, 3)], outputs=[(0, 9)], segments=[(0, 0)])
        kw.update(bad)
        with pytest.raises(ValueError):
            L.draw_table(**kw)
    assert "lr_draw_lines_device" not in L.EXPORTS and L.WARP_LINES == 0x1000


# ---- the recipe ------------------------------------------------------------------------------------------------------


def test_recipe_with_lines_and_no_gpu_writes_the_csv_files_and_fails(tmp_path):
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    exe = str(tmp_path / "rectify_recipe")
    lib_dir = os.path.join(ROOT, "librectify_amd")
    src = os.path.join(ROOT, "examples", "rectify_recipe.cpp")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", src, "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-l:librectify_amd.so", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    usage = subprocess.run([exe], text=True, capture_output=True)
    assert usage.returncode == 2 and "--lines" in usage.stderr
    a = np.load(os.path.join(G, "doc_image_gray.npy"))
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes())
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, pgm, str(tmp_path / "out"), "--lines"], text=True, capture_output=True, env=env)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "lines picture failed" in r.stderr and "unknown or incomplete option" not in r.stderr
    assert open(str(tmp_path / "out_lines.csv")).read() == ""
    assert len(open(str(tmp_path / "out_tform.csv")).read().split()) == 6
    assert not os.path.exists(str(tmp_path / "out_lines.ppm"))
    assert L.LIB_PATH.startswith(lib_dir)
