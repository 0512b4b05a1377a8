"""LR_WARP_BORDER and the constrained crop without a GPU: the second source against the unbordered ones and against np.pad,
the tables and border words of the Python package, the crop on three transforms (no border inside it, whatever the border
rule), and the header's lr_crop_homography, compiled as C, against its Python twin."""
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_border_ref as RB
import numpy_warp_cubic_ref as RC
import numpy_warp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

BORDERS = [(RB.CONSTANT, 0), (RB.CONSTANT, 255), (RB.REPLICATE, 0), (RB.REFLECT, 0), (RB.REFLECT_101, 0)]


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


def source(fmt, w, h, seed):
    rng = np.random.default_rng(seed)
    if fmt == 2:
        return rng.standard_normal((h, w)).astype(np.float32)
    return rng.integers(0, 256, (h, w, 3) if fmt == 1 else (h, w), dtype=np.uint8)


def test_constant_zero_is_the_unbordered_rule():
    M = np.array([[0.9, -0.2, -3.0], [0.15, 1.1, -4.5], [0.0004, -0.0007, 1.0]])
    for fmt in (0, 1, 2):
        src = source(fmt, 23, 17, fmt)
        for cubic, old in ((False, R.warp), (True, RC.warp)):
            got = RB.warp(src, M, 37, 29, RB.CONSTANT, (0, 0, 0) if fmt == 1 else 0, cubic)
            exp = old(src, M, 37, 29)
            assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), (fmt, cubic)


@pytest.mark.parametrize("mode,pad", [(RB.REPLICATE, "edge"), (RB.REFLECT, "symmetric"), (RB.REFLECT_101, "reflect")])
def test_index_rule_is_np_pad(mode, pad):
    for n in (1, 2, 3, 7):
        p = np.arange(-5 * n, 5 * n + 1)
        padded = np.pad(np.arange(n), 5 * n + 1, mode=pad)
        np.testing.assert_array_equal(RB.index(p, n, mode), padded[p + 5 * n + 1])
    # an integer translation of a 5 x 4 source is the padded array
    src = source(0, 5, 4, 9)
    M = np.array([[1.0, 0, -11], [0, 1, -9], [0, 0, 1]])
    np.testing.assert_array_equal(RB.warp(src, M, 27, 22, mode), np.pad(src, ((9, 9), (11, 11)), mode=pad))
    np.testing.assert_array_equal(RB.warp(src, M, 27, 22, mode, cubic=True), np.pad(src, ((9, 9), (11, 11)), mode=pad))


def test_constant_value_is_np_pad():
    src = source(1, 5, 4, 3)
    M = np.array([[1.0, 0, -3], [0, 1, -2], [0, 0, 1]])
    exp = np.stack([np.pad(src[..., c], ((2, 2), (3, 3)), constant_values=v) for c, v in enumerate((7, 200, 31))], axis=-1)
    np.testing.assert_array_equal(RB.warp(src, M, 11, 8, RB.CONSTANT, (7, 200, 31)), exp)


def test_tables_with_and_without_border(L):
    Ms = np.stack([np.eye(3)] * 3)
    sizes = np.array([(5, 4), (7, 3), (2, 2)])
    plain, total = L.warp_table(Ms, sizes, 3)
    with_b, total_b = L.warp_table(Ms, sizes, 3, border="reflect")
    assert plain.shape == (3, 13) and with_b.shape == (3, 14) and total == total_b
    np.testing.assert_array_equal(with_b[:, :13], plain)
    assert with_b[:, 13].tolist() == [2.0, 2.0, 2.0]
    per_frame, _ = L.warp_table(Ms, sizes, 3, border=[None, ("constant", (1, 2, 3)), "reflect101"])
    assert per_frame[:, 13].tolist() == [0.0, 8.0 * (1 | 2 << 8 | 3 << 16), 4.0]
    zero, _ = L.warp_table(Ms, sizes, 3, border=[None] * 3)
    assert zero.shape == (3, 14) and not zero[:, 13].any()

    sources = np.array([(9, 9, 0, 9), (9, 9, 81, 9), (4, 4, 200, 4)])
    rag, _ = L.ragged_table(Ms, sizes, sources, 1)
    rag_b, _ = L.ragged_table(Ms, sizes, sources, 1, border=["replicate", ("constant", 255), None])
    assert rag.shape == rag_b.shape == (3, 18) and not rag[:, 17].any()
    np.testing.assert_array_equal(rag_b[:, :17], rag[:, :17])
    assert rag_b[:, 17].tolist() == [1.0, 8.0 * 255, 0.0]
    f32, _ = L.ragged_table(Ms, sizes, sources * np.array([1, 1, 4, 4]), 4, border=("constant", -1.5))
    assert f32[0, 17] == 8.0 * int(np.float32(-1.5).view(np.uint32))
    for bad in ("wrap", ["reflect"], [None] * 4, ("constant", 256), 3):
        with pytest.raises(ValueError, match="warp_table"):
            L.warp_table(Ms, sizes, 1, border=bad)
    with pytest.raises(ValueError, match="ragged_table"):
        L.ragged_table(Ms, sizes, sources, 1, border=("replicate", 1))


def test_border_word_accepts_and_rejects_what_the_library_does(L):
    assert L.WARP_BORDER == 0x40000
    assert (L.BORDER_CONSTANT, L.BORDER_REPLICATE, L.BORDER_REFLECT, L.BORDER_REFLECT_101) == (0, 1, 2, 4)
    for fmt in (L.PIX_U8, L.PIX_U8X3, L.PIX_F32):
        assert L.border_word(None, fmt) == 0 and L.border_word("constant", fmt) == 0
        assert [L.border_word(m, fmt) for m in ("replicate", "reflect", "reflect101")] == [1, 2, 4]
    assert L.border_word(("constant", 0), L.PIX_U8) == 0 and L.border_word(("constant", 255), L.PIX_U8) == 8 * 255
    assert L.border_word(("constant", (255, 0, 128)), L.PIX_U8X3) == 8 * (255 | 128 << 16)
    assert L.border_word(("constant", 1.0), L.PIX_F32) == 8 * 0x3F800000
    assert L.border_word(("constant", -0.0), L.PIX_F32) == 8 * 0x80000000
    for word, fmt in ((RB.word(RB.CONSTANT, 17, np.zeros((1, 1), np.uint8)), 0), (RB.word(RB.CONSTANT, (1, 2, 3), np.zeros((1, 1, 3), np.uint8)), 1),
                      (RB.word(RB.CONSTANT, 0.25, np.zeros((1, 1), np.float32)), 2)):
        assert word == L.border_word(("constant", [17, (1, 2, 3), 0.25][fmt]), fmt)
    bad = [("wrap", 0), ("transparent", 0), (("constant", 256), 0), (("constant", -1), 0), (("constant", 1.5), 0), (("constant", True), 0),
           (("constant", 7), 1), (("constant", (1, 2)), 1), (("constant", (1, 2, 256)), 1), (("constant", float("inf")), 2),
           (("constant", float("nan")), 2), (("constant", 1e39), 2), (("replicate", 0), 0), (("reflect", 5), 0), (3, 0), (("constant",), 0)]
    for spec, fmt in bad:
        with pytest.raises(ValueError):
            L.border_word(spec, fmt)
    with pytest.raises(ValueError):
        L.border_word("reflect", 3)


# ---- the constrained crop ----

def golden_corners():
    rows = [[float(v) for v in line.split(",")] for line in open(os.path.join(G, "doc_warp_tform.csv"))]
    return [tuple(r[:2]) for r in rows[:4]]


def crop_cases():
    return [(golden_corners(), 1000, 664),
            ([(-9.5, 4.25), (101, -7.5), (6, 66), (88.5, 52)], 97, 61),
            ([(3, -12), (55, 2), (-8, 99), (70, 90)], 61, 97)]


def transform(L, corners, width, height):
    t = L.ImageTransform()
    t.width, t.height = width, height
    t.top_left, t.top_right, t.bottom_left, t.bottom_right = [L.Point(float(x), float(y), 0.0) for x, y in corners]
    return t


@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("cubic", [False, True])
def test_crop_holds_no_border(L, case, cubic):
    corners, w, h = crop_cases()[case]
    m = 1 if cubic else 0
    H, M, (ow, oh) = L.rectification_homography(transform(L, corners, w, h), 3.0)
    H2, M2, (x0, y0, cw, ch) = L.crop_homography(H, M, w, h, (ow, oh), margin=m)
    M_ref, rect, (bounds, s, c, a, Q) = RB.crop(H, M, w, h, ow, oh, m)
    print("transform %d, margin %d: output %d x %d, crop %d x %d at (%d, %d), s = %.6f" % (case, m, ow, oh, cw, ch, x0, y0, s))
    assert rect == (x0, y0, cw, ch) and cw >= 1 and ch >= 1
    np.testing.assert_array_equal(M2, M_ref)
    assert H2[2, 2] == 1.0
    np.testing.assert_allclose(H2 @ M2 / (H2 @ M2)[2, 2], np.eye(3), atol=1e-9)
    assert 0 <= x0 and x0 + cw <= ow and 0 <= y0 and y0 + ch <= oh
    assert a == w / h

    # every crop pixel maps inside [m, w - 1 - m] x [m, h - 1 - m]: in the warp's own fixed-point coordinates
    X, Y = R.fixed_coords(M2, cw, ch)
    assert X.min() >= 32 * m and X.max() <= 32 * (w - 1 - m) and Y.min() >= 32 * m and Y.max() <= 32 * (h - 1 - m)

    # at least one of the eight bounds is tight: s is one of them, and the rectangle of half-height s + 1 no longer fits --
    # one of its corners leaves the window or the quadrilateral (a point is inside Q where it is on one side of all edges)
    assert min(bounds) == s and s > 0
    grown = [(c[0] + sx * (s + 1) * a, c[1] + sy * (s + 1)) for sx in (-1, 1) for sy in (-1, 1)]

    def fits(x, y):
        e, d = np.roll(Q, -1, axis=0) - Q, np.array([x, y]) - Q
        side = e[:, 0] * d[:, 1] - e[:, 1] * d[:, 0]
        return 0 <= x <= ow - 1 and 0 <= y <= oh - 1 and ((side >= 0).all() or (side <= 0).all())

    assert not all(fits(x, y) for x, y in grown)
    assert all(fits(x, y) for x in (x0, x0 + cw - 1) for y in (y0, y0 + ch - 1))

    # the crop is the same picture under every border rule
    src = source(0, w, h, 100 + case)
    pictures = [RB.warp(src, M2, cw, ch, mode, value, cubic) for mode, value in BORDERS]
    for p in pictures[1:]:
        assert p.tobytes() == pictures[0].tobytes()
    # ... which the uncropped picture is not
    if case:
        full = [RB.warp(src, M, ow, oh, mode, value, cubic) for mode, value in ((RB.CONSTANT, 0), (RB.REPLICATE, 0))]
        assert (full[0] != full[1]).mean() > 0.05


C_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "librectify_amd.h"
/* argv: 9 H, 9 M, width height out_width out_height margin aspect; prints the code and, on 0, the outputs as hex floats */
int main(int argc, char** argv) {
    double H[9], M[9], Ho[9], Mo[9], aspect;
    int i, v[5], x0 = -1, y0 = -1, cw = -1, ch = -1, rc;
    if (argc != 25) return 99;
    for (i = 0; i < 9; ++i) { H[i] = strtod(argv[1 + i], 0); M[i] = strtod(argv[10 + i], 0); }
    for (i = 0; i < 5; ++i) v[i] = atoi(argv[19 + i]);
    aspect = strtod(argv[24], 0);
    rc = lr_crop_homography(H, M, v[0], v[1], v[2], v[3], v[4], aspect, Ho, Mo, &x0, &y0, &cw, &ch);
    printf("%d\n", rc);
    if (rc == 0) {
        printf("%d %d %d %d\n", x0, y0, cw, ch);
        for (i = 0; i < 9; ++i) printf("%a %a\n", Ho[i], Mo[i]);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def crop_exe(tmp_path_factory):
    """the header compiled as C (it must stay C), without contraction like the library itself"""
    d = tmp_path_factory.mktemp("crop")
    src, exe = str(d / "crop.c"), str(d / "crop")
    with open(src, "w") as f:
        f.write(C_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-x", "c", src, "-I",
                           os.path.join(ROOT, "include"), "-lm", "-o", exe])
    return exe


def run_c(exe, H, M, w, h, ow, oh, margin, aspect):
    args = [float(v).hex() for v in np.asarray(H, np.float64).reshape(9)] + [float(v).hex() for v in np.asarray(M, np.float64).reshape(9)]
    args += [str(int(v)) for v in (w, h, ow, oh, margin)] + [float(aspect).hex()]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.split("\n")
    rc = int(out[0])
    if rc:
        return rc, None
    rect = tuple(int(v) for v in out[1].split())
    vals = np.array([[float.fromhex(v) for v in line.split()] for line in out[2:11]])
    return 0, (vals[:, 0].reshape(3, 3), vals[:, 1].reshape(3, 3), rect)


def test_c_header_and_python_twin_agree(L, crop_exe):
    for corners, w, h in crop_cases():
        H, M, (ow, oh) = L.rectification_homography(transform(L, corners, w, h), 3.0)
        for margin, aspect in ((0, 0.0), (1, 0.0), (0, 1.0), (1, 2.5), (0, -3.0)):
            rc, got = run_c(crop_exe, H, M, w, h, ow, oh, margin, aspect)
            assert rc == 0
            H2, M2, rect = L.crop_homography(H, M, w, h, (ow, oh), margin=margin, aspect=aspect)
            assert got[2] == rect
            assert got[0].tobytes() == H2.tobytes() and got[1].tobytes() == M2.tobytes()
    assert L.crop_homography(H, M, w, h, (ow, oh))[2] == L.crop_homography(H, M, w, h, (ow, oh), 0, None)[2]

    # one input per failure class, the same code from both
    I = np.eye(3)
    nan_H = I.copy()
    nan_H[0, 1] = np.nan
    zero_den = np.array([[1.0, 0, 0], [0, 1, 0], [-0.1, 0, 1]])     # the denominator is 0 at the corner (10, 0)
    mixed = np.array([[1.0, 0, 0], [0, 1, 0], [-0.2, 0, 1]])         # ... and changes sign across x = 5
    far = np.array([[1.0, 0, 500], [0, 1, 0], [0, 0, 1]])            # the picture lies outside the window
    cases = [
        (1, (nan_H, I, 11, 11, 11, 11, 0, 0.0)),
        (1, (I, I, 11, 11, 11, 11, 0, float("inf"))),
        (1, (I, I, 11, 11, 0, 11, 0, 0.0)),
        (2, (I, I, 3, 11, 3, 11, 1, 0.0)),
        (2, (I, I, 11, 1, 11, 1, 0, 0.0)),
        (3, (zero_den, I, 11, 11, 11, 11, 0, 0.0)),
        (3, (mixed, I, 11, 11, 11, 11, 0, 0.0)),
        (4, (np.array([[1.0, 1, 0], [1, 1, 0], [0, 0, 1]]), I, 11, 11, 40, 40, 0, 0.0)),  # rank 2: all points on a line
        (5, (far, I, 11, 11, 11, 11, 0, 0.0)),
    ]
    for code, (Hc, Mc, w, h, ow, oh, margin, aspect) in cases:
        rc, _ = run_c(crop_exe, Hc, Mc, w, h, ow, oh, margin, aspect)
        assert rc == code, (code, rc)
        with pytest.raises(L.LibrectifyError) as e:
            L.crop_homography(Hc, Mc, w, h, (ow, oh), margin=margin, aspect=aspect)
        assert e.value.code == code
    # the identity on an 11 x 11 source: the whole picture, and with a margin all but a pixel all round
    assert run_c(crop_exe, I, I, 11, 11, 11, 11, 0, 0.0)[1][2] == (0, 0, 11, 11) == L.crop_homography(I, I, 11, 11, (11, 11))[2]
    assert L.crop_homography(I, I, 11, 11, (11, 11), margin=1)[2] == (1, 1, 9, 9)
