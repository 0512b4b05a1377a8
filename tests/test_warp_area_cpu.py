"""LR_WARP_AREA without a GPU: the second source (tests/numpy_warp_area_ref.py) on the pure shrink, where it is the rounded box
mean and, for a power of two, PIL's Image.reduce; S = 1 against the plain reference; the header's lr_area_fine_map and
lr_shrink_homography, compiled on their own, against their Python twins; shrink_homography's invariants; the table builders."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import numpy_warp_area_ref as RA
import numpy_warp_cubic_ref as RC
import numpy_warp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
OW, OH = 50, 40


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L

    return L


@pytest.fixture(scope="module")
def photograph():
    return np.asarray(Image.open(os.path.join(G, "doc_image.jpg")).convert("RGB"))


def shrink_map(S):
    t = (S - 1) / 2.0
    return np.array([[S, 0, t], [0, S, t], [0, 0, 1.0]])


@pytest.mark.parametrize("S", [2, 3, 4, 5, 8])
def test_the_pure_shrink_is_the_rounded_box_mean(L, photograph, S):
    assert np.array_equal(RA.fine_map(shrink_map(S), S), np.eye(3))  # exactly
    assert np.array_equal(L.area_fine_map(shrink_map(S), S), np.eye(3))
    src = np.ascontiguousarray(photograph[100: 100 + S * OH, 60: 60 + S * OW])
    assert src.shape == (S * OH, S * OW, 3)
    for frame in (src, np.ascontiguousarray(src[..., 1])):
        got = RA.warp_area(frame, shrink_map(S), OW, OH, S)
        blocks = frame.astype(np.int64).reshape((OH, S, OW, S) + frame.shape[2:]).sum(axis=(1, 3))
        exp = (2 * blocks + S * S) // (2 * S * S)
        assert got.dtype == np.uint8 and np.array_equal(got, exp)
        pil = np.asarray(Image.fromarray(frame).reduce(S))
        diff = np.abs(got.astype(int) - pil.astype(int))
        print("S = %d, %s: differs from Image.reduce on %.2f %% of the bytes, by at most %d" % (S, frame.shape, 100.0 * (diff != 0).mean(), diff.max()))
        if S in (2, 4, 8):
            assert np.array_equal(got, pil)
        else:  # (PIL multiplies by a fixed-point reciprocal; the cap only keeps the test from hiding a gross error)
            assert diff.max() <= 1 and (diff != 0).mean() <= 0.15
    f32 = (src[..., 0].astype(np.float32) - 100.0) / 7.0
    got = RA.warp_area(f32, shrink_map(S), OW, OH, S)
    acc = np.zeros((OH, OW), np.float32)
    for j in range(S):
        for i in range(S):
            acc = acc + f32[j::S, i::S]
    assert got.dtype == np.float32 and got.tobytes() == (acc / np.float32(S * S)).tobytes()
    assert np.abs(got - f32.astype(np.float64).reshape(OH, S, OW, S).mean(axis=(1, 3))).max() < 1e-4


def test_a_factor_of_one_is_the_plain_rule(L):
    M = np.array([[0.9, -0.2, -3.0], [0.15, 1.1, -4.5], [0.0004, -0.0007, 1.0]])
    assert np.array_equal(L.area_fine_map(M, 1), M) and np.array_equal(RA.fine_map(M, 1), M)
    rng = np.random.default_rng(3)
    for src in (rng.integers(0, 256, (17, 23), dtype=np.uint8), rng.integers(0, 256, (17, 23, 3), dtype=np.uint8),
                rng.standard_normal((17, 23)).astype(np.float32)):
        for cubic, old in ((False, R.warp), (True, RC.warp)):
            got, exp = RA.warp_area(src, M, 37, 29, 1, cubic=cubic), old(src, M, 37, 29)
            assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes()


def test_the_sub_samples_lie_where_the_rule_says(L):
    """pixel (S x + i, S y + j) under F is destination point (x + (i + 0.5) / S - 0.5, y + (j + 0.5) / S - 0.5) under M"""
    M = np.array([[1.1, 0.07, -3.2], [-0.05, 0.93, 2.5], [1e-4, -2e-4, 1.0]])
    for S in (2, 3, 5, 8):
        F = L.area_fine_map(M, S)
        assert np.array_equal(F, RA.fine_map(M, S))
        for x, y, i, j in ((0, 0, 0, 0), (7, 3, S - 1, 1), (69, 18, S // 2, S - 1)):
            p = F @ np.array([S * x + i, S * y + j, 1.0])
            q = M @ np.array([x + (i + 0.5) / S - 0.5, y + (j + 0.5) / S - 0.5, 1.0])
            np.testing.assert_allclose(p, q, rtol=1e-13, atol=1e-12)


CXX_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "librectify_amd.h"
static void put(const double* v, int n) {
    for (int i = 0; i < n; ++i) {
        unsigned long long b;
        std::memcpy(&b, &v[i], 8);
        std::printf("%016llx ", b);
    }
}
// stdin, per line: "F" S and nine hex doubles M, or "S" out_width out_height max_size and eighteen hex doubles H, M;
// prints the fine map, or rc, H_out, M_out (in place: H_out is H, M_out is M), new size and S
int main() {
    char kind[4];
    while (std::scanf("%3s", kind) == 1) {
        double H[9], M[9], F[9];
        if (kind[0] == 'F') {
            int S;
            if (std::scanf("%d", &S) != 1) return 99;
            for (int i = 0; i < 9; ++i)
                if (std::scanf("%la", &M[i]) != 1) return 99;
            lr_area_fine_map(M, S, F);
            put(F, 9);
            lr_area_fine_map(M, S, M);  // (F may be M)
            if (std::memcmp(F, M, sizeof F) != 0) return 98;
        } else {
            int ow, oh, max_size, nw = -1, nh = -1, S = -1;
            if (std::scanf("%d %d %d", &ow, &oh, &max_size) != 3) return 99;
            for (int i = 0; i < 9; ++i)
                if (std::scanf("%la", &H[i]) != 1) return 99;
            for (int i = 0; i < 9; ++i)
                if (std::scanf("%la", &M[i]) != 1) return 99;
            double M2[9];
            int S2 = -1;
            const int rc2 = lr_shrink_homography(NULL, M, ow, oh, max_size, NULL, M2, NULL, NULL, &S2);  // (NULL-tolerant)
            const int rc = lr_shrink_homography(H, M, ow, oh, max_size, H, M, &nw, &nh, &S);
            if (rc != rc2 || (rc == 0 && (S != S2 || std::memcmp(M, M2, sizeof M) != 0))) return 98;
            std::printf("%d ", rc);
            put(H, 9);
            put(M, 9);
            std::printf("%d %d %d", nw, nh, S);
        }
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def area_exe(tmp_path_factory):
    """the header's inlines in a program of their own, without contraction like the library itself"""
    d = tmp_path_factory.mktemp("area")
    src, exe = str(d / "area.cpp"), str(d / "area")
    with open(src, "w") as f:
        f.write(CXX_PROGRAM)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", src, "-I", os.path.join(ROOT, "include"), "-o", exe])
    return exe


def _maps(rng, n):
    Ms = [np.array([[1.1, 0.07, -3.2], [-0.05, 0.93, 2.5], [1e-4, -2e-4, 1.0]]), np.eye(3), np.array([[1e300, 1e300, -1e308], [1e-310, 3.0, -0.0], [0.0, -0.0, 1.0]])]
    while len(Ms) < n:
        Ms.append(rng.standard_normal((3, 3)) * 10.0 ** rng.integers(-6, 7, (3, 3)))
    return Ms


def test_header_inlines_and_python_twins_agree(L, area_exe):
    rng = np.random.default_rng(11)
    hexes = lambda a: " ".join(float(v).hex() for v in np.asarray(a).reshape(-1))  # noqa: E731
    bits = lambda words: np.array([int(v, 16) for v in words], np.uint64)  # noqa: E731
    fine = [(S, M) for M in _maps(rng, 12) for S in range(1, 9)]
    cases = []
    for k, M in enumerate(_maps(rng, 40)):
        ow, oh = (int(v) for v in rng.integers(1, 9000, 2))
        max_size = int(rng.integers(1, 2 * max(ow, oh)))
        if k == 3:
            ow, oh, max_size = 2 ** 31 - 1, 7, 2 ** 31 - 2  # (the products need 64 bits)
        if k == 4:
            ow, oh, max_size = 5000, 3, 100  # (a side that would fall below 1; S capped at 8)
        cases.append((ow, oh, max_size, np.linalg.inv(M) if k not in (2,) and abs(np.linalg.det(M)) > 1e-200 else np.eye(3), M))
    text = "".join("F %d %s\n" % (S, hexes(M)) for S, M in fine) + "".join("S %d %d %d %s %s\n" % (ow, oh, ms, hexes(H), hexes(M)) for ow, oh, ms, H, M in cases)
    lines = subprocess.run([area_exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(lines) == len(fine) + len(cases)
    with np.errstate(all="ignore"):
        for (S, M), line in zip(fine, lines):
            got, exp = bits(line.split()), L.area_fine_map(M, S)
            nan = np.isnan(exp).reshape(-1)
            assert np.array_equal(np.isnan(got.view(np.float64)), nan) and np.array_equal(got[~nan], exp.reshape(-1).view(np.uint64)[~nan]), (S, M)
        shrunk = 0
        for (ow, oh, ms, H, M), line in zip(cases, lines[len(fine):]):
            words = line.split()
            H_out, M_out, size, S = L.shrink_homography(H, M, (ow, oh), ms)
            assert int(words[0]) == 0 and [int(v) for v in words[19:]] == [size[0], size[1], S], (ow, oh, ms, words[19:], size, S)
            for got, exp in ((bits(words[1:10]), H_out), (bits(words[10:19]), M_out)):
                nan = np.isnan(exp).reshape(-1)
                assert np.array_equal(np.isnan(got.view(np.float64)), nan) and np.array_equal(got[~nan], exp.reshape(-1).view(np.uint64)[~nan])
            shrunk += S > 1
        assert shrunk > 10
    # what the header refuses, the twin refuses
    bad = [(1, 0, 0, 5, np.eye(3)), (1, 5, 0, 5, np.eye(3)), (1, 5, 5, 0, np.eye(3)), (1, 5, 5, 5, np.array([[1, 0, 0], [0, np.nan, 0], [0, 0, 1.0]])),
           (1, 5, 5, 5, np.array([[1, 0, 0], [0, 1, np.inf], [0, 0, 1.0]]))]
    text = "".join("S %d %d %d %s %s\n" % (ow, oh, ms, hexes(np.eye(3)), hexes(M)) for _, ow, oh, ms, M in bad)
    lines = subprocess.run([area_exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for (rc, ow, oh, ms, M), line in zip(bad, lines):
        words = line.split()
        assert int(words[0]) == rc and words[19:] == ["-1", "-1", "-1"]
        assert np.array_equal(bits(words[10:19]).view(np.float64), M.reshape(-1), equal_nan=True)  # (nothing written)
        with pytest.raises(ValueError, match="shrink_homography"):
            L.shrink_homography(np.eye(3), M, (ow, oh), ms)
    with pytest.raises(ValueError, match="shrink_homography"):
        L.shrink_homography(None, None, (5, 5), 3)


def test_shrink_homography_invariants(L):
    rng = np.random.default_rng(2)
    M = np.array([[1.1, 0.07, -3.2], [-0.05, 0.93, 2.5], [1e-4, -2e-4, 1.0]])
    H = np.linalg.inv(M)
    H = H / H[2, 2]
    for _ in range(200):
        ow, oh = (int(v) for v in rng.integers(1, 12000, 2))
        max_size = int(rng.integers(1, 4000))
        H_out, M_out, (nw, nh), S = L.shrink_homography(H, M, (ow, oh), max_size)
        if max(ow, oh) <= max_size:  # the identity when the picture already fits
            assert (nw, nh, S) == (ow, oh, 1) and np.array_equal(H_out, H) and np.array_equal(M_out, M)
            continue
        assert 1 <= nw <= max_size and 1 <= nh <= max_size and 1 <= S <= 8
        assert max(nw, nh) == max_size  # (the longer side takes the whole bound)
        sx, sy = ow / nw, oh / nh
        assert S == min(8, int(np.ceil(max(sx, sy)))) and S >= 2
        assert H_out[2, 2] == H[2, 2] == 1.0
        P = H_out @ M_out
        assert np.abs(P / P[2, 2] - np.eye(3)).max() < 1e-9
        # destination pixel (x, y) of the small picture is centred on the footprint [sx x, sx (x + 1)) of the large one
        for x, y in ((0, 0), (nw - 1, nh - 1), (nw // 2, nh // 3)):
            p = M_out @ np.array([x, y, 1.0])
            q = M @ np.array([sx * (x + 0.5) - 0.5, sy * (y + 0.5) - 0.5, 1.0])
            np.testing.assert_allclose(p, q, rtol=1e-12, atol=1e-9)
    assert L.shrink_homography(None, M, (100, 50), 100)[0] is None and L.shrink_homography(H, None, (100, 50), 10)[1] is None
    Hc, Mc = H.copy(), M.copy()
    L.shrink_homography(Hc, Mc, (3000, 2000), 100)
    assert np.array_equal(Hc, H) and np.array_equal(Mc, M)  # (the inputs are left as they were)


def test_table_shapes_with_area(L):
    Ms = np.stack([np.eye(3)] * 3)
    sizes = np.array([(40, 30), (17, 5), (64, 16)])
    sources = np.array([(50, 40, 0, 52), (20, 10, 2080, 20), (70, 20, 2280, 72)])
    lens = L.Lens(30.0, 30.0, 10.0, 8.0, -0.1)
    plain, total = L.warp_table(Ms, sizes, 1)
    for border, lensed, cols in ((None, None, 14), ("reflect", None, 15), (None, lens, 23), ("reflect", lens, 24)):
        t, end = L.warp_table(Ms, sizes, 1, border=border, lens=lensed, area=[1, 4, 8])
        assert t.shape == (3, cols) and end == total and np.array_equal(t[:, :13], plain) and t[:, -1].tolist() == [1.0, 4.0, 8.0]
        assert np.array_equal(t[:, :-1], L.warp_table(Ms, sizes, 1, border=border, lens=lensed)[0])
    ragged, total = L.ragged_table(Ms, sizes, sources, 1)
    for border, lensed, cols in ((None, None, 19), ("replicate", None, 19), (None, lens, 28), ("replicate", lens, 28)):
        t, end = L.ragged_table(Ms, sizes, sources, 1, border=border, lens=lensed, area=3)
        assert t.shape == (3, cols) and end == total and t[:, -1].tolist() == [3.0] * 3
        assert np.array_equal(t[:, :-1], L.ragged_table(Ms, sizes, sources, 1, border=border, lens=lensed)[0])
        assert t[:, 17].tolist() == [float(L.border_word(border, L.PIX_U8))] * 3  # (the border word stays entry [17])
    assert L.warp_table(Ms, sizes, 1, area=np.int64(2))[0][:, -1].tolist() == [2.0] * 3
    for fmt, M, lensed, border, n in ((0, np.eye(3), None, None, 10), (1, np.eye(3), None, "reflect", 11), (2, np.eye(3), lens, None, 19), (0, np.eye(3), lens, "reflect", 20)):
        bits, row = L._border_bit_and_map(border, fmt, M, "test", lensed, 5)
        assert bits & L.WARP_AREA and len(row) == n and row[-1] == 5.0
    assert L.WARP_AREA & (L.WARP_PREPARE | L.WARP_PACKED | L.WARP_RAGGED | L.WARP_LINES | L.WARP_JPEG | L.WARP_JPEG_DECODE | L.WARP_CUBIC | L.WARP_BORDER
                          | L.WARP_LENS | L.JPEG_SCALED | L.JPEG_ANY_SAMPLING | 0x400 | 0x10000 | 0x200000 | (1 << 30) | 0xFF) == 0


@pytest.mark.parametrize("area", [0, 9, -1, 2.5, 2.0, float("nan"), True, "2", [1, 2], [1, 2, 3, 4], [1, 2, 9], [1, None, 2], object()])
def test_table_refusals_with_area(L, area):
    Ms = np.stack([np.eye(3)] * 3)
    sizes = np.array([(40, 30), (17, 5), (64, 16)])
    sources = np.array([(50, 40, 0, 52), (20, 10, 2080, 20), (70, 20, 2280, 72)])
    with pytest.raises(ValueError, match="warp_table"):
        L.warp_table(Ms, sizes, 1, area=area)
    with pytest.raises(ValueError, match="ragged_table"):
        L.ragged_table(Ms, sizes, sources, 1, area=area)
    if not isinstance(area, list):
        with pytest.raises(ValueError, match="test"):
            L._border_bit_and_map(None, 0, np.eye(3), "test", None, area)
    with pytest.raises(ValueError, match="area_fine_map"):
        L.area_fine_map(np.eye(3), 0)
    with pytest.raises(ValueError, match="area_fine_map"):
        L.area_fine_map(np.eye(3), 9)
