"""LR_WARP_LENS_MODEL without a GPU: the second source (tests/numpy_warp_lens_model_ref.py) against the nine-entry reference
it extends, its arctangent against math.atan, the fisheye against a restatement of cv::fisheye::distortPoints, model 0 against
OpenCV's closed form, the header's lr_lens_distort_model and lr_lens_atan, compiled on their own, against their Python twins,
and the table builders."""
import math
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_lens_model_ref as RM
import numpy_warp_lens_ref as RL
import numpy_warp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_M52 = 2.0 ** -52


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L

    return L


def random_map(rng, w, h):
    """a perspective map of a w x h output: near the identity, with a shear, a shift and a little perspective"""
    return np.array([[rng.uniform(0.7, 1.3), rng.uniform(-0.2, 0.2), rng.uniform(-20, 20)],
                     [rng.uniform(-0.2, 0.2), rng.uniform(0.7, 1.3), rng.uniform(-20, 20)],
                     [rng.uniform(-0.5, 0.5) / w, rng.uniform(-0.5, 0.5) / h, 1.0]])


def test_model_0_rows_with_zeros_behind_k3_are_the_nine_entry_rule():
    rng = np.random.default_rng(11)
    w, h = 61, 47
    for trial in range(200):
        M = random_map(rng, w, h)
        f = rng.uniform(20, 200)
        nine = (f, f * rng.uniform(0.9, 1.1), rng.uniform(0, w), rng.uniform(0, h), rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2),
                rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(-0.1, 0.1))
        if trial % 5 == 0:
            nine = nine[:6] + (0.0, 0.0) + nine[8:]  # (no tangential terms)
        zeros = tuple(rng.choice([0.0, -0.0], 7))
        X, Y = RM.fixed_coords(M, w, h, nine + zeros + (0.0,))
        X0, Y0 = RL.fixed_coords(M, w, h, nine)
        assert np.array_equal(X, X0) and np.array_equal(Y, Y0), trial
    # twelve zeros of either sign: the plain rule, by definition
    for zeros in ((0.0,) * 12, (-0.0, 0.0) * 6):
        X, Y = RM.fixed_coords(M, w, h, (31.5, 27.25, 11.0, 8.5) + zeros + (0.0,))
        X0, Y0 = R.fixed_coords(M, w, h)
        assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
    assert not RM.has_lens((1.0, 1.0, 0.0, 0.0) + (-0.0,) * 12 + (0.0,)) and RM.has_lens((1.0, 1.0, 0.0, 0.0) + (0.0,) * 12 + (1.0,))


def atan_sample():
    rng = np.random.default_rng(3)
    r = 10.0 ** rng.uniform(-12.0, 6.0, 800000)
    return np.sort(np.concatenate([r, np.arange(9) / 8.0, [0.0, 1.0, 1e300]]))


def test_atan_is_within_2_to_minus_52_of_math_atan_and_monotone(L):
    r = atan_sample()
    got = RM.atan(r)
    exp = np.array([math.atan(v) for v in r])
    err = np.abs(got - exp).max()
    print("ATAN: largest absolute difference from math.atan %.3e (2^-52 = %.3e) over %d values" % (err, TWO_M52, len(r)))
    assert err <= TWO_M52
    assert (np.diff(got) >= 0.0).all()
    assert RM.atan(0.0) == 0.0 and not np.signbit(RM.atan(0.0))
    assert RM.atan(np.inf) == RM.PI_2 and np.isnan(RM.atan(np.nan))
    assert np.array_equal(RM.atan(np.arange(9) / 8.0), RM.A)  # (the table points are the table)
    # the package's twin is the same function, bit for bit
    assert np.array_equal(L.lens_atan(r).view(np.uint64), got.view(np.uint64))


def fisheye_points(lens, u, v):
    """cv::fisheye::distortPoints as its documentation writes it, with NumPy's arctangent: shared with nothing"""
    fx, fy, cx, cy, k1, k2, k3, k4 = lens
    a, b = (u - cx) / fx, (v - cy) / fy
    r = np.hypot(a, b)
    theta = np.arctan(r)
    theta_d = theta * (1.0 + k1 * theta ** 2 + k2 * theta ** 4 + k3 * theta ** 6 + k4 * theta ** 8)
    scale = np.where(r > 1e-8, theta_d / np.where(r > 1e-8, r, 1.0), 1.0)
    return fx * (a * scale) + cx, fy * (b * scale) + cy


def test_fisheye_against_distort_points():
    """1.6 million random coordinates: fx 300 .. 2000, pictures up to 4000 px, k of the order 0.05, 0.01, 0.005, 0.001.  The fixed
    coordinates may differ by one unit of 1/32 pixel (two roundings of values a few ulp apart that straddle a half), in at most 1
    in 10 000 coordinates.  Measured: 0 of 1 600 000 differ (the printed line)."""
    rng = np.random.default_rng(17)
    total = differing = 0
    worst = 0
    for _ in range(8):
        w, h = int(rng.integers(500, 4001)), int(rng.integers(500, 4001))
        fx = rng.uniform(300, 2000)
        lens8 = (fx, fx * rng.uniform(0.95, 1.05), w / 2.0 + rng.uniform(-30, 30), h / 2.0 + rng.uniform(-30, 30),
                 rng.normal(0, 0.05), rng.normal(0, 0.01), rng.normal(0, 0.005), rng.normal(0, 0.001))
        lens = lens8 + (0.0,) * 8 + (1.0,)
        ow, oh = 400, 250  # 100 000 points a lens, spread over the whole picture by the map
        M = np.array([[w / ow, 0.013, rng.uniform(-3, 3)], [-0.007, h / oh, rng.uniform(-3, 3)], [0.0, 0.0, 1.0]])
        X, Y = RM.fixed_coords(M, ow, oh, lens)
        U, V = RM.unrounded_coords(M, ow, oh, None)
        eu, ev = fisheye_points(lens8, U / 32.0, V / 32.0)
        for got, exp in ((X, eu), (Y, ev)):
            d = np.abs(got - np.rint(exp * 32.0).astype(np.int64))
            total += d.size
            differing += int((d != 0).sum())
            worst = max(worst, int(d.max()))
    print("fisheye against distortPoints: %d of %d coordinates differ, by at most %d unit(s)" % (differing, total, worst))
    assert total == 1600000
    assert worst <= 1
    assert differing * 10000 <= total


def test_model_0_against_the_closed_form():
    """OpenCV's x'' = x' num / den + tangential + prism terms, in float64, against the rule's displacement form, before rounding,
    for |a|, |b| <= 2: within 1e-9 of a 1/32-pixel unit.  This checks the algebra, not the last bits.  The lenses are of a real
    calibration's size -- fx 300 .. 2000, a radial factor that stays of order 1 out to r2 = 8 and a denominator that stays above
    1/2 -- so that the coordinates stay below about 3e5 units, whose ulp is 6e-11: both forms are a few such roundings from the
    exact value.  Measured: 8.7e-11 (the printed line)."""
    rng = np.random.default_rng(23)
    worst = 0.0
    for _ in range(40):
        fx, fy = rng.uniform(300, 2000, 2)
        cx, cy = rng.uniform(200, 2000, 2)
        k1, k2, k3 = rng.uniform(-1, 1) * 0.05, rng.uniform(-1, 1) * 0.005, rng.uniform(-1, 1) * 0.0005
        k4, k5, k6 = rng.uniform(0, 1) * 0.05, rng.uniform(0, 1) * 0.005, rng.uniform(0, 1) * 0.0005  # (den >= 1)
        p1, p2 = rng.uniform(-1, 1, 2) * 0.002
        s1, s2, s3, s4 = rng.uniform(-1, 1, 4) * np.array([0.002, 0.0002, 0.002, 0.0002])
        lens = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, 0.0)
        n = 101  # the grid a, b = -2 .. 2 as the ideal picture of an n x n output
        M = np.array([[4.0 * fx / (n - 1), 0.0, cx - 2.0 * fx], [0.0, 4.0 * fy / (n - 1), cy - 2.0 * fy], [0.0, 0.0, 1.0]])
        U, V = RM.unrounded_coords(M, n, n, lens)
        u, v = RM.unrounded_coords(M, n, n, None)
        a, b = (u / 32.0 - cx) / fx, (v / 32.0 - cy) / fy
        assert np.abs(a).max() <= 2.0 + 1e-12 and np.abs(a).max() > 1.99 and np.abs(b).max() > 1.99
        r2 = a * a + b * b
        factor = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        xd = a * factor + 2 * p1 * a * b + p2 * (r2 + 2 * a * a) + s1 * r2 + s2 * r2 ** 2
        yd = b * factor + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b + s3 * r2 + s4 * r2 ** 2
        worst = max(worst, np.abs(U - 32.0 * (fx * xd + cx)).max(), np.abs(V - 32.0 * (fy * yd + cy)).max())
    print("model 0 against the closed form: largest difference %.3e of a 1/32-pixel unit" % worst)
    assert worst <= 1e-9


CXX_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "librectify_amd.h"
// stdin: seventeen lens entries, then pairs u v, all as hex doubles; prints each result's two doubles and lr_lens_atan(|u|) as
// their 64 bits in hex
int main() {
    double lens[17], u, v, ud, vd;
    for (int i = 0; i < 17; ++i)
        if (std::scanf("%la", &lens[i]) != 1) return 99;
    while (std::scanf("%la %la", &u, &v) == 2) {
        lr_lens_distort_model(lens, u, v, &ud, &vd);
        const double at = lr_lens_atan(u < 0 ? -u : u);
        unsigned long long bu, bv, ba;
        std::memcpy(&bu, &ud, 8);
        std::memcpy(&bv, &vd, 8);
        std::memcpy(&ba, &at, 8);
        std::printf("%016llx %016llx %016llx\n", bu, bv, ba);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def lens_exe(tmp_path_factory):
    """the header's inlines in a program of its own, without contraction like the library itself"""
    d = tmp_path_factory.mktemp("lens_model")
    src, exe = str(d / "lens.cpp"), str(d / "lens")
    with open(src, "w") as f:
        f.write(CXX_PROGRAM)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", src, "-I", os.path.join(ROOT, "include"), "-o", exe])
    return exe


LENSES = [
    (100.0, 100.0, 79.5, 59.5, -0.2, 0.05, 0.002, -0.001, 0.01, 0.03, -0.004, 0.0005, 0.001, -0.0002, 0.0007, 0.0001, 0.0),
    (812.25, 807.5, 640.3, 355.9, 0.11, -0.27, -0.0013, 0.0021, 0.09, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),  # (fits the nine)
    (31.0, 29.0, 16.0, 12.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),  # (a denominator that crosses 0)
    (50.0, 60.0, 3.0, -2.0) + (-0.0, 0.0) * 6 + (0.0,),  # (no lens)
    (420.0, 415.0, 319.5, 239.5, 0.05, -0.01, 0.005, -0.001) + (0.0,) * 8 + (1.0,),
    (60.0, 60.0, 32.0, 24.0) + (0.0,) * 12 + (1.0,),  # (the pure equidistant lens)
    (0.5, 0.5, 10.0, 10.0, 0.0, 0.0, 0.0, 1e300) + (0.0,) * 8 + (1.0,),
]


def test_header_inlines_and_python_twins_agree(L, lens_exe):
    rng = np.random.default_rng(5)
    for k, lens in enumerate(LENSES):
        pts = np.concatenate([rng.uniform(-200, 1500, (280, 2)), rng.standard_normal((13, 2)) * 1e6, 10.0 ** rng.uniform(-12, 3, (100, 2)),
                              np.array([[0.0, 0.0], [-0.0, 5.0], [lens[2], lens[3]], [1e308, 1.0], [np.inf, 2.0], [1.0, 1.0], [0.125, 0.0]])])
        text = " ".join(float(v).hex() for v in lens) + "\n" + "\n".join("%s %s" % (float(u).hex(), float(v).hex()) for u, v in pts) + "\n"
        out = subprocess.run([lens_exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        got = np.array([int(v, 16) for v in out], np.uint64).reshape(-1, 3)
        exp = np.concatenate([L.lens_distort(L.LensModel(*lens), pts), L.lens_atan(np.abs(pts[:, 0]))[:, None]], axis=1)
        assert got.shape == exp.shape == (400, 3)
        nan = np.isnan(exp)  # (a NaN is a NaN where the twin has one: its sign and payload are the compiler's)
        assert np.array_equal(np.isnan(got.view(np.float64)), nan), k
        assert np.array_equal(got[~nan], exp.view(np.uint64)[~nan]), k  # (bits: infinities and the sign of zero included)
    # ... and the twin is the second source's rule before its rounding: rint(32 * distort) are the fixed coordinates
    grid = np.stack(np.meshgrid(np.arange(160.0), np.arange(120.0)), axis=-1)
    for lens in (LENSES[0], LENSES[4]):
        X, Y = RM.fixed_coords(np.eye(3), 160, 120, lens)
        d = L.lens_distort(L.LensModel(*lens), grid)
        assert np.array_equal(np.rint(d[..., 0] * 32.0).astype(np.int64), X) and np.array_equal(np.rint(d[..., 1] * 32.0).astype(np.int64), Y)
    # a nine-entry tuple still goes the nine-entry way
    assert np.array_equal(L.lens_distort(L.Lens(*LENSES[1][:9]), grid), L.lens_distort(LENSES[1][:9], grid))


def test_a_fisheye_moves_the_coordinates_towards_the_centre():
    lens = (30.0, 30.0, 11.0, 8.0) + (0.0,) * 12 + (1.0,)
    X, Y = RM.fixed_coords(np.eye(3), 23, 17, lens)
    X0, Y0 = R.fixed_coords(np.eye(3), 23, 17)
    assert X[8, 11] == X0[8, 11] and Y[8, 11] == Y0[8, 11]  # the centre stays (r == 0: sc = 1)
    assert X[0, 0] > X0[0, 0] and Y[0, 0] > Y0[0, 0] and X[16, 22] < X0[16, 22] and Y[16, 22] < Y0[16, 22]  # atan(r) < r


# ---- the table builders ----

def test_table_row_lengths_and_bits(L):
    Ms = np.stack([np.eye(3)] * 3)
    sizes = [(5, 4), (7, 3), (2, 2)]
    sources = [(9, 8, 0, 9), (6, 5, 72, 6), (4, 4, 102, 4)]
    nine = L.Lens(10.0, 11.0, 4.0, 3.5, -0.1, 0.02, 0.001, -0.002, 0.003)
    full = L.LensModel(10.0, 11.0, 4.0, 3.5, -0.1, 0.02, 0.001, -0.002, 0.003, 0.01, 0.02, 0.03, 0.001, 0.002, 0.003, 0.004)
    fish = L.LensModel.fisheye(20.0, 21.0, 2.0, 2.5, 0.05, 0.01, 0.005, 0.001)
    assert L.WARP_LENS_MODEL == 0x800000 and (L.LENS_RATIONAL, L.LENS_FISHEYE) == (0, 1)
    assert tuple(L.LensModel(1, 2, 3, 4, 5, 6, 7, 8, 9)) == (1, 2, 3, 4, 5, 6, 7, 8, 9) + (0,) * 8 and full.model == 0
    assert tuple(fish) == (20.0, 21.0, 2.0, 2.5, 0.05, 0.01, 0.005, 0.001) + (0.0,) * 8 + (1,)
    assert L.Lens._fields == ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")  # (Lens is what it was)
    for area, more in ((None, 0), (2, 1)):
        for lens in (full, fish, [nine, None, fish]):
            t = L.warp_table(Ms, sizes, 1, align=1, lens=lens, area=area)[0]
            assert t.shape == (3, 30 + more) and np.array_equal(t[:, :13], L.warp_table(Ms, sizes, 1, align=1)[0])
            t = L.warp_table(Ms, sizes, 1, border="reflect", lens=lens, area=area)[0]
            assert t.shape == (3, 31 + more) and (t[:, 13] == 2).all()
            t = L.ragged_table(Ms, sizes, sources, 1, lens=lens, area=area)[0]
            assert t.shape == (3, 35 + more) and np.array_equal(t[:, :18], L.ragged_table(Ms, sizes, sources, 1)[0])
            t = L.ragged_table(Ms, sizes, sources, 1, border=("constant", 7), lens=lens, area=area)[0]
            assert t.shape == (3, 35 + more) and (t[:, 17] == 56).all()
            if area:
                assert (t[:, -1] == 2).all()
            bits, row = L._border_bit_and_map(None, L.PIX_U8, np.eye(3), "t", lens if not isinstance(lens, list) else fish, area)
            assert bits == L.WARP_LENS | L.WARP_LENS_MODEL | (L.WARP_AREA if area else 0) and row.shape == (26 + more,)
            bits, row = L._border_bit_and_map("replicate", L.PIX_U8, np.eye(3), "t", full, area)
            assert bits & L.WARP_BORDER and row.shape == (27 + more,) and row[9] == 1 and tuple(row[10:27]) == tuple(full)
    t = L.ragged_table(Ms, sizes, sources, 1, lens=[nine, None, fish])[0][:, 18:]
    assert tuple(t[0]) == tuple(nine) + (0.0,) * 8 and tuple(t[2]) == tuple(fish)  # (a Lens fills the first nine of a model-0 row)
    assert (t[1, 4:] == 0).all() and t[1, 0] > 0 and t[1, 1] > 0
    # Lens alone: today's tables, byte for byte, and today's bit
    for lens in (nine, [nine, None, nine._replace(k1=0.3)]):
        t = L.warp_table(Ms, sizes, 3, border="reflect101", lens=lens, area=3)[0]
        assert t.shape == (3, 24) and t[:, 14:23].tobytes() == np.array([tuple(v) if v else (1, 1, 0, 0, 0, 0, 0, 0, 0) for v in (lens if isinstance(lens, list) else [lens] * 3)], np.float64).tobytes()
        assert L.ragged_table(Ms, sizes, sources, 1, lens=lens)[0].shape == (3, 27)
    assert L._border_bit_and_map(None, L.PIX_U8, np.eye(3), "t", nine)[0] == L.WARP_LENS


def test_table_refusals_name_the_frame(L):
    Ms = np.stack([np.eye(3)] * 3)
    sizes = [(5, 4), (7, 3), (2, 2)]
    sources = [(9, 8, 0, 9), (6, 5, 72, 6), (4, 4, 102, 4)]
    good = L.LensModel(10.0, 11.0, 4.0, 3.5, -0.1, k5=0.02, s3=0.001)
    fish = L.LensModel.fisheye(20.0, 21.0, 2.0, 2.5, 0.05)
    bads = [good._replace(fx=0.0), good._replace(fy=-3.0), good._replace(k6=float("nan")), good._replace(s4=float("inf")), good._replace(model=float("nan")),
            good._replace(model=2), good._replace(model=-1), good._replace(model=0.5), fish._replace(k3=0.1), fish._replace(s4=-1e-300), fish._replace(fx=-1.0)]
    for bad in bads:
        with pytest.raises(ValueError, match=r"warp_table.*frame 0"):
            L.warp_table(Ms, sizes, 1, lens=bad)
        with pytest.raises(ValueError, match=r"ragged_table.*frame 1"):
            L.ragged_table(Ms, sizes, sources, 1, lens=[good, bad, None])
        with pytest.raises(ValueError, match=r"ragged_table.*frame 2"):
            L.ragged_table(Ms, sizes, sources, 1, lens=[L.Lens(5.0, 5.0, 1.0, 1.0), None, bad])
    with pytest.raises(ValueError, match="as many lenses as frames"):
        L.warp_table(Ms, sizes, 1, lens=[good, fish])
    # lens_scale_map and its refusals
    np.testing.assert_array_equal(L.lens_scale_map(fish, 0.5), [[2.0, 0.0, -2.0], [0.0, 2.0, -2.5], [0.0, 0.0, 1.0]])
    np.testing.assert_array_equal(L.lens_scale_map(L.Lens(3.0, 3.0, 7.0, 9.0), 1), np.eye(3))
    for s in (0, -1.0, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="lens_scale"):
            L.lens_scale_map(fish, s)
