"""LR_WARP_LENS without a GPU: the second source against the references it extends (zero coefficients), the header's
lr_lens_distort, compiled on its own, against its Python twin, an independent geometric check of the rule (a known picture
distorted by a Newton inverse written here and undistorted by the reference), and the table builders."""
import math
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_border_ref as RB
import numpy_warp_cubic_ref as RC
import numpy_warp_lens_ref as RL
import numpy_warp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# maps of the existing references' tests (test_warp_border_cpu.py, test_gpu_warp*.py): an affine with a little perspective, the
# identity, one whose W0 = 0 line crosses the output, and a rotation with scale
MAPS = [
    np.array([[0.9, -0.2, -3.0], [0.15, 1.1, -4.5], [0.0004, -0.0007, 1.0]]),
    np.eye(3),
    np.array([[1.0, 0.1, 2.0], [0.05, 1.0, -1.0], [0.05, 0.0, -1.0]]),
    np.array([[0.7 * math.cos(math.pi / 6), -0.7 * math.sin(math.pi / 6), 5.0], [0.7 * math.sin(math.pi / 6), 0.7 * math.cos(math.pi / 6), -3.0], [0, 0, 1.0]]),
]


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L

    return L


def source(fmt, w, h, seed):
    rng = np.random.default_rng(seed)
    if fmt == 2:
        return rng.standard_normal((h, w)).astype(np.float32)
    return rng.integers(0, 256, (h, w, 3) if fmt == 1 else (h, w), dtype=np.uint8)


@pytest.mark.parametrize("zeros", [(0.0,) * 5, (-0.0, 0.0, -0.0, 0.0, -0.0)])
def test_zero_coefficients_are_the_existing_references(zeros):
    lens = (31.5, 27.25, 11.0, 8.5) + zeros
    for M in MAPS:
        X, Y = RL.fixed_coords(M, 37, 29, lens)
        X0, Y0 = R.fixed_coords(M, 37, 29)
        assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
        for fmt in (0, 1, 2):
            src = source(fmt, 23, 17, fmt)
            for cubic, old in ((False, R.warp), (True, RC.warp)):
                got = RL.warp(src, M, 37, 29, lens, cubic=cubic)
                exp = old(src, M, 37, 29)
                assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), (fmt, cubic)
                for mode, value in ((RB.CONSTANT, 200), (RB.REPLICATE, 0), (RB.REFLECT, 0), (RB.REFLECT_101, 0)):
                    v = (value,) * 3 if fmt == 1 else value
                    got = RL.warp(src, M, 37, 29, lens, mode, v, cubic)
                    exp = RB.warp(src, M, 37, 29, mode, v, cubic)
                    assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), (fmt, cubic, mode)
    assert RB.fixed_coords is R.fixed_coords  # (the bordered reference is left as it was)


def test_a_lens_moves_the_coordinates():
    lens = (30.0, 30.0, 11.0, 8.0, -0.3, 0.1, 0.0, 0.0, 0.0)
    X, Y = RL.fixed_coords(np.eye(3), 23, 17, lens)
    X0, Y0 = R.fixed_coords(np.eye(3), 23, 17)
    assert X[8, 11] == X0[8, 11] and Y[8, 11] == Y0[8, 11]  # the centre stays
    assert X[0, 0] > X0[0, 0] and Y[0, 0] > Y0[0, 0]  # barrel: a corner of the ideal picture is shown nearer the centre
    assert X[16, 22] < X0[16, 22] and Y[16, 22] < Y0[16, 22]


CXX_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "librectify_amd.h"
// stdin: nine lens entries, then pairs u v, all as hex doubles; prints each result's two doubles as their 64 bits in hex
int main() {
    double lens[9], u, v, ud, vd;
    for (int i = 0; i < 9; ++i)
        if (std::scanf("%la", &lens[i]) != 1) return 99;
    while (std::scanf("%la %la", &u, &v) == 2) {
        lr_lens_distort(lens, u, v, &ud, &vd);
        unsigned long long bu, bv;
        std::memcpy(&bu, &ud, 8);
        std::memcpy(&bv, &vd, 8);
        std::printf("%016llx %016llx\n", bu, bv);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def lens_exe(tmp_path_factory):
    """the header's inline in a program of its own, without contraction like the library itself"""
    d = tmp_path_factory.mktemp("lens")
    src, exe = str(d / "lens.cpp"), str(d / "lens")
    with open(src, "w") as f:
        f.write(CXX_PROGRAM)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", src, "-I", os.path.join(ROOT, "include"), "-o", exe])
    return exe


LENSES = [
    (100.0, 100.0, 79.5, 59.5, -0.2, 0.05, 0.002, -0.001, 0.0),
    (812.25, 807.5, 640.3, 355.9, 0.11, -0.27, -0.0013, 0.0021, 0.09),
    (31.0, 29.0, 16.0, 12.0, 50.0, 0.0, 0.0, 0.0, 0.0),
    (31.0, 29.0, 16.0, 12.0, 0.0, 0.0, 0.0, 0.0, 1e300),
    (50.0, 60.0, 3.0, -2.0, 0.0, 0.0, 0.0, 0.0, 0.0),
]


def test_header_inline_and_python_twin_agree(L, lens_exe):
    rng = np.random.default_rng(5)
    for k, lens in enumerate(LENSES):
        pts = np.concatenate([rng.uniform(-200, 1500, (180, 2)), rng.standard_normal((15, 2)) * 1e6,
                              np.array([[0.0, 0.0], [-0.0, 5.0], [lens[2], lens[3]], [1e308, 1.0], [np.inf, 2.0]])])
        text = " ".join(float(v).hex() for v in lens) + "\n" + "\n".join("%s %s" % (float(u).hex(), float(v).hex()) for u, v in pts) + "\n"
        out = subprocess.run([lens_exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        got = np.array([int(v, 16) for v in out], np.uint64).reshape(-1, 2)
        exp = L.lens_distort(L.Lens(*lens), pts)
        assert got.shape == exp.shape == (200, 2)
        nan = np.isnan(exp)  # (a NaN is a NaN where the twin has one: its sign and payload are the compiler's)
        assert np.array_equal(np.isnan(got.view(np.float64)), nan)
        assert np.array_equal(got[~nan], exp.view(np.uint64)[~nan]), k  # (bits: infinities and the sign of zero included)
    # ... and the twin is the reference's rule before its rounding: rint(32 * distort) are the fixed coordinates
    lens = LENSES[0]
    X, Y = RL.fixed_coords(np.eye(3), 160, 120, lens)
    grid = np.stack(np.meshgrid(np.arange(160.0), np.arange(120.0)), axis=-1)
    d = L.lens_distort(L.Lens(*lens), grid)
    assert np.array_equal(np.rint(d[..., 0] * 32.0).astype(np.int64), X) and np.array_equal(np.rint(d[..., 1] * 32.0).astype(np.int64), Y)


# ---- an independent geometric check ----

W, H = 160, 120
OMEGA = 2.0 * math.pi / 64.0


def picture(u, v):
    return 127.5 + 100.0 * np.sin(OMEGA * u) * np.sin(OMEGA * v)


def forward(lens, u, v):
    """the lens model as the text books write it (normalised point, radial factor, tangential terms): not the rule's order of
    operations, and shared with nothing"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = lens
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return cx + fx * xd, cy + fy * yd


def newton_inverse(lens, pu, pv):
    """the ideal points whose images under `forward` are the stored pixels (pu, pv): Newton's iteration with a Jacobian from
    central differences, started at the pixels themselves"""
    u, v = np.array(pu, np.float64), np.array(pv, np.float64)
    e = 1e-4
    for _ in range(40):
        fu, fv = forward(lens, u, v)
        ru, rv = fu - pu, fv - pv
        a, c = [(p - m) / (2 * e) for p, m in zip(forward(lens, u + e, v), forward(lens, u - e, v))]
        b, d = [(p - m) / (2 * e) for p, m in zip(forward(lens, u, v + e), forward(lens, u, v - e))]
        det = a * d - b * c
        u, v = u - (d * ru - b * rv) / det, v - (a * rv - c * ru) / det
    fu, fv = forward(lens, u, v)
    assert np.abs(fu - pu).max() < 1e-9 and np.abs(fv - pv).max() < 1e-9
    return u, v


def inverse_derivatives(lens):
    """(m, kappa): the largest spectral norm of the inverse map's Jacobian and the largest length of a pure second derivative
    of it along an axis, over the stored frame, by central differences of step 1/2 on the pixel grid (2 % added for what lies
    between the samples)"""
    if not RL.has_lens(lens):
        return 1.0, 0.0
    pv, pu = np.mgrid[0:H, 0:W].astype(np.float64)
    s = 0.5
    c = np.stack(newton_inverse(lens, pu, pv))
    xp, xm = np.stack(newton_inverse(lens, pu + s, pv)), np.stack(newton_inverse(lens, pu - s, pv))
    yp, ym = np.stack(newton_inverse(lens, pu, pv + s)), np.stack(newton_inverse(lens, pu, pv - s))
    J = np.stack([(xp - xm) / (2 * s), (yp - ym) / (2 * s)], axis=-1)  # (2, H, W, 2): columns are the axes' derivatives
    m = np.linalg.norm(np.moveaxis(J, 0, 2), ord=2, axis=(2, 3)).max()
    kappa = max(np.sqrt((((p - 2 * c + q) / (s * s)) ** 2).sum(axis=0)).max() for p, q in ((xp, xm), (yp, ym)))
    return 1.02 * m, 1.02 * kappa


@pytest.mark.parametrize("lens", [(100.0, 100.0, 79.5, 59.5, -0.2, 0.05, 0.002, -0.001, 0.0), (100.0, 100.0, 79.5, 59.5, 0.0, 0.0, 0.0, 0.0, 0.0)],
                         ids=["lens", "zeros"])
def test_undistorting_a_known_picture(lens):
    """The stored frame is D(p) = round(f(inv(p))), inv the Newton inverse of the lens; the reference's undistorted picture O
    is compared with round(f) where all four taps are inside.

    The bound.  g = f o inv is what the stored frame samples on the unit grid.  With m the largest norm of inv's Jacobian and
    kappa the largest length of inv's second derivative along an axis (both measured above from the Newton inverse: properties
    of the lens, not of the code under test), w = 2 pi / 64:
      |f''| : the Hessian of f is 100 w^2 [[-ss, cc], [cc, -ss]] with eigenvalues 100 w^2 (-ss +- cc), at most 100 w^2;
      |grad f| <= 100 w;
      |g_xx|, |g_yy| <= 100 w^2 m^2 + 100 w kappa                 (chain rule)
      bilinear interpolation on a unit cell: (1/8) (|g_xx| + |g_yy|) = (1/4) (100 w^2 m^2 + 100 w kappa)
      the stored samples are rounded: a convex blend of errors of at most 1/2 is at most                       1/2
      the coordinates are rounded to 1/32, so off by at most 1/64 per axis: (1/64) (|g_x| + |g_y|) <= (sqrt 2 / 64) m 100 w
    Their sum e bounds |B - f|, B being the exact blend.  O = round(B) (the rule's (s + 512) >> 10) and the comparison is with
    round(f): two integers whose unrounded values differ by at most e differ by less than e + 1, so by at most floor(e + 1)
    when e is no integer.  With the lens e is about 1.5 (bound 2 levels), without it 0.96 (bound 1 level)."""
    m, kappa = inverse_derivatives(lens)
    e = 0.25 * (100.0 * OMEGA ** 2 * m * m + 100.0 * OMEGA * kappa) + 0.5 + math.sqrt(2.0) / 64.0 * m * 100.0 * OMEGA
    bound = math.floor(e + 1.0)
    assert bound == (2 if RL.has_lens(lens) else 1), (m, kappa, e)

    pv, pu = np.mgrid[0:H, 0:W].astype(np.float64)
    iu, iv = newton_inverse(lens, pu, pv) if RL.has_lens(lens) else (pu, pv)
    stored = np.rint(picture(iu, iv)).astype(np.uint8)
    got = RL.warp(stored, np.eye(3), W, H, lens).astype(np.int64)
    X, Y = RL.fixed_coords(np.eye(3), W, H, lens)
    inside = ((X >> 5) >= 0) & ((X >> 5) + 1 < W) & ((Y >> 5) >= 0) & ((Y >> 5) + 1 < H)
    assert inside.mean() > 0.9
    exp = np.rint(picture(pu, pv)).astype(np.int64)
    diff = np.abs(got - exp)[inside]
    print("lens %r: m %.4f kappa %.5f e %.4f bound %d, largest difference %d, mean %.4f" % (lens[4:], m, kappa, e, bound, diff.max(), diff.mean()))
    assert diff.max() <= bound
    if RL.has_lens(lens):  # the stored frame itself is not the picture: the lens moved it by several pixels
        assert np.abs(stored.astype(np.int64) - exp).max() > 40


# ---- the table builders ----

def test_table_row_lengths(L):
    Ms = np.stack([np.eye(3)] * 3)
    sizes = [(5, 4), (7, 3), (2, 2)]
    sources = [(9, 8, 0, 9), (6, 5, 72, 6), (4, 4, 102, 4)]
    lens = L.Lens(10.0, 11.0, 4.0, 3.5, -0.1, 0.02, 0.001, -0.002, 0.003)
    assert L.WARP_LENS == 0x100000
    assert tuple(L.Lens(1, 2, 3, 4)) == (1, 2, 3, 4, 0, 0, 0, 0, 0)
    t, total = L.warp_table(Ms, sizes, 1, align=1, lens=lens)
    assert t.shape == (3, 22) and np.array_equal(t[:, :13], L.warp_table(Ms, sizes, 1, align=1)[0]) and total == 20 + 21 + 4
    assert (t[:, 13:] == np.array(lens)).all()
    t = L.warp_table(Ms, sizes, 1, border="reflect", lens=lens)[0]
    assert t.shape == (3, 23) and (t[:, 13] == 2).all() and (t[:, 14:] == np.array(lens)).all()
    t = L.ragged_table(Ms, sizes, sources, 1, lens=lens)[0]
    assert t.shape == (3, 27) and np.array_equal(t[:, :18], L.ragged_table(Ms, sizes, sources, 1)[0]) and (t[:, 18:] == np.array(lens)).all()
    t = L.ragged_table(Ms, sizes, sources, 1, border=("constant", 7), lens=lens)[0]
    assert t.shape == (3, 27) and (t[:, 17] == 56).all()
    # the single-frame rows: 18 doubles, 19 with a border word
    bits, row = L._border_bit_and_map(None, L.PIX_U8, np.eye(3), "t", lens)
    assert bits == L.WARP_LENS and row.shape == (18,) and tuple(row[9:]) == tuple(lens)
    bits, row = L._border_bit_and_map("replicate", L.PIX_U8, np.eye(3), "t", lens)
    assert bits == L.WARP_LENS | L.WARP_BORDER and row.shape == (19,) and row[9] == 1 and tuple(row[10:]) == tuple(lens)
    assert L._border_bit_and_map(None, L.PIX_U8, np.eye(3), "t")[0] == 0


def test_table_lens_lists_and_refusals(L):
    Ms = np.stack([np.eye(3)] * 3)
    sizes = [(5, 4), (7, 3), (2, 2)]
    sources = [(9, 8, 0, 9), (6, 5, 72, 6), (4, 4, 102, 4)]
    a, b = L.Lens(10.0, 11.0, 4.0, 3.5, k1=-0.1), L.Lens(20.0, 21.0, 2.0, 2.5, p2=0.01)
    for t in (L.warp_table(Ms, sizes, 3, lens=[a, None, b])[0][:, 13:], L.ragged_table(Ms, sizes, sources, 1, lens=[a, None, b])[0][:, 18:]):
        assert tuple(t[0]) == tuple(a) and tuple(t[2]) == tuple(b)
        assert (t[1, 4:] == 0).all() and t[1, 0] > 0 and t[1, 1] > 0  # None: zero coefficients (and a focal length the library takes)
    for bad in (a._replace(fx=0.0), a._replace(fy=-3.0), a._replace(k2=float("nan")), a._replace(cx=float("inf")), a._replace(p1=-float("inf"))):
        with pytest.raises(ValueError, match="warp_table"):
            L.warp_table(Ms, sizes, 1, lens=bad)
        with pytest.raises(ValueError, match="ragged_table"):
            L.ragged_table(Ms, sizes, sources, 1, lens=[a, bad, None])
    with pytest.raises(ValueError, match="as many lenses as frames"):
        L.warp_table(Ms, sizes, 1, lens=[a, b])
    with pytest.raises(ValueError):
        L.warp_table(Ms, sizes, 1, lens="barrel")
