"""A SECOND, independent source for the opt-in estimators of kernels_ransac.hip -- the diamond-space accumulator and its
peeling (cht.h:13-24 with the published mapping of Dubska & Herout 2013, rasterised as cht.cpp:163-197), the Hough weights
(line_pencil.cpp:35-86) -- in float64 NumPy and Python integers, written from the reference's text and the paper, not from
the oracle or the kernels.  Like numpy_grouping_ref.py, whose building blocks it uses (normalised_f32, Model with its
bounds dh, line_errors / decide, refit, peel_chain's verdicts), it does not reproduce fp32 bits: every fp32 decision is
SURE or AMBIGUOUS, an accumulator cell is an integer interval [lo, hi], and a result is checked for lying inside what the
intervals allow.  Test infrastructure only.

The bands (u = 2^-24; G = 1.01 absorbs the second-order terms, as in numpy_grouping_ref.py)
--------------------------------------------------------------------------------------------
DIAMOND SPACE.  A line h = (a, b, c), |h| = 1, with the componentwise bound dh of Model, maps to the polyline
    P0 = (al a / d1, -al c / d1)   P1 = (b / d2, 0)   P2 = (0, b / d3)   P3 = -P0
    al = sgn(a b), be = sgn(b c), ga = sgn(a c), sgn(0) = +1;   d1 = c + ga a, d2 = c + be b, d3 = a + al b.
Signs.  A component that is exactly zero (value 0, bound 0: a horizontal or vertical segment, a line through the
normalisation centre -- the differences and the products that make it are then exact zeros in fp32 too) makes the product
+-0, whose sign is +1.  Two components that are surely not zero give the product of their signs (no underflow: a
component of a unit vector made of fp32 coordinates is either 0 or far above 2^-75).  A component within its bound of 0
without being exactly 0 leaves a sign open, and the line is AMBIGUOUS AS A WHOLE: it may vote for anything.
Denominators.  |d1| = |c| + |a| and so on (the sign in front of the second term makes the terms agree), so a denominator
is zero only if both of its terms are exactly zero; then the corner does not exist and the two segments (one for d2, d3)
that end in it are dropped.  Otherwise dd = dh_1 + dh_2 + u |d| and the quotient q = n / d is off by at most
(dn + |q| dd) / (|d| - dd) + u (|q| + that); |d| <= 2 dd makes the line ambiguous as a whole.  Where the numerator is
exactly zero the quotient is exactly 0, and where the other term of the denominator is exactly zero the quotient is x / x
= +-1 exactly, whatever the error of x.  |q| <= 1 also in fp32 (fl(|c| + |a|) >= |a|, and division is monotone), so the
range test of the rasteriser never fires and is not modelled.
Corner cells.  pos = (q + 1) / 2 (d - 1) is exact where q is exactly 0 or +-1 (a half-integer at most: roundf takes a half
away from zero, upwards here).  Else dpos = (d - 1) / 2 (dq + u |q + 1|) + u pos, and the cell is round(pos) if pos is further than
dpos from a half, else one of two.  A segment with an open corner is voted for as a whole: every cell that one of the
(at most 16) combinations of end cells reaches may get its votes, none surely does, and its number of votes is between
the fewest and the most steps of the combinations.
Steps.  With integer end cells, S = max(|x1 - x0|, |y1 - y0|), steps = S + 1 (integers below 2^24: exact), and vote j lands
in round(x0 + j sx), sx = fl((x1 - x0) / S).  The exact position is the rational x0 + j D / S, computed here in integers.
Along the longer axis |D| = S, sx = +-1 and everything is an integer.  Along the shorter one:
  * S a power of two: sx = D / S is exact, j sx < 2^14 is exact, and x0 + j sx is a multiple of 1/128 below 128: exact.  A half
    is a half in fp32 as well and goes up (positions are not negative): SURE.
  * else, if the rational position is a half (2 (j D mod S) = S), the fp32 value is a half or a neighbour of it: AMBIGUOUS
    between the two cells.
  * else the rational position is at least 1 / (2 S) >= 1 / 254 from a half (d <= 128: S <= 127), and the fp32 position is
    off by at most: sx (1 + e1), j sx (1 + e1)(1 + e2): j |sx| 2.01u <= 2.01u |D| <= 256u; the sum: u 128; together
    384u = 2.3e-5.  (The coarser count (j + 2) u extent <= 130 x 127 u = 9.9e-4 does as well.)  Both are below
    1 / 254 = 3.9e-3: SURE.
A segment of no length has h = 0 / 0: NaN fails every comparison of the range test, nothing is voted.
Votes.  floor(len 65536 + 0.5) of the fp32 length.  len carries 3u relative (Model), the scaling is exact, the sum one more
rounding: dv = 3u v + u (v + 0.5).  If v + 0.5 is within dv of an integer the vote is one of two neighbouring integers.
Intervals.  lo[cell] = sum of (sure votes) x (lower vote), hi[cell] = sum of (sure + possible votes) x (upper vote); the total
is bracketed by the numbers of votes (an ambiguous vote counts once, not in both of its cells).  The AMBIGUOUS SHARE of a
case is (weight of the votes whose cell is open + the one-unit slack of open lengths) / (upper total); the cases keep it
below AMBIGUITY_CAP.
Cell to point (the inverse mapping of the paper): cell (ix, iy) -> u = 2 ix / (d - 1) - 1, v = 2 iy / (d - 1) - 1, point
(v, |u| + |v| - 1, u).  In fp32: a quotient, an exact doubling, a difference: 3u absolute on u and v, 8u on the middle
component (taken for all three).  De-normalised (normalize_point, geometry.cpp:232-238, then scale x + centre): u = 0
exactly (odd d, middle column) is an ideal point and stays as it is; else |u| >= 1 / (d - 1) and X = v / u is off by
(3u + 3u |X|) (d - 1) + u |X|, Y likewise with 8u for its numerator, and the image coordinate by scale times that plus 2u (|scale X| +
|centre|).  Neighbouring cells differ by a factor 1 + 1 / (d - 1) at least in X or Y, four orders of magnitude more.

HOUGH WEIGHTS (line_pencil.cpp:35-86): see the second half of this file.
"""
import itertools

import numpy as np

import numpy_grouping_ref as N
from numpy_grouping_ref import G, U

AMBIGUITY_CAP = 0.05  # of the total votes of a case, by weight


class _Open(Exception):
    """a decision on which the whole line hangs is within its bound"""


# ---- diamond space: one line's votes ---------------------------------------------------------------------------------------
def _sign_of_product(x, dx, y, dy):
    if (x == 0 and dx == 0) or (y == 0 and dy == 0):
        return 1.0
    if abs(x) <= dx or abs(y) <= dy:
        raise _Open()
    return 1.0 if (x > 0) == (y > 0) else -1.0


def _quotient(num, dnum, den, dden):
    if abs(den) <= 2 * dden:
        raise _Open()
    q = num / den
    e = (dnum + abs(q) * dden) / (abs(den) - dden)
    return q, G * (e + U * (abs(q) + e))


def polyline(h, dh):
    """-> [P0, P1, P2, P3], each None (its denominator is surely zero) or ((x, dx), (y, dy)); raises _Open"""
    (a, b, c), (da, db, dc) = h, dh
    za, zb, zc = a == 0 and da == 0, b == 0 and db == 0, c == 0 and dc == 0
    al, be, ga = _sign_of_product(a, da, b, db), _sign_of_product(b, db, c, dc), _sign_of_product(a, da, c, dc)
    d1, d2, d3 = c + ga * a, c + be * b, a + al * b
    dd1, dd2, dd3 = dc + da + U * abs(d1), dc + db + U * abs(d2), da + db + U * abs(d3)
    if za and zc:
        p0 = None
    else:
        x = (0.0, 0.0) if za else (al, 0.0) if zc else _quotient(al * a, da, d1, dd1)
        y = (0.0, 0.0) if zc else (-al, 0.0) if za else _quotient(-al * c, dc, d1, dd1)
        p0 = (x, y)
    p1 = None if zb and zc else ((0.0, 0.0) if zb else (1.0, 0.0) if zc else _quotient(b, db, d2, dd2), (0.0, 0.0))
    p2 = None if za and zb else ((0.0, 0.0), (0.0, 0.0) if zb else (1.0, 0.0) if za else _quotient(b, db, d3, dd3))
    p3 = None if p0 is None else ((-p0[0][0], p0[0][1]), (-p0[1][0], p0[1][1]))
    return [p0, p1, p2, p3]


def _cells_of(q, dq, d):
    """the accumulator coordinate(s) of the polyline coordinate q +- dq"""
    sc = d - 1
    pos = (q + 1.0) * 0.5 * sc
    if dq == 0 and q in (0.0, 1.0, -1.0):
        return [int(np.floor(pos + 0.5))]
    dpos = G * (0.5 * sc * (dq + U * abs(q + 1.0)) + U * abs(pos))
    fl = int(np.floor(pos))
    if abs(pos - fl - 0.5) > dpos:
        return [int(np.floor(pos + 0.5))]
    return [fl, fl + 1]


def _axis(x0, D, S, j):
    """round(x0 + j D / S) for j = 0..S in exact arithmetic -> (cells, open: the other candidate is cell + 1)"""
    num = j * D
    q = num // S
    r = num - q * S
    pow2 = (S & (S - 1)) == 0
    half = 2 * r == S
    up = (2 * r > S) | (half & pow2)
    return x0 + q + up, half & (not pow2)


def rasterise(x0, y0, x1, y1, d):
    """accumulate_lines (cht.cpp:163-197) between integer end cells -> (sure cells, pairs of cells of the open votes)"""
    S = max(abs(x1 - x0), abs(y1 - y0))
    if S == 0:
        return np.array([y0 * d + x0], np.int64), np.zeros((0, 2), np.int64)
    j = np.arange(S + 1, dtype=np.int64)
    xs, ox = _axis(x0, x1 - x0, S, j)
    ys, oy = _axis(y0, y1 - y0, S, j)
    opened = ox | oy
    cells = ys * d + xs
    other = (ys + oy) * d + xs + ox
    return cells[~opened], np.stack([cells[opened], other[opened]], 1)


def vote_of(length):
    """floor(len 65536 + 0.5) of the fp32 length -> (lower, upper)"""
    v = length * 65536.0
    dv = G * (3 * U * v + U * (v + 0.5))
    t = v + 0.5
    k = int(np.floor(t))
    if t - k < dv:
        return k - 1, k
    if k + 1 - t < dv:
        return k, k + 1
    return k, k


def _sparse(a):
    at = np.nonzero(a)[0]
    return at, a[at]


def line_votes(h, dh, d):
    """one line -> dict(sure: (cells, votes surely cast there), maybe: (cells, votes possibly cast there on top), n_sure, t_lo, t_hi: the
    number of further votes, n_open: votes whose cell is open, steps: per segment its number of steps, None where the
    segment is dropped, -1 where it is open)"""
    cells = d * d
    sure, maybe = np.zeros(cells, np.int64), np.zeros(cells, np.int64)
    try:
        P = polyline(h, dh)
    except _Open:
        return dict(sure=_sparse(sure), maybe=_sparse(maybe + 3), n_sure=0, t_lo=0, t_hi=3 * d, n_open=3 * d, steps=[-1, -1, -1], whole=True)
    t_lo = t_hi = n_open = 0
    steps = []
    for s in range(3):
        if P[s] is None or P[s + 1] is None:
            steps.append(None)
            continue
        cand = [_cells_of(*P[s][0], d), _cells_of(*P[s][1], d), _cells_of(*P[s + 1][0], d), _cells_of(*P[s + 1][1], d)]
        combos = list(itertools.product(*cand))
        if len(combos) == 1:
            c, pairs = rasterise(*combos[0], d)
            np.add.at(sure, c, 1)
            np.add.at(maybe, pairs.reshape(-1), 1)
            t_lo += len(pairs)
            t_hi += len(pairs)
            n_open += len(pairs)
            steps.append(len(c) + len(pairs))
        else:  # an open corner: the segment as a whole may go any of these ways
            reach, counts = np.zeros(cells, np.int64), []
            for combo in combos:
                c, pairs = rasterise(*combo, d)
                one = np.zeros(cells, np.int64)
                np.add.at(one, c, 1)
                np.add.at(one, pairs.reshape(-1), 1)
                reach = np.maximum(reach, one)
                counts.append(len(c) + len(pairs))
            maybe += reach
            t_lo += min(counts)
            t_hi += max(counts)
            n_open += max(counts)
            steps.append(-1)
    return dict(sure=_sparse(sure), maybe=_sparse(maybe), n_sure=int(sure.sum()), t_lo=t_lo, t_hi=t_hi, n_open=n_open, steps=steps, whole=False)


class Diamond:
    """the votes of every line of a model in a d x d diamond space; lines with the same record are worked out once"""

    def __init__(self, M, d):
        self.M, self.d = M, d
        self.votes = {}
        for i in np.unique(M.canon):
            if M.length[i] == 0:  # a segment of no length: h is 0 / 0, and the rasteriser's range test lets no NaN pass
                none = (np.zeros(0, np.int64), np.zeros(0, np.int64))
                self.votes[int(i)] = dict(sure=none, maybe=none, n_sure=0, t_lo=0, t_hi=0, n_open=0, steps=[None, None, None], whole=False, weight=(0, 0))
                continue
            self.votes[int(i)] = dict(line_votes(M.h[i], M.dh[i], d), weight=vote_of(M.length[i]))

    def of(self, i):
        return self.votes[int(self.M.canon[i])]

    def intervals(self, idx=None):
        """the accumulator of the lines idx (default: all) -> dict(lo, hi: per cell; total_lo, total_hi: of the sum over
        cells; count_lo, count_hi: of the number of votes cast; open: the ambiguous weight; share)"""
        idx = np.arange(self.M.n) if idx is None else np.asarray(idx, np.int64)
        canon, mult = np.unique(self.M.canon[idx], return_counts=True)
        cells = self.d * self.d
        lo, hi = np.zeros(cells, np.int64), np.zeros(cells, np.int64)
        t_lo = t_hi = c_lo = c_hi = opened = 0
        for i, m in zip(canon.tolist(), mult.tolist()):
            V = self.votes[i]
            w_lo, w_hi = V["weight"]
            lo[V["sure"][0]] += V["sure"][1] * (w_lo * m)
            hi[V["sure"][0]] += V["sure"][1] * (w_hi * m)
            hi[V["maybe"][0]] += V["maybe"][1] * (w_hi * m)
            c_lo += m * (V["n_sure"] + V["t_lo"])
            c_hi += m * (V["n_sure"] + V["t_hi"])
            t_lo += m * (V["n_sure"] + V["t_lo"]) * w_lo
            t_hi += m * (V["n_sure"] + V["t_hi"]) * w_hi
            opened += m * (V["n_open"] * w_hi + V["n_sure"] * (w_hi - w_lo))
        return dict(lo=lo, hi=hi, total_lo=t_lo, total_hi=t_hi, count_lo=c_lo, count_hi=c_hi, open=opened, share=opened / t_hi if t_hi else 0.0, d=self.d)


def check_accumulator(name, acc, A):
    """acc: the d x d accumulator an implementation returned, row-major [y][x]; A: Diamond.intervals of the same lines"""
    got = [int(v) for v in np.asarray(acc).reshape(-1)]
    assert len(got) == len(A["lo"]), "[%s] accumulator: %d cells, not %d" % (name, len(got), len(A["lo"]))
    for c, v in enumerate(got):
        if not (A["lo"][c] <= v <= A["hi"][c]):
            raise AssertionError("[%s] cell interval: cell %d (x %d, y %d) holds %d, outside [%d, %d]" % (
                name, c, c % A["d"], c // A["d"], v, A["lo"][c], A["hi"][c]))
    total = sum(got)
    assert A["total_lo"] <= total <= A["total_hi"], "[%s] total: the cells sum to %d, outside [%d, %d]" % (name, total, A["total_lo"], A["total_hi"])


def check_peak(name, cell, A):
    """the strongest cell: the first maximum in row-major order, as far as the intervals say"""
    lo, hi = A["lo"], A["hi"]
    cell = int(cell)
    assert 0 <= cell < len(lo), "[%s] peak: cell %d of %d" % (name, cell, len(lo))
    best = int(lo.max())
    assert hi[cell] >= best, "[%s] peak beaten: cell %d holds at most %d, cell %d at least %d" % (name, cell, hi[cell], int(np.argmax(lo)), best)
    before = np.nonzero(lo[:cell] > hi[cell])[0]
    assert len(before) == 0, "[%s] peak beaten: cell %d before %d holds at least %d, more than %d" % (name, before[0] if len(before) else -1, cell, lo[before[0]] if len(before) else 0, hi[cell])
    if lo[cell] == hi[cell]:
        tied = np.nonzero((lo[:cell] == hi[:cell]) & (lo[:cell] == lo[cell]))[0]
        assert len(tied) == 0, "[%s] peak tie: cell %d before %d holds the same %d" % (name, tied[0] if len(tied) else -1, cell, lo[cell])


def peak_candidates(A):
    """the cells check_peak lets pass"""
    out = []
    for c in np.nonzero(A["hi"] >= A["lo"].max())[0]:
        try:
            check_peak("", c, A)
            out.append(int(c))
        except AssertionError:
            pass
    return out


def cell_point(cell, d):
    """cell -> the point it stands for in normalised homogeneous coordinates, with the bound of its fp32 evaluation"""
    ix, iy = cell % d, cell // d
    u, v = 2.0 * ix / (d - 1) - 1.0, 2.0 * iy / (d - 1) - 1.0
    return np.array([v, abs(u) + abs(v) - 1.0, u]), np.full(3, 8 * U)


def check_vanishing_point(name, vp, A, lines):
    """what lr_cht_vanishing_point returns (the de-normalised point of the strongest cell) -> that cell.  Every cell whose
    point is the returned one within the fp32 bound is looked up; one of them has to be an allowed peak."""
    d = A["d"]
    cx, cy, scale = [float(t) for t in N.normalisation_f32(lines)]
    vp = np.asarray(vp, np.float64)
    match = []
    for cell in range(d * d):
        p, _ = cell_point(cell, d)
        if p[2] == 0.0:
            ok = vp[2] == 0.0 and abs(vp[0] - p[0]) <= 8 * U and abs(vp[1] - p[1]) <= 8 * U
        else:
            X, Y = p[0] / p[2], p[1] / p[2]
            tx = scale * G * ((3 * U + 3 * U * abs(X)) * (d - 1) + U * abs(X)) + 2 * U * (abs(scale * X) + abs(cx))
            ty = scale * G * ((8 * U + 3 * U * abs(Y)) * (d - 1) + U * abs(Y)) + 2 * U * (abs(scale * Y) + abs(cy))
            ok = vp[2] == 1.0 and abs(vp[0] - (scale * X + cx)) <= tx and abs(vp[1] - (scale * Y + cy)) <= ty
        if ok:
            match.append(cell)
    assert match, "[%s] vanishing point: %r is the point of no cell" % (name, vp)
    errors = []
    for cell in match:
        try:
            check_peak(name, cell, A)
            return cell
        except AssertionError as e:
            errors.append(e)
    raise errors[0]


# ---- diamond space: the estimator ----------------------------------------------------------------------------------------
def cht_chain(name, segments, d, max_models, cells, inlier_deg=2.0, garbage_deg=4.0):
    """estimate_line_pencils_cht as far as float64 can say what fp32 does: peel_chain's rounds, where the hypothesis of round k
    is the point of cells[k], the cell the implementation returned -- which is checked against the accumulator of the lines
    still in the game.  -> peel_chain's dict, and votes_lo / votes_hi: the votes cast and taken back over the decided rounds"""
    D = {}
    cells = [int(c) for c in cells]

    def propose(M, obs, k, tol, dtol):
        if "d" not in D:
            D["d"] = Diamond(M, d)
        assert k < len(cells), "[%s] rounds: the second source starts round %d, the result has %d" % (name, k, len(cells))
        A = D["d"].intervals(obs)
        check_peak("%s, round %d" % (name, k), cells[k], A)
        p, dp = cell_point(cells[k], d)
        return cells[k], p, dp, ""

    chain = N.peel_chain(segments, 0, 0, max_models, inlier_deg, garbage_deg, propose=propose)
    if chain["complete"]:
        assert len(cells) == chain["rounds"], "[%s] rounds: %d ran, the second source ends after %d" % (name, len(cells), chain["rounds"])
    if len(segments):  # the votes of every line are cast once, whether a round follows or not
        if "d" not in D:
            D["d"] = Diamond(N.Model(N._xy(N.normalised_f32(segments))), d)
        A = D["d"].intervals()
        lo, hi = A["count_lo"], A["count_hi"]
        left = len(segments)
        for k, out in enumerate(chain["removed"]):
            left -= len(out)
            if left >= 2 and k + 1 < max_models and len(out):  # another round follows: the votes are taken back
                B = D["d"].intervals(out)
                lo, hi = lo + B["count_lo"], hi + B["count_hi"]
        chain.update(votes_lo=lo, votes_hi=hi, share=A["share"])
    else:
        chain.update(votes_lo=0, votes_hi=0, share=0.0)
    return chain


def check_models(name, models, chain):
    """the refit of every decided round, up to sign and scale, within the Davis-Kahan bound"""
    for k, (f, df) in enumerate(chain["refits"]):
        m = np.asarray(models[k], np.float64)
        m = m / np.linalg.norm(m)
        err = min(np.abs(m - f).max(), np.abs(m + f).max())
        assert err <= df.max() + 4 * U, "[%s] refit: round %d gives %r, the second source %r (+- %.3g)" % (name, k, m, f, df.max())


# ---- Hough weights (line_pencil.cpp:47-86) -----------------------------------------------------------------------------------
# The bands.  Vote pairs: std::mt19937, default seeded, through std::uniform_int_distribution<int>(0, n - 1) -- integers,
# restated below (the generator from its published recurrence, pinned by the standard's known answer: the 10000th output
# is 4123659995; the distribution as libstdc++ maps a 32-bit generator: Lemire's multiply-and-reject, bits/uniform_int_dist.h).
# Per pair x = h_a x h_b with the bound dp of numpy_grouping_ref.hypotheses (two copies of a record give exact zeros).
#   * skip test: all |x_k| < 1e-4f.  Surely skipped if every |x_k| + dp_k is below, surely kept if some |x_k| - dp_k is not.
#   * n = x / |x|: (dp_k + |n_k| |dp|) / |x| from the perturbed quotient, 4u for the squares, sums, root and quotient.
#   * flip if z < 0: sure if |x_z| > dp_z, or x_z is an exact zero (then nothing is flipped); else the vote is open between
#     the cell and its mirror image.
#   * cells round(k1 n_x + k), k = floor(S / 2), k1 = k - 1: dpos = k1 dn + u (|k1 n_x| + |pos|); sure if further than that from a
#     half, else one of two.
#   * vote floor((len_a + len_b) 2^20 + 0.5): each length carries 3u relative (none where the segment is parallel to an axis:
#     sqrt(fl(x^2)) = |x|), the sum u (none where the float64 sum is an fp32 number), the scaling and the half nothing below
#     2^22: the vote is any integer from floor(t - dv) to floor(t + dv).
# A cell is an interval: lo sums the lower votes of the pairs that surely land there, hi the upper votes of all that may.
# Peak: the first maximum in COLUMN-major order (Eigen's maxCoeff visitor on a column-major array); cells are kept in that
# order here, position v S + u, so that check_peak's "earlier" is the text's.
# Peak point p = ((u - k) / k1, (v - k) / k1, .): with i = u - k, j = v - k integers, |p| > 1 iff i^2 + j^2 > k1^2 (the nearest
# other integers are a relative 1 / k1^2 away: sure).  Inside: z^2 = 1 - (p0^2 + p1^2) >= 1 / k1^2 or exactly 0 (p0 = +-1), off by 6u.
# Outside p is normalised (5u per component), the radicand is 0 +- 14u, and z is anything from 0 to sqrt(14u) = 9e-4 -- or,
# as line_pencil.cpp:83 writes it, the root of a radicand that rounding left below zero: NaN, and then EVERY weight is NaN.
# Where pairs voted both outcomes are what the text implies, and check_weights takes either (all weights NaN, or all
# within their bands).  Where nobody voted (cell (0, 0), always beyond the rim) the library and the oracle take the radicand
# as 0, the ideal point: the weights have to be numbers.  The weight of a line is |cos|^4 of its direction against the point: err and band of
# numpy_grouping_ref.line_errors (whose ideal-point branch covers z in [0, 9e-4]), inc = 1 - err, and (inc + b)^4 - inc^4 <=
# 4 inc^3 b + 11 b^2, plus 4u for the two squarings.  A line whose anchor is within its bound of the point (0 / 0) is undecided.
HT_SIZE, HT_PAIRS = 65, 20000  # line_pencil.h: ht_space_size, ht_num_hypotheses
HT_SKIP = float(np.float32(0.0001))


def mt19937(count, seed=5489):
    """the first `count` outputs of std::mt19937 (Matsumoto & Nishimura 1998), in Python integers"""
    mt = [0] * 624
    mt[0] = seed
    for i in range(1, 624):
        mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
    out = []
    while len(out) < count:
        for i in range(624):
            y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        for y in mt:
            y ^= y >> 11
            y ^= (y << 7) & 0x9D2C5680
            y ^= (y << 15) & 0xEFC60000
            out.append(y ^ (y >> 18))
    return out[:count]


_MT = []


def vote_pairs(n, n_pairs=HT_PAIRS):
    """the pairs (a, b) of positions in 0..n-1 that get_weights draws: uniform_int_distribution<int>(0, n - 1) of libstdc++
    over a 32-bit generator: product = g() n; while its low word is below 2^32 mod n, draw again; the high word"""
    if not _MT:
        _MT.extend(mt19937(4 * HT_PAIRS))
    threshold = (1 << 32) % n
    out, at = [], 0
    while len(out) < 2 * n_pairs:
        product = _MT[at] * n
        at += 1
        if (product & 0xFFFFFFFF) >= threshold:
            out.append(product >> 32)
    pairs = np.array(out, np.int64).reshape(-1, 2)
    return pairs[:, 0], pairs[:, 1]


def _length_bounds(M, xy):
    axis = (xy[:, 0] == xy[:, 2]) | (xy[:, 1] == xy[:, 3])
    return np.where(axis, 0.0, 3 * U * M.length)


def ht_accumulator(norm, idx, size=HT_SIZE, n_pairs=HT_PAIRS):
    """the accumulator of get_weights over the lines idx of the normalised records -> dict(lo, hi: per cell in column-major
    order (position v size + u), open: pairs with an open decision, cast: pairs that surely vote, M)"""
    xy = N._xy(norm)
    M = N.Model(xy)
    idx = np.asarray(idx, np.int64)
    dlen = _length_bounds(M, xy)
    k = float(size // 2)
    k1 = k - 1
    pa, pb = vote_pairs(len(idx), n_pairs)
    ia, ib = idx[pa], idx[pb]
    x, dx, _ = N.hypotheses(M, ia, ib)
    same = M.canon[ia] == M.canon[ib]
    skip = same | (np.abs(x) + dx < HT_SKIP).all(1)
    keep = ~same & (np.abs(x) - dx >= HT_SKIP).any(1)
    nrm = np.linalg.norm(x, axis=1)
    nz = np.where(nrm > 0, nrm, 1.0)
    n = x / nz[:, None]
    dn = G * (dx + np.abs(n) * np.linalg.norm(dx, axis=1)[:, None]) / nz[:, None] + 4 * U
    z_zero = (x[:, 2] == 0) & (dx[:, 2] == 0)
    z_sure = z_zero | (np.abs(x[:, 2]) > dx[:, 2])
    s = np.where(x[:, 2] < 0, -1.0, 1.0)
    pos = k1 * n[:, :2] * s[:, None] + k
    dpos = G * (k1 * dn[:, :2] + U * (np.abs(k1 * n[:, :2]) + np.abs(pos)))
    fl = np.floor(pos)
    cell_sure = np.abs(pos - fl - 0.5) > dpos
    cell = np.floor(pos + 0.5).astype(np.int64)
    total = M.length[ia] + M.length[ib]
    exact_sum = total == total.astype(np.float32).astype(np.float64)
    dv = (G * (dlen[ia] + dlen[ib]) + np.where(exact_sum, 0.0, U * total)) * 1048576.0
    t = total * 1048576.0 + 0.5
    v_lo, v_hi = np.floor(t - dv).astype(np.int64), np.floor(t + dv).astype(np.int64)
    lo, hi = np.zeros(size * size, np.int64), np.zeros(size * size, np.int64)
    sure = keep & z_sure & cell_sure.all(1)
    where = cell[:, 1] * size + cell[:, 0]
    np.add.at(lo, where[sure], v_lo[sure])
    np.add.at(hi, where[sure], v_hi[sure])
    opened = np.nonzero(~sure & ~skip)[0]
    for i in opened:  # every cell the vote may land in
        us = [cell[i, 0]] if cell_sure[i, 0] else [int(fl[i, 0]), int(fl[i, 0]) + 1]
        vs = [cell[i, 1]] if cell_sure[i, 1] else [int(fl[i, 1]), int(fl[i, 1]) + 1]
        cand = {(u, v) for u in us for v in vs}
        if not z_sure[i]:
            cand |= {(int(2 * k) - u, int(2 * k) - v) for u, v in cand}
        for u, v in cand:
            if 0 <= u < size and 0 <= v < size:
                hi[v * size + u] += v_hi[i]
    return dict(lo=lo, hi=hi, open=len(opened), cast=int(sure.sum()), M=M, size=size, idx=idx, d=size)


def ht_peak_point(position, size=HT_SIZE):
    """column-major position -> the point (p, dp) the weights are taken against"""
    k = size // 2
    k1 = k - 1
    u, v = position % size, position // size
    i, j = u - k, v - k
    r2 = i * i + j * j
    if r2 > k1 * k1:
        z_max = np.sqrt(G * 14 * U)
        return np.array([i / np.sqrt(r2), j / np.sqrt(r2), z_max / 2]), np.array([5 * U, 5 * U, z_max / 2])
    p0, p1 = i / k1, j / k1
    if r2 == k1 * k1:
        return np.array([p0, p1, 0.0]), np.zeros(3)
    z = np.sqrt(1.0 - (p0 * p0 + p1 * p1))
    return np.array([p0, p1, z]), np.array([U * abs(p0), U * abs(p1), G * 6 * U / (2 * z) + U * z])


def ht_weights(H, position):
    """the weights of the lines H['idx'] against the point of the cell at `position` -> (w, dw; dw = inf: undecided)"""
    p, dp = ht_peak_point(position, H["size"])
    err, band, _, zero = N.line_errors(H["M"], H["idx"], p[None, :], dp[None, :])
    err, band = err[0], np.where(zero[0], np.inf, band[0])
    known = np.isfinite(band)
    inc, b = np.where(known, 1.0 - err, 0.0), np.where(known, band, 0.0)
    return inc ** 4, np.where(known, G * (4 * inc ** 3 * b + 11 * b * b) + 4 * U, np.inf)


def check_weights(name, weights, H):
    """lr_ht_weights returns only the weights: they have to be those of ONE allowed peak, on every line -> that position"""
    got = np.asarray(weights, np.float64)
    assert len(got) == len(H["idx"]), "[%s] %d weights for %d lines" % (name, len(got), len(H["idx"]))
    first = None
    k1 = H["size"] // 2 - 1
    for position in peak_candidates(H):
        i, j = position % H["size"] - (k1 + 1), position // H["size"] - (k1 + 1)
        if i * i + j * j > k1 * k1 and H["hi"].any() and np.isnan(got).all():
            return position  # a voted peak beyond the rim whose radicand fell below zero
        w, dw = ht_weights(H, position)
        with np.errstate(invalid="ignore"):
            bad = np.nonzero(np.isfinite(dw) & ~(np.abs(got - w) <= dw))[0]
        if len(bad) == 0:
            return position
        if first is None:
            first = "[%s] weight: line %d has %r, against the peak (u %d, v %d) it is %.9g +- %.3g (%d lines differ)" % (
                name, bad[0], weights[bad[0]], position % H["size"], position // H["size"], w[bad[0]], dw[bad[0]], len(bad))
    raise AssertionError(first)


# ---- PROSAC (prosac.h:104-299) ------------------------------------------------------------------------------------------------
# The sequential loop as written, with the documented deviations of the canonical text: samples from the counter-based
# generator (sample_pair of numpy_grouping_ref for the finishing stage; one uniform index out of n - 1 -- the low word of the
# same hash by multiply-high -- paired with u_n for the growth stage), and prosac.h:186's sample(m - 1) = n read as n - 1.
# The replay is fed the implementation's own Hough weights (the weights are checked by the part above: each stage is fed
# the output of the stage before) and sorts them as utils.h:36-44 does, stably and descending, a NaN last.
# Bands: the support of a hypothesis is the count of `err < tol` over all lines: line_errors / decide of the grouping source give
# the sure and the ambiguous inliers, I_N in [lo, hi].  The loop's bookkeeping (growth function, Imin, niter_RANSAC) is float64
# in the text and float64 here, operation by operation; its constants are the floats of prosac.h:62-66 widened.  Three
# comparisons hinge on counts: I_N > I_N_best, the maximality tests and I_n_best n_star > I_n_star n_best.  Where an interval
# leaves one of them open -- or a float64 comparison of the termination length is closer than 1e-9 relative -- the replay
# STOPS UNDECIDED; what it decided up to there is checked, and the cases are chosen so that it stops only after the
# result's best iteration.
_CHI2 = [np.inf, 6.6348966, 5.41189443, 4.70929225, 4.21788459, 3.84145882, 3.5373846, 3.28302029, 3.06490172, 2.8743734, 2.70554345,
         2.55422131, 2.41732093, 2.29250453, 2.17795916, 2.07225086, 1.97422609, 1.88294329, 1.79762406, 1.71761761]  # prosac.h:20-25
_F = np.float32
PROSAC = dict(eta=float(_F(0.05)), beta=float(_F(0.01)), p_good=float(_F(0.9)), max_outlier=float(_F(0.5)),
              chi2=float(_F(_CHI2[int(np.floor(np.clip(_F(2) * _F(0.02), _F(0.01), _F(0.2)) * _F(100)))])))


def niter_ransac(p, epsilon, s, n_max):
    """prosac.h:31-55 -> (value, whether the ceiling is clear of an integer)"""
    if n_max == -1:
        n_max = 2 ** 31 - 1
    if epsilon <= 0.0:
        return 1, True
    logval = np.log(1.0 + -np.exp(s * np.log(1.0 - epsilon)))
    n = np.log(1.0 - p) / logval
    if logval < 0.0 and n < n_max:
        return int(np.ceil(n)), abs(n - round(n)) > 1e-9 * max(1.0, abs(n)) and abs(n - n_max) > 1e-9 * n_max
    return n_max, True


def sample_one(seed, rnd, it, n):
    """one uniform index out of n: the low word of sample_pair's hash by multiply-high"""
    z = N.splitmix64(seed ^ N.splitmix64((rnd << 32) | it))
    return ((z & 0xFFFFFFFF) * n) >> 32


def stable_order_descending(weights):
    """utils.h:36-44: argsort, stable, descending; NaN weights last in their own order"""
    w = np.asarray(weights, np.float64)
    return np.array(sorted(range(len(w)), key=lambda i: (1, 0.0) if np.isnan(w[i]) else (0, -w[i])), np.int64)


class _Growth:
    def __init__(self, T_N, n_lines, m=2):
        self.t, self.n, self.T_n_prime, self.T_n = 0, m, 1, float(T_N)
        for i in range(m):
            self.T_n *= float(self.n - i) / (n_lines - i)

    def copy(self):
        g = _Growth.__new__(_Growth)
        g.__dict__.update(self.__dict__)
        return g

    def advance(self, n_star, m=2):
        self.t += 1
        if self.t > self.T_n_prime and self.n < n_star:
            nxt = (self.T_n * (self.n + 1)) / (self.n + 1 - m)
            self.n += 1
            self.T_n_prime += int(np.ceil(nxt - self.T_n))
            self.T_n = nxt

    def sample(self, seed, rnd):
        if self.t > self.T_n_prime:
            return N.sample_pair(seed, rnd, self.t, self.n)
        return sample_one(seed, rnd, self.t, self.n - 1), self.n - 1


def prosac_replay(norm, indices, tol, T_N, seed, rnd, weights, dtol=0.0, model=None):
    """PROSAC_Estimator::solve over the lines `indices` of the normalised records -> dict(iterations, n_star, best_iter, I_lo,
    I_hi, inliers: the best hypothesis's sure inliers (line numbers) or None if some are open, complete, reason, events: (t,
    lo, hi, n_star, k_n_star) of every new best whose termination length is decided, best_pair: its two lines, counts: per iteration its support's interval (-1: the sample failed its check), M, idx)"""
    M = N.Model(N._xy(norm)) if model is None else model
    indices = np.asarray(indices, np.int64)
    idx = indices[stable_order_descending(weights)]
    n_lines, m = len(idx), 2
    T_N = T_N if T_N > 0 else niter_ransac(PROSAC["p_good"], PROSAC["max_outlier"], m, -1)[0]
    R = dict(iterations=0, n_star=n_lines, best_iter=-1, I_lo=0, I_hi=0, inliers=np.zeros(0, np.int64), complete=True, reason="complete",
             events=[], counts=[], M=M, idx=idx, T_N=T_N)
    if n_lines < 2:
        return R
    beta = PROSAC["beta"]

    def imin(n):
        return int(np.ceil(m + n * beta + np.sqrt(n * beta * (1 - beta)) * np.sqrt(PROSAC["chi2"])))

    n_star, I_n_star, best_lo, best_hi, k_n_star = n_lines, 0, 0, 0, T_N
    I_N_min = int((1.0 - PROSAC["max_outlier"]) * n_lines)
    g = _Growth(T_N, n_lines)
    batch = max(16, min(4096, (1 << 21) // n_lines))

    def running(s):
        return (best_hi < I_N_min or s.t <= k_n_star) and s.t < T_N

    def stop(reason):
        R.update(complete=False, reason=reason, iterations=g.t, n_star=n_star)
        return R

    while running(g):
        if best_lo < I_N_min <= best_hi:
            return stop("iteration %d: whether the best support %d..%d reaches the minimum %d is open" % (g.t, best_lo, best_hi, I_N_min))
        plan, s = [], g.copy()
        while len(plan) < batch and running(s):
            s.advance(n_star)
            plan.append((s.copy(), s.sample(seed, rnd)))
        ia = idx[np.array([p[1][0] for p in plan])]
        ib = idx[np.array([p[1][1] for p in plan])]
        p, dp, valid = N.hypotheses(M, ia, ib)
        err, band, _, _ = N.line_errors(M, idx, p, dp, dtol)
        sure, amb = N.decide(err, band, tol)
        lo, hi = sure.sum(1), (sure | amb).sum(1)
        for j, (state, _) in enumerate(plan):
            g = state
            if valid[j] == 0:
                return stop("iteration %d: the sample check is open" % g.t)
            if valid[j] < 0:
                R["counts"].append((-1, -1))
                continue
            R["counts"].append((int(lo[j]), int(hi[j])))
            if hi[j] <= best_lo:
                continue
            if lo[j] <= best_hi:
                return stop("iteration %d: support %d..%d against the best %d..%d is open" % (g.t, lo[j], hi[j], best_lo, best_hi))
            best_lo, best_hi = int(lo[j]), int(hi[j])
            R.update(best_iter=g.t, I_lo=best_lo, I_hi=best_hi, inliers=None if amb[j].any() else idx[sure[j]])
            R["best_pair"] = (int(ia[j]), int(ib[j]))
            if amb[j].any():
                return stop("iteration %d: a new best with %d lines inside the band: the termination length is open" % (g.t, amb[j].sum()))
            # the search for the termination length (prosac.h:236-282)
            pre = np.concatenate([[0], np.cumsum(sure[j])])
            I_N = best_lo
            n_best, I_n_best, eps = n_lines, I_N, float(I_N) / n_lines
            for n_test in range(n_lines, m, -1):
                I_n_test = int(pre[n_test])
                if I_n_test * n_best > I_n_best * n_test:
                    rhs = eps * n_test + np.sqrt(n_test * eps * (1.0 - eps) * 2.706)
                    if abs(I_n_test - rhs) <= 1e-9 * max(1.0, rhs):
                        return stop("iteration %d: the maximality test at length %d is open" % (g.t, n_test))
                    if I_n_test > rhs:
                        if I_n_test < imin(n_test):
                            break
                        n_best, I_n_best = n_test, I_n_test
                        eps = float(I_n_best) / n_best
            if I_n_best * n_star > I_n_star * n_best:
                n_star, I_n_star = n_best, I_n_best
                k_n_star, clear = niter_ransac(1.0 - PROSAC["eta"], 1.0 - I_n_star / float(n_star), m, T_N)
                if not clear:
                    return stop("iteration %d: the number of samples for the new termination length is open" % g.t)
            R["events"].append((g.t, best_lo, best_hi, n_star, k_n_star))
            break  # the plan was drawn with the old n_star
    R.update(iterations=g.t, n_star=n_star)
    return R


def check_prosac(name, result, R):
    """result: dict(h, iterations, n_star, best_iter, I_N_best) of one solve"""
    assert result["best_iter"] == R["best_iter"], "[%s] best_iter: %d, the second source's %d (%s)" % (name, result["best_iter"], R["best_iter"], R["reason"])
    assert R["I_lo"] <= result["I_N_best"] <= R["I_hi"], "[%s] I_N_best: %d outside [%d, %d]" % (name, result["I_N_best"], R["I_lo"], R["I_hi"])
    if R["complete"]:
        assert result["iterations"] == R["iterations"], "[%s] iterations: %d, the second source's %d" % (name, result["iterations"], R["iterations"])
        assert result["n_star"] == R["n_star"], "[%s] n_star: %d, the second source's %d" % (name, result["n_star"], R["n_star"])
    else:
        assert result["iterations"] >= R["iterations"], "[%s] iterations: %d, the second source is at %d and undecided" % (name, result["iterations"], R["iterations"])
    if R["inliers"] is not None:
        f, df = N.refit(R["M"], R["inliers"] if len(R["inliers"]) else None)
        h = np.asarray(result["h"], np.float64)
        if df is not None and np.linalg.norm(h) > 0:
            h = h / np.linalg.norm(h)
            err = min(np.abs(h - f).max(), np.abs(h + f).max())
            assert err <= df.max() + 4 * U, "[%s] h: %r, fit_optimal of the %d inliers is %r (+- %.3g)" % (name, h, len(R["inliers"]), f, df.max())
            return dict(h_checked=True)
    return dict(h_checked=False)


def prosac_paths(R, seed, rnd):
    """Which paths of the chunked host replay (speculative chunks of 2048, 8192, 32 768, 65 536 iterations, two in flight;
    a chunk is cut where, after a new best, the loop ends or the true state draws another sample than the one the chunk was
    generated with; the sizes go on growing all the same) a case reaches, worked out from the second source's own trace
    -> dict(chunks: iterations used of every chunk, drawn: their generated lengths, wide: a chunk of 16 384 or more is
    generated (eight hypotheses per wavefront), new_bests: the most inside one chunk, beyond_cap: a new best whose rank
    among the chunk's records is beyond 32, cuts)"""
    events = {e[0]: e for e in R["events"]}
    n_lines, T_N = len(R["idx"]), R["T_N"]
    I_N_min = int((1.0 - PROSAC["max_outlier"]) * n_lines)
    st = dict(best=0, n_star=n_lines, k=T_N, size=2048)
    out = dict(chunks=[], drawn=[], wide=False, new_bests=0, beyond_cap=False, cuts=0)
    if n_lines < 2:
        return out

    def running(s):
        return (st["best"] < I_N_min or s.t <= st["k"]) and s.t < T_N

    def draw(start):
        s, samples = start.copy(), []
        while len(samples) < st["size"] and running(s):
            s.advance(st["n_star"])
            samples.append(s.sample(seed, rnd))
        ch = dict(start=start.copy(), end=s, samples=samples, n_star=st["n_star"], best_in=st["best"])
        if samples:
            out["drawn"].append(len(samples))
            out["wide"] = out["wide"] or len(samples) >= 16384
            st["size"] = min(4 * st["size"], 1 << 16)
        return ch

    g = _Growth(T_N, n_lines)
    cur = nxt = None
    while running(g) and g.t < R["iterations"]:
        if cur is None:
            cur = draw(g)
            if not cur["samples"]:
                break
        if nxt is None:
            nxt = draw(cur["end"])
        same = cur["n_star"] == st["n_star"] and cur["start"].__dict__ == g.__dict__
        top, rank, found, j = cur["best_in"], 0, 0, 0
        while j < len(cur["samples"]) and running(g) and g.t < R["iterations"]:
            gn = g.copy()
            gn.advance(st["n_star"])
            if not same and gn.sample(seed, rnd) != cur["samples"][j]:
                break
            g = gn
            count = R["counts"][g.t - 1][0]
            if count > top:
                top, rank = count, rank + 1
            if g.t in events:
                found += 1
                out["beyond_cap"] = out["beyond_cap"] or rank > 32
                _, lo, _, n_star, k = events[g.t]
                same = same and n_star == st["n_star"]
                st.update(best=lo, n_star=n_star, k=k)
            j += 1
        out["chunks"].append(j)
        out["new_bests"] = max(out["new_bests"], found)
        if j == len(cur["samples"]) and nxt["samples"]:
            cur, nxt = nxt, None
        else:
            out["cuts"] += j < len(cur["samples"])
            cur = nxt = None
    return out
