"""A SECOND, independent source for the vanishing-point grouping -- the sampling rule, the RANSAC scoring
(estimator.h:37-78, line_pencil.cpp:89-140, geometry.cpp:214-229) and the peeling rounds (estimator.h:99-145,
line_pencil.cpp:25-32,111-128,148-177) -- in float64 NumPy, written from the reference's text.  The oracle and the kernels
(kernels_ransac.hip, kernels_groups.hip) share their scalar fp32 formulas; this file shares nothing with either and does not
try to reproduce their bits.  It brackets them instead: every fp32 decision of the canonical text is either SURE here (the
float64 value is further from its threshold than fp32 rounding can move it) or AMBIGUOUS, a score is an interval [lo, hi],
and a result is checked for lying inside what the intervals allow.  Test infrastructure only.

The bands (u = 2^-24, the unit roundoff of fp32; (1 + u)^k <= 1 + 1.01 k u for the k used here)
---------------------------------------------------------------------------------------------
Inputs.  The model is built from NORMALISED fp32 segments.  lr_ransac_best takes them from its caller;
lr_estimate_line_pencils makes them itself (geometry.cpp:96-112,258-282): size = max - min, centre = min + 0.5 size, scale =
the larger side, x' = (x - centre) / scale, five fp32 operations whose order the text fixes.  normalised_f32() below does
exactly those in numpy.float32 and nothing more; everything after it is float64.  (Bounding them instead costs the test its
teeth: an error of u in an end point turns a segment of length 0.03 by 4e-6, the refit of a pencil inherits that through
an eigenvalue gap of a few percent, and every round has lines inside such a band.)

Model of a line (line_pencil.cpp:25-32), from exact inputs.  h_raw = (y1 - y2, x2 - x1, x1 y2 - y1 x2): the differences
carry u |.|, the third component u (|x1 y2| + |y1 x2|) + u |h_raw.z| (two products, one difference; nothing where the two
products are the same real number, as for a segment whose end points mirror each other in the centre).  The norm N = |h_raw| is
three squares, two sums and a root (relative 3u / 2 + u) and the quotient adds u: with the error vector r of h_raw,
dh_k <= r_k / N + |h_k| (|r| / N + 4u).  The anchor (p1 + p2) / 2 carries u |a| per component.  The direction
(p2 - p1) / |p2 - p1| is off, as a vector, by at most  dd = 2 |r_d| / len + 4u = 6u  (r_d: error of the difference, u |.| per
component; once for the numerator, once through the norm; 4u for the norm's and the quotient's own roundings), and the
length by the relative 3u, which the score's bound below counts.

Sample check (line_pencil.cpp:89-98).  dist = |h_a - h_b| against 0.05f: off by at most |dh_a| + |dh_b| + 4u dist.

Hypothesis p = h_a x h_b (line_pencil.cpp:101-108).  Each component is two products and a difference of perturbed
inputs: dp = X(|h_a| + dh_a, |h_b| + dh_b) - X(|h_a|, |h_b|) + 2u X(|h_a|, |h_b|) with X the cross product taken with plus
signs.  The ideal-point test |p.z| < 1e-6f (geometry.cpp:218) is sure if |p.z| is further than dp.z from the threshold.
Only the DIRECTION of v enters the error, up to sign: for a finite point v = p.xy / p.z - anchor is parallel to
w = p.xy - anchor p.z, which is off by dw = dp.xy + |anchor| dp.z + da |p.z| + u (|p.xy| + |w|) (the last term: the roundings of
the quotient and of the difference, scaled by p.z like the rest); for an ideal point w = p.xy and dw = dp.xy.  This form
has no quotient by p.z, so a far point costs nothing.  Where the ideal-point test is open, w = p.xy with
dw + (|p.z| + dp.z) (|anchor| + da) covers both branches.

Error of a line (geometry.cpp:224-228).  err = 1 - |cos t| with t the angle between v and the direction d.  Turning v by
at most rho = |dw| / |w| and d by at most dd turns t by phi <= rho + dd (phi < 1/4 is required, else the line is ambiguous),
and |cos(t + phi) - cos t| <= sin t phi + phi^2 / 2.  The fp32 evaluation itself: |v|^2 (2u), the root (u + u), the two
quotients (3u each), the dot product (products 4u, sum 5u on terms whose absolute values sum to at most 1), 1 - inc (u):
6u, taken as 8u.  So  band = 1.01 (sin t phi + phi^2) + 8u, plus 2^-23 where the tolerance is 1 - cosf(deg) evaluated in
fp32 by the callee (one rounding of the cosine, one of the difference).  The kernel's own band kErrBand = 3e-6 around the
same threshold is about its cheap ESTIMATE and is not used here.  |w| = 0 exactly, with dw = 0, gives NaN: surely not an
inlier (NaN < tol is false); with dw > 0 it is ambiguous.

Score.  lo = sum of the lengths of the sure inliers, hi = lo + the ambiguous ones.  The fp32 score is the canonical tree: per lane ceil(n / 64) sequential adds,
six butterfly levels, and the rounding of the lengths: (ceil(n / 64) + 8) u relative.

Refit (line_pencil.cpp:111-128).  cov = sum len h h^T in fp32 trees against the same sum in float64: entrywise
E = S(len (1 + 3u), |h| + dh) - S(len, |h|) + (ceil(m / 64) + 8) u S(len, |h|); the smallest eigenvalue's eigenvector moves by
at most 2 |E|_F / (gap - 2 |E|_F) (Davis-Kahan, gap = distance to the next eigenvalue), plus u for the cast.  A refit whose gap
is below 4 |E|_F is undecided.
"""
import numpy as np

from numpy_ref import fit_optimal

U = 2.0 ** -24
G = 1.01
EPS32 = float(np.float32(1e-6))  # config.h:59, as the float the comparison uses
DEGENERACY = float(np.float32(0.05))  # line_pencil.h:25
_M64 = (1 << 64) - 1


# ---- the sampling rule (common.h: sample_pair) ------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample_pair(seed, rnd, it, n):
    """iteration `it` of round `rnd`: two draws without replacement out of n by 32-bit multiply-high, ascending"""
    z = splitmix64(seed ^ splitmix64((rnd << 32) | it))
    i = ((z & 0xFFFFFFFF) * n) >> 32
    j = ((z >> 32) * (n - 1)) >> 32
    if j >= i:
        j += 1
    return (i, j) if i < j else (j, i)


def _splitmix64_v(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def sample_pairs(seed, rnd, n_iter, n):
    """sample_pair for iterations 0..n_iter-1 at once (uint64 arrays wrap as the integers above are masked)"""
    it = np.arange(n_iter, dtype=np.uint64)
    z = _splitmix64_v(np.uint64(seed) ^ _splitmix64_v((np.uint64(rnd) << np.uint64(32)) | it))
    i = ((z & np.uint64(0xFFFFFFFF)) * np.uint64(n)) >> np.uint64(32)
    j = ((z >> np.uint64(32)) * np.uint64(n - 1)) >> np.uint64(32)
    j = j + (j >= i).astype(np.uint64)
    return np.minimum(i, j).astype(np.int64), np.maximum(i, j).astype(np.int64)


# ---- normalisation and model ---------------------------------------------------------------------------------------------
def _xy(lines):
    return np.stack([np.asarray(lines[k], np.float64) for k in ("x1", "y1", "x2", "y2")], 1)


def normalisation_f32(lines):
    """geometry.cpp:96-112 in fp32 -> (centre x, centre y, scale) as the fp32 numbers the records are normalised with"""
    f = np.float32
    x = np.concatenate([lines["x1"], lines["x2"]]).astype(f)
    y = np.concatenate([lines["y1"], lines["y2"]]).astype(f)
    sx, sy = f(x.max() - x.min()), f(y.max() - y.min())
    return f(x.min() + f(0.5) * sx), f(y.min() + f(0.5) * sy), max(sx, sy)


def normalised_f32(lines):
    """geometry.cpp:96-112,258-282 in fp32, operation by operation (see the head of the file) -> fp32 records"""
    f = np.float32
    cx, cy, scale = normalisation_f32(lines)
    out = lines.copy()
    out["x1"], out["x2"] = (lines["x1"].astype(f) - cx) / scale, (lines["x2"].astype(f) - cx) / scale
    out["y1"], out["y2"] = (lines["y1"].astype(f) - cy) / scale, (lines["y2"].astype(f) - cy) / scale
    return out


class Model:
    """LinePencilModel (line_pencil.cpp:25-32) of normalised coordinates xy (n, 4), which are exact fp32 numbers"""

    def __init__(self, xy):
        xy = np.asarray(xy, np.float64)
        x1, y1, x2, y2 = xy.T
        raw = np.stack([y1 - y2, x2 - x1, x1 * y2 - y1 * x2], 1)
        r = U * np.stack([np.abs(raw[:, 0]), np.abs(raw[:, 1]), np.abs(x1 * y2) + np.abs(y1 * x2) + np.abs(raw[:, 2])], 1)
        # The same real number rounds to the same float, so the difference is an exact zero.  Two assumptions: the inputs
        # are fp32 numbers, whose float64 products here are exact (the test compares the real products), and the
        # implementations round both products before they subtract (built with -ffp-contract=off: no FMA of the difference).
        r[x1 * y2 == y1 * x2, 2] = 0.0
        nrm = np.linalg.norm(raw, axis=1)
        ok = nrm > 0
        nz = np.where(ok, nrm, 1.0)
        self.h = raw / nz[:, None]
        self.dh = np.where(ok[:, None], G * (r / nz[:, None] + np.abs(self.h) * (np.linalg.norm(r, axis=1) / nz + 4 * U)[:, None]), 1.0)
        self.a = np.stack([(x2 + x1) / 2, (y2 + y1) / 2], 1)
        self.da = U * np.linalg.norm(self.a, axis=1)
        dv = np.stack([x2 - x1, y2 - y1], 1)
        self.length = np.linalg.norm(dv, axis=1)
        self.d = dv / np.where(self.length > 0, self.length, 1.0)[:, None]
        self.dd = np.where(self.length > 0, G * 6 * U, 1.0)
        # lines with the same record have the same model, hence the same hypotheses and the same scores, bit for bit
        _, first, inv = np.unique(xy, axis=0, return_index=True, return_inverse=True)
        self.canon = first[np.asarray(inv).reshape(-1)]
        self.n = len(xy)


def _xabs(A, B):
    return np.stack([A[:, 1] * B[:, 2] + A[:, 2] * B[:, 1], A[:, 2] * B[:, 0] + A[:, 0] * B[:, 2],
                     A[:, 0] * B[:, 1] + A[:, 1] * B[:, 0]], 1)


def hypotheses(M, ia, ib):
    """samples (ia[k], ib[k]) -> p = h_a x h_b with its bound, and the sample check: +1 surely valid, -1 surely not, 0"""
    ha, hb, dha, dhb = M.h[ia], M.h[ib], M.dh[ia], M.dh[ib]
    dist = np.linalg.norm(ha - hb, axis=1)
    ddist = G * (np.linalg.norm(dha, axis=1) + np.linalg.norm(dhb, axis=1) + 4 * U * dist)
    same = M.canon[ia] == M.canon[ib]  # identical records: dist is exactly 0
    valid = np.where(same | (dist + ddist <= DEGENERACY), -1, np.where(dist - ddist > DEGENERACY, 1, 0))
    p = np.cross(ha, hb)
    A, B = np.abs(ha), np.abs(hb)
    dp = _xabs(A + dha, B + dhb) - _xabs(A, B) + 2 * U * _xabs(A, B)
    return p, dp, valid


def line_errors(M, idx, p, dp, dtol=0.0):
    """err (K, n) of the lines idx against the K points p (geometry.cpp:214-229) with band (K, n); band = inf where nothing
    can be said.  Also per point: ideal (+1 surely ideal, -1 surely finite, 0 open), and where v is exactly the zero vector."""
    pz, dpz = p[:, 2], dp[:, 2]
    ideal = np.where(np.abs(pz) + dpz < EPS32, 1, np.where(np.abs(pz) - dpz >= EPS32, -1, 0))
    a, d, da = M.a[idx], M.d[idx], M.da[idx]
    na = np.linalg.norm(a, axis=1)
    pxy, dpxy = p[:, :2], np.linalg.norm(dp[:, :2], axis=1)
    npxy = np.linalg.norm(pxy, axis=1)
    fin = ideal == -1
    # the direction of v, up to sign: p.xy - anchor p.z for a finite point, p.xy for an ideal one
    w = pxy[:, None, :] - np.where(fin, pz, 0.0)[:, None, None] * a[None, :, :]
    nw = np.linalg.norm(w, axis=2)
    dw = dpxy[:, None] + np.where(fin, dpz, 0.0)[:, None] * na[None, :] + np.where(fin, np.abs(pz), 0.0)[:, None] * da[None, :]
    dw = dw + np.where(fin, U, 0.0)[:, None] * (npxy[:, None] + nw)
    dw = dw + np.where(ideal == 0, np.abs(pz) + dpz, 0.0)[:, None] * (na + da)[None, :]  # open: either branch
    zero = nw == 0
    nz = np.where(zero, 1.0, nw)
    inc = np.abs((w * d[None, :, :]).sum(2)) / nz
    err = np.where(zero, np.nan, 1.0 - inc)
    phi = G * dw / nz + M.dd[idx][None, :]
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - np.minimum(inc, 1.0) ** 2))
    band = G * (sin_t * phi + phi * phi) + 8 * U + dtol
    band = np.where(phi >= 0.25, np.inf, band)
    band = np.where(zero, np.where(dw == 0, 0.0, np.inf), band)  # NaN for sure, or anything
    return err, band, ideal, zero


def decide(err, band, tol):
    """-> (sure inlier, ambiguous) for `err < tol` in fp32"""
    with np.errstate(invalid="ignore"):
        sure_in = err < tol - band
        sure_out = (err > tol + band) | (np.isnan(err) & (band == 0))
    return sure_in, ~(sure_in | sure_out)


def tree_bound(n):
    return (-(-n // 64) + 8) * U


def score_intervals(M, idx, tol, n_iter, seed, rnd, dtol=0.0):
    """every iteration of one solve (estimator.h:37-71) over the lines idx of the model: pair, validity, [lo, hi], coverage"""
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    a, b = sample_pairs(seed, rnd, n_iter, n)
    ia, ib = idx[a], idx[b]
    length = M.length[idx]
    lo, hi = np.zeros(n_iter), np.zeros(n_iter)
    valid, ideal = np.zeros(n_iter, np.int64), np.zeros(n_iter, np.int64)
    n_amb, n_nan = np.zeros(n_iter, np.int64), np.zeros(n_iter, np.int64)
    P, DP = np.zeros((n_iter, 3)), np.zeros((n_iter, 3))
    sets = np.zeros(n_iter, np.uint64)
    wts = np.random.RandomState(n).randint(1, 1 << 62, n).astype(np.uint64)
    step = max(1, (1 << 20) // max(n, 1))
    for s in range(0, n_iter, step):
        sl = slice(s, min(n_iter, s + step))
        p, dp, valid[sl] = hypotheses(M, ia[sl], ib[sl])
        P[sl], DP[sl] = p, dp
        err, band, ideal[sl], zero = line_errors(M, idx, p, dp, dtol)
        sure, amb = decide(err, band, tol)
        lo[sl] = (sure * length[None, :]).sum(1)
        hi[sl] = ((sure | amb) * length[None, :]).sum(1)
        n_amb[sl] = amb.sum(1)
        n_nan[sl] = zero.sum(1)
        with np.errstate(over="ignore"):
            sets[sl] = (sure * wts[None, :]).sum(1, dtype=np.uint64)
    lo = np.where(valid == 1, lo, 0.0)  # a sample that may fail the check may score nothing
    hi = np.where(valid == -1, 0.0, hi)
    cia, cib = M.canon[ia], M.canon[ib]
    key = np.minimum(cia, cib) * M.n + np.maximum(cia, cib)
    # Iterations that tie exactly: the same pair of (identical) lines, or the same inlier set with no line left open -- the
    # tree sum is a function of the set.  tie[i] is the first iteration of i's class.
    cls = np.where((valid == 1) & (n_amb == 0), sets, key.astype(np.uint64) | np.uint64(1 << 63))
    _, first, inv = np.unique(cls, return_index=True, return_inverse=True)
    tie = first[np.asarray(inv).reshape(-1)]
    return dict(tie=tie, n=n, n_iter=n_iter, a=a, b=b, ia=ia, ib=ib, lo=lo, hi=hi, valid=valid, ideal=ideal, n_amb=n_amb, n_nan=n_nan,
                key=key, p=P, dp=DP, bound=tree_bound(n))


def coverage(S):
    """what a content case asserts of itself"""
    ok = S["valid"] != -1  # (what a sample that fails the check would have scored is never looked at)
    return dict(ideal=int((ok & (S["ideal"] == 1)).sum()), invalid=int((~ok).sum()), in_band=int(S["n_amb"][ok].sum()),
                nan=int(S["n_nan"][ok].sum()))


def winner(S):
    """-> (iteration or -1, decided).  The winner by the intervals alone: -1 if surely nothing scores; the first iteration of
    the tie class whose lo is above the hi of every iteration outside it, if there is such a class; else open."""
    lo, hi, tie = S["lo"] * (1 - S["bound"]), S["hi"] * (1 + S["bound"]), S["tie"]
    if not (hi > 0).any():
        return -1, True
    k = int(np.argmax(lo))
    if lo[k] <= 0 or (hi[tie != tie[k]] >= lo[k]).any():
        return k, False
    return int(tie[k]), True


def check_ransac(name, result, S):
    """result: dict(iter, score, best_h) of one solve.  Raises AssertionError naming the case and the check; returns the
    counts that the callers print and assert."""
    it, score, bh = int(result["iter"]), float(result["score"]), np.asarray(result["best_h"], np.float64)
    lo, hi, B = S["lo"], S["hi"], S["bound"]
    scoring = np.nonzero((S["valid"] == 1) & (lo > 0))[0]
    if it < 0:
        assert it == -1, "[%s] iteration: %d" % (name, it)
        assert len(scoring) == 0, "[%s] surely better: nothing returned, but iteration %d surely scores %.9g" % (name, scoring[0], lo[scoring[0]])
        assert score == 0.0 and not bh.any(), "[%s] nothing scored: score %r and hypothesis %r must be zero" % (name, score, bh)
        return dict(decided=True, later_draws=0, later_ties=0, rivals=0)
    assert it < S["n_iter"], "[%s] iteration: %d of %d" % (name, it, S["n_iter"])
    assert hi[it] > 0, "[%s] score interval: iteration %d cannot score (sample check %d, hi 0)" % (name, it, S["valid"][it])
    assert lo[it] * (1 - B) <= score <= hi[it] * (1 + B), "[%s] score interval: %.9g outside [%.9g, %.9g] (1 +- %.3g) of iteration %d" % (
        name, score, lo[it], hi[it], B, it)
    better = np.nonzero(lo * (1 - B) > hi[it] * (1 + B))[0]
    assert len(better) == 0, "[%s] surely better: iteration %d scores at least %.9g, the returned %d at most %.9g" % (
        name, better[0], lo[better[0]], it, hi[it])
    same = np.nonzero(S["key"] == S["key"][it])[0]
    assert same[0] == it, "[%s] same pair earlier: iteration %d draws the pair of the returned %d" % (name, same[0], it)
    assert S["tie"][it] == it, "[%s] same inliers earlier: iteration %d has the inlier set of the returned %d" % (name, S["tie"][it], it)
    # the hypothesis itself: h_a x h_b of that pair
    p, dp = S["p"][it], S["dp"][it]
    assert (np.abs(bh - p) <= dp + U * np.abs(p)).all(), "[%s] hypothesis: %r is not h_a x h_b = %r (+- %r)" % (name, bh, p, dp)
    if np.linalg.norm(p) > 1e-3:
        c = abs(float(bh @ p)) / (np.linalg.norm(bh) * np.linalg.norm(p))
        assert np.sqrt(max(0.0, 2 - 2 * c)) <= 1e-5, "[%s] hypothesis: %r is not parallel to h_a x h_b = %r" % (name, bh, p)
    rivals = int(((S["tie"] != it) & (hi * (1 + B) >= lo[it] * (1 - B))).sum())
    return dict(decided=rivals == 0, later_draws=int(len(same) - 1), later_ties=int((S["tie"] == it).sum() - 1), rivals=rivals)


# ---- the peeling rounds (estimator.h:99-145 around line_pencil.cpp:111-128) -----------------------------------------
def cos_tolerance(deg):
    """line_pencil.cpp:143-146 -> (1 - cos(deg) in float64, bound of the fp32 evaluation)"""
    return 1.0 - np.cos(np.deg2rad(deg)), 2.0 ** -23


def refit(M, inl):
    """fit_optimal over the lines inl (None: every line of the model) -> (eigenvector, bound per component or None)"""
    sel = np.arange(M.n) if inl is None else np.asarray(inl, np.int64)
    h, L = M.h[sel], M.length[sel]
    f = fit_optimal(M.h, M.length, None if inl is None else sel)
    A, dA, dL = np.abs(h), M.dh[sel], L * 3 * U
    S0 = A.T @ (A * L[:, None])
    E = (A + dA).T @ ((A + dA) * (L + dL)[:, None]) - S0 + G * (-(-len(sel) // 64) + 8) * U * S0
    w = np.linalg.eigvalsh(h.T @ (h * L[:, None]))
    e, gap = float(np.linalg.norm(E)), float(w[1] - w[0])
    if gap < 4 * e:
        return f, None
    return f, np.full(3, 2 * e / (gap - 2 * e) + U)


def ransac_proposal(n_iter, seed):
    """the hypothesis of a round as estimate_line_pencils takes it: the winner of n_iter scored samples"""
    def propose(M, obs, k, tol, dtol):
        if n_iter <= 0:
            return -1, None, None, ""
        S = score_intervals(M, obs, tol, n_iter, seed, k, dtol)
        it, decided = winner(S)
        if not decided:
            return it, None, None, "round %d: the winner is open between iteration %d and its rivals" % (k, it)
        if it < 0:
            return -1, None, None, ""
        return it, S["p"][it], S["dp"][it], ""
    return propose


def peel_chain(segments, n_iter, seed, max_models, inlier_deg=2.0, garbage_deg=4.0, propose=None):
    """estimate_line_pencils as far as float64 can say what fp32 does.  -> dict(ids: expected group ids (valid for the lines
    in `settled`), settled: lines whose final id the decided rounds fix, rounds: rounds decided, complete: the chain ran to
    the end of the peeling, reason, per round: winner, its inliers, lines grouped / garbage / staying, the refit and its
    bound).  propose(M, obs, k, tol, dtol) -> (id of the hypothesis or -1 for none, p, dp, reason if it is open): where the
    round's hypothesis comes from; the default is the RANSAC solve, another estimator's second source passes its own and
    shares the verdicts."""
    n = len(segments)
    ids = -np.ones(n, np.int64)
    out = dict(ids=ids, settled=np.zeros(n, bool), rounds=0, complete=False, reason="", winners=[], winner_inliers=[], grouped=[],
               garbage=[], in_band=0, refits=[], removed=[])
    if n < 2 or max_models <= 0:
        out.update(settled=np.ones(n, bool), complete=True, reason="nothing to do")
        return out
    if propose is None:
        propose = ransac_proposal(n_iter, seed)
    M = Model(_xy(normalised_f32(segments)))
    tol, dtol = cos_tolerance(inlier_deg)
    gtol, _ = cos_tolerance(garbage_deg)
    obs = np.arange(n)
    for k in range(max_models):
        if len(obs) < 2:
            break
        inl = None
        it, p, dp, open_reason = propose(M, obs, k, tol, dtol)
        if open_reason:
            out["reason"] = open_reason
            return out
        if it >= 0:
            err, band, _, _ = line_errors(M, obs, p[None, :], dp[None, :], dtol)
            sure, amb = decide(err[0], band[0], tol)
            if amb.any():
                out["in_band"] += int(amb.sum())
                out["reason"] = "round %d: %d lines within the band of the winner's tolerance" % (k, amb.sum())
                return out
            inl = obs[sure]
            if len(inl) == 0:
                inl = None
        f, df = refit(M, inl)  # no winner, or a winner without inliers: every line of the model
        if df is None:
            out["reason"] = "round %d: the refit's eigenvector is not separated" % k
            return out
        err, band, _, _ = line_errors(M, obs, f[None, :], df[None, :], dtol)
        s_in, a_in = decide(err[0], band[0], tol)
        s_gb, a_gb = decide(err[0], band[0], gtol)
        if a_in.any() or a_gb.any():
            out["in_band"] += int((a_in | a_gb).sum())
            out["reason"] = "round %d: %d lines within the band of a threshold of the refit" % (k, (a_in | a_gb).sum())
            return out
        ids[obs[s_in]] = k
        out["settled"][obs[s_gb]] = True  # grouped, or garbage: out of the game with id -1
        out["winners"].append(it)
        out["winner_inliers"].append(0 if inl is None else len(inl))
        out["grouped"].append(int(s_in.sum()))
        out["garbage"].append(int((s_gb & ~s_in).sum()))
        out["refits"].append((f, df))
        out["removed"].append(obs[s_gb])
        obs = obs[~s_gb]
        out["rounds"] = k + 1
    out["settled"][:] = True
    out["complete"] = True
    out["reason"] = "complete"
    return out


def check_groups(name, group_id, chain):
    """the ids a grouping call returned against the rounds the chain decided"""
    got = np.asarray(group_id, np.int64)
    st, exp = chain["settled"], chain["ids"]
    bad = np.nonzero(st & (got != exp))[0]
    assert len(bad) == 0, "[%s] group id: line %d has %d, the second source %d (%d lines differ; %d rounds decided)" % (
        name, bad[0], got[bad[0]], exp[bad[0]], len(bad), chain["rounds"])
    stray = np.nonzero(~st & (got >= 0) & (got < chain["rounds"]))[0]
    assert len(stray) == 0, "[%s] group id: line %d has %d, a round whose members the second source knows" % (name, stray[0], got[stray[0]])
    return dict(rounds=chain["rounds"], complete=chain["complete"], settled=int(st.sum()))
