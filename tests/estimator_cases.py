"""The cases of the estimator second-source tests (test_estimators_second_source_cpu.py holds the oracle to them,
test_gpu_estimators_second_source.py the kernels) and the drivers that run an implementation through
numpy_estimators_ref's checks.  What each case is for is said where it is built.  Whether a case keeps its ambiguity cap,
has one candidate or is decided to the end depends on the second source alone, so seeds and coordinates were chosen on
the CPU; the CPU module asserts that they still hold.  Test infrastructure only."""
import functools

import numpy as np

import grouping_cases as Gc
import numpy_estimators_ref as E
import numpy_grouping_ref as N
from grouping_cases import records, segments


def pencils(counts, clutter, seed, noise=0.002, size=1000.0):
    """counts[k] segments on pencil k of grouping_cases.VPS (turned by N(0, noise) rad) and `clutter` uniform ones, in
    random order"""
    rng = np.random.RandomState(seed)
    which = np.concatenate([np.full(c, k) for k, c in enumerate(counts)] + [np.full(clutter, 3)]).astype(int)
    n = len(which)
    c = rng.uniform(0.05, 0.95, (n, 2)) * size
    half = rng.uniform(0.03, 0.15, n) * size / 2
    to_vp = Gc.VPS[np.minimum(which, 2)] - c
    ang = np.where(which < 3, np.arctan2(to_vp[:, 1], to_vp[:, 0]) + rng.normal(0, noise, n), rng.uniform(0, np.pi, n))
    dd = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    return records(c - dd, c + dd)[rng.permutation(n)]


def rows(*r):
    a = np.array(r, np.float64)
    return records(a[:, :2], a[:, 2:])


# ---- diamond space: the accumulator (lr_cht_vanishing_point) ---------------------------------------------------------
# name -> (segments, d, what the case asserts of itself from the second source)
#
# A set of copies of ONE segment is its own bounding box, so the line runs through the normalisation centre: c = 0
# exactly, d1 = a, d2 = b, and the polyline is (al, 0) -> (1, 0) -> (0, b / (a + al b)) -> (-al, 0).  With al = -1 (the
# segment rises to the right in image coordinates) the first segment is the whole middle row: 128 steps at d = 128.  The
# other two go from cell (127, 64) to (64, y) and back, y = round(63.5 (1 + b / (a - b))):
#   * the diagonal (0, 0)-(1000, 1000), a = -b: y = round(31.75) = 32, extent 63 both times: 64 steps (and the longest
#     possible vote, sqrt 2 in normalised coordinates: 92682 units);
#   * (0, 0)-(1000, 5), a = -b / 200: 63.5 (1 - 200 / 201) = 0.32, y = 0, extent 64: 65 steps.
DIAGONAL = rows([0, 0, 1000, 1000])
SHALLOW = rows([0, 0, 1000, 5])


def _accumulator():
    out = {}
    base = segments(1025, 41)
    for n in (1, 2, 3, 4, 5):  # the wavefront stride of four lines
        out["%d lines" % n] = (base[:n], 128, {})
    for n in (511, 512, 513, 1025):  # one workgroup of 512 lines short, full, and a ragged second and third
        out["%d lines" % n] = (base[:n], 128, {})
    for d in (8, 16, 127, 128):  # 64 cells under 1024 peak threads; an odd size, whose middle column is the ideal points
        out["200 lines, d = %d" % d] = (segments(200, 42), d, {})
    out["128 and 64 steps"] = (DIAGONAL, 128, dict(steps=[128, 64, 64]))
    out["128 and 65 steps"] = (SHALLOW, 128, dict(steps=[128, 65, 65]))
    # zero coefficients.  Alone, a horizontal segment has a = 0 and c = 0 (d1 = 0: its first and last segment are dropped), a
    # vertical one b = 0 and c = 0 (d2 = 0: the first two are dropped); among others they have a = 0 or b = 0 alone; the
    # diagonal of the set's bounding box has c = 0 alone.  (No line has all three dropped: that needs d1 = 0 or d2 = d3 = 0
    # on top of d2 = 0 or d3 = 0, which is a = b = c = 0.)
    # ... so the accumulator nobody voted for, and the peak kernel's answer to it (cell 0), take segments of no length:
    # three points.  Their h is 0 / 0 and the range test of the rasteriser lets no NaN pass.
    out["three points"] = (rows([100, 100, 100, 100], [400, 300, 400, 300], [250, 700, 250, 700]), 128, dict(exact=True, peak_value=0, cell=0))
    out["one horizontal"] = (rows([100, 300, 700, 300]), 128, dict(steps=[None, 64, None]))
    out["one vertical"] = (rows([400, 100, 400, 900]), 128, dict(steps=[None, None, 65]))
    out["horizontal, vertical, through the centre"] = (rows([0, 0, 1000, 1000], [100, 300, 700, 300], [400, 100, 400, 900], [0, 1000, 1000, 0],
                                                            [0, 500, 1000, 500], [500, 0, 500, 1000], [200, 200, 800, 650]), 128, dict(dropped=4))
    # the longest vote 600 and 50 000 times.  Cell (127, 64) is the end of the first segment, the start of the second and
    # (P3 = -P0 = (1, 0)) the end of the third: three votes a line, 3 x 512 x 92682 = 1.4e8 < 2^32 in the LDS of one workgroup;
    # 50 000 copies take it to 1.4e10, beyond the low word of the global atomic and of the peak kernel's shuffle
    out["600 diagonals"] = (np.tile(DIAGONAL, 600), 128, dict(exact=True, peak_value=600 * 3 * 92682))
    out["50 000 diagonals"] = (np.tile(DIAGONAL, 50000), 128, dict(exact=True, peak_value=50000 * 3 * 92682))
    # two segments, mirror images in the line y = 0: equal fp32 lengths, polylines mirrored in the row axis; the doubly
    # voted corner cells of the two tie exactly, and the first in row-major order is the answer
    out["mirror images"] = (rows([200, 100, 800, 300], [200, -100, 800, -300]), 128, dict(exact=True, tie=2))
    return out


ACCUMULATOR_CASES = _accumulator()


@functools.lru_cache(maxsize=None)
def diamond(name):
    segs, d, _ = ACCUMULATOR_CASES[name]
    D = E.Diamond(N.Model(N._xy(N.normalised_f32(segs))), d)
    return D, D.intervals()


def check_accumulator_case(name):
    """what the case asserts of itself, on the second source alone -> its ambiguous share"""
    segs, d, expect = ACCUMULATOR_CASES[name]
    D, A = diamond(name)
    assert A["share"] <= E.AMBIGUITY_CAP, "[%s] cap: %.4f of the votes are ambiguous" % (name, A["share"])
    assert not any(v["whole"] for v in D.votes.values()), "[%s] cap: a line is ambiguous as a whole" % name
    if "steps" in expect:
        assert D.of(0)["steps"] == expect["steps"], "[%s] coverage: steps %r, the case needs %r" % (name, D.of(0)["steps"], expect["steps"])
    if "dropped" in expect:
        k = sum(s is None for i in range(len(segs)) for s in D.of(i)["steps"])
        assert k >= expect["dropped"], "[%s] coverage: %d segments dropped, the case needs %d" % (name, k, expect["dropped"])
    if expect.get("exact"):
        assert (A["lo"] == A["hi"]).all() and A["total_lo"] == A["total_hi"], "[%s] coverage: the integers are not exact" % name
    if "peak_value" in expect:
        assert A["lo"].max() == expect["peak_value"], "[%s] coverage: the strongest cell holds %d, not %d" % (name, A["lo"].max(), expect["peak_value"])
    if "tie" in expect:
        k = int((A["lo"] == A["lo"].max()).sum())
        assert k >= expect["tie"], "[%s] coverage: %d cells hold the maximum, the case needs %d" % (name, k, expect["tie"])
    assert len(E.peak_candidates(A)) == 1 or not expect.get("exact"), "[%s] coverage: exact integers leave one peak" % name
    return A["share"]


def run_accumulator_case(name, vanishing_point):
    """vanishing_point(segments, d) -> (vp, accumulator).  -> the cell the returned point stands for"""
    segs, d, _ = ACCUMULATOR_CASES[name]
    _, A = diamond(name)
    vp, acc = vanishing_point(segs, d)
    E.check_accumulator(name, acc, A)
    cell = E.check_vanishing_point(name, vp, A, segs)
    assert cell == ACCUMULATOR_CASES[name][2].get("cell", cell), "[%s] peak: cell %d" % (name, cell)
    return cell


# ---- diamond space: the estimator (lr_estimate_line_pencils_cht) ------------------------------------------------------------
# name -> (segments, d, max_models, what the case asserts).  The seeds are those at which peel_chain's verdicts leave no
# line inside a band in any round (the RANSAC_CASES discipline).
def _cht_peel():
    out = {}
    three = pencils((300, 200, 150), 400, 1)
    for mm in (0, 1, 2, 3, 4):
        out["three pencils and clutter, max_models %d" % mm] = (three, 128, mm, dict(complete=True, rounds=mm))
    # round 0 removes more than 512 lines: their votes are taken back by two workgroups
    out["a pencil of 700"] = (pencils((700, 0, 0), 300, 1), 128, 4, dict(complete=True, removed0=513))
    # forty lines of one pencil and a stray one: after round 0 a single line is left, and the peeling ends
    out["forty and a stray"] = (pencils((40, 0, 0), 1, 2), 128, 4, dict(complete=True, rounds=1))
    return out


CHT_PEEL_CASES = _cht_peel()


def diamond_share(segs, d):
    """the ambiguous share of the votes of all the lines, from the second source alone"""
    return E.Diamond(N.Model(N._xy(N.normalised_f32(segs))), d).intervals()["share"]


def run_cht_peel_case(name, estimate):
    """estimate(segments, max_models, d) -> (records with group ids, refit models, winning cells, votes cast or None)"""
    segs, d, mm, expect = CHT_PEEL_CASES[name]
    share = diamond_share(segs, d)  # on the second source alone, before any result is looked at
    assert share <= E.AMBIGUITY_CAP, "[%s] cap: %.4f of the votes are ambiguous" % (name, share)
    got, models, cells, votes = estimate(segs, mm, d)
    assert len(got) == len(segs), "[%s] %d lines came back for %d" % (name, len(got), len(segs))
    chain = E.cht_chain(name, segs, d, mm, cells)
    counts = N.check_groups(name, got["group_id"], chain)
    E.check_models(name, models, chain)
    if votes is not None and chain["complete"]:
        assert chain["votes_lo"] <= votes <= chain["votes_hi"], "[%s] votes: %d cast and taken back, outside [%d, %d]" % (name, votes, chain["votes_lo"], chain["votes_hi"])
    counts.update(grouped=chain["grouped"], garbage=chain["garbage"], reason=chain["reason"], share=chain["share"])
    if expect.get("complete"):
        assert chain["complete"], "[%s] coverage: the second source stops early (%s)" % (name, chain["reason"])
    if "rounds" in expect:
        assert chain["rounds"] >= expect["rounds"], "[%s] coverage: %d rounds decided (%s), the case needs %d" % (name, chain["rounds"], chain["reason"], expect["rounds"])
    if "removed0" in expect:
        assert len(chain["removed"][0]) >= expect["removed0"], "[%s] coverage: round 0 removes %d lines, the case needs %d" % (name, len(chain["removed"][0]), expect["removed0"])
    return counts


# ---- Hough weights (lr_ht_weights) ------------------------------------------------------------------------------------------
# name -> (normalised fp32 records, indices, what the case asserts of itself).  Every case has exactly one candidate peak.
def _normalised(p1, p2):
    """records of coordinates that are given in normalised units already, as the fp32 numbers the entry point is handed"""
    return records(np.asarray(p1, np.float32).astype(np.float64), np.asarray(p2, np.float32).astype(np.float64))


def _pencil_norm(vp, n, clutter, seed):
    """n segments towards the point vp (normalised units) and `clutter` others, in random order"""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-0.4, 0.4, (n + clutter, 2))
    to = np.asarray(vp, np.float64) - c
    ang = np.where(np.arange(n + clutter) < n, np.arctan2(to[:, 1], to[:, 0]), rng.uniform(0, np.pi, n + clutter))
    dd = np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0.03, 0.1, n + clutter)[:, None]
    order = rng.permutation(n + clutter)
    return (c - dd)[order], (c + dd)[order]


def _tie():
    """Three segments parallel to the axes, so that their fp32 lengths are exact: 0 horizontal at y = 3/16, 1 and 2 vertical at
    x = 5/16 and -5/16.  The pairs {0, 1} and {0, 2} vote for two cells of one accumulator column v, {1, 2} (parallel: an exact
    ideal point) for the rim.  With c01 and c02 draws of the two pairs among the 20 000, the lengths are set so that the votes
    are v01 = c02 K and v02 = c01 K units of 2^-20: both cells hold c01 c02 K exactly, and the lower u, that of {0, 2}, is first
    in column-major order."""
    a, b = E.vote_pairs(3)
    c01, c02 = int(((a + b == 1) & (a != b)).sum()), int(((a + b == 2) & (a != b)).sum())
    K = (5 << 18) // c02  # v01 about 1.25 x 2^20
    l0 = 943718 / 1048576.0
    l1, l2 = c02 * K / 1048576.0 - l0, c01 * K / 1048576.0 - l0
    p1 = [[-l0 / 2, 0.1875], [0.3125, -l1 / 2], [-0.3125, -l2 / 2]]
    p2 = [[l0 / 2, 0.1875], [0.3125, l1 / 2], [-0.3125, l2 / 2]]
    return _normalised(p1, p2), c01 * c02 * K


def _hough():
    out = {}
    for n, seed in [(2, 2), (3, 3), (63, 4), (64, 5), (65, 6), (1000, 7)]:
        out["%d lines" % n] = (N.normalised_f32(segments(n, seed)), np.arange(n, dtype=np.int32), {})
    # a strict subset of the table, as in a later peeling round
    out["every third of 1000"] = (N.normalised_f32(segments(1000, 7)), np.arange(0, 1000, 3, dtype=np.int32), {})
    # a pencil towards (21, 21): the unit vector of its point is 0.9994 (cos 45, sin 45, .): cell i = j = round(21.9) = 22, and
    # 22^2 + 22^2 = 968 > 31^2: the peak point is beyond the rim and the normalising branch runs (its z is the root of 0 give
    # or take an ulp: a small number, or NaN and every weight with it -- check_weights takes either; today's arithmetic gives
    # numbers for this pencil, and the case says so, so that a silent change of the outcome shows)
    out["peak on the rim"] = (_normalised(*_pencil_norm((21.0, 21.0), 80, 20, 8)), np.arange(100, dtype=np.int32), dict(rim=True, all_nan=False))
    # a pencil towards (0.01, 0.005), inside the middle cell, whose point is p = (0, 0, 1) exactly; its first line has its
    # anchor there: 0 / 0 (the pencil's own point is a little off, so that PROSAC's hypotheses see that line like any other)
    p1, p2 = _pencil_norm((0.01, 0.005), 80, 20, 9)
    p1[0], p2[0] = (-0.1, -0.05), (0.1, 0.05)
    out["peak in the centre, an anchor on it"] = (_normalised(p1, p2), np.arange(100, dtype=np.int32), dict(position=32 * 65 + 32, undecided=1))
    tie, value = _tie()
    out["two cells tie"] = (tie, np.arange(3, dtype=np.int32), dict(tie=value))
    # no pair votes: every cross product is an exact zero.  The all-zero accumulator's first cell is (0, 0), its point
    # (-32, -32) / 31 beyond the rim: normalised, an ideal point give or take the root of an ulp
    out["1 line"] = (N.normalised_f32(segments(1, 1)), np.arange(1, dtype=np.int32), dict(no_vote=True, position=0))
    out["one line five times"] = (N.normalised_f32(np.tile(segments(3, 3)[:1], 5)), np.arange(5, dtype=np.int32), dict(no_vote=True, position=0))
    return out


HT_CASES = _hough()


@functools.lru_cache(maxsize=None)
def hough(name):
    norm, idx, _ = HT_CASES[name]
    return E.ht_accumulator(norm, idx)


def check_hough_case(name):
    """what the case asserts of itself, on the second source alone -> the one candidate's position (v 65 + u)"""
    _, idx, expect = HT_CASES[name]
    H = hough(name)
    cand = E.peak_candidates(H)
    assert len(cand) == 1, "[%s] coverage: %d candidate peaks" % (name, len(cand))
    assert H["open"] <= E.AMBIGUITY_CAP * E.HT_PAIRS, "[%s] cap: %d of the pairs are open" % (name, H["open"])
    u, v = cand[0] % 65 - 32, cand[0] // 65 - 32
    if expect.get("rim"):
        assert u * u + v * v > 31 * 31, "[%s] coverage: the peak (%d, %d) is inside the rim" % (name, u, v)
    if "position" in expect:
        assert cand[0] == expect["position"], "[%s] coverage: the peak is at %d" % (name, cand[0])
    if expect.get("no_vote"):
        assert H["cast"] == 0 and H["open"] == 0 and not H["hi"].any(), "[%s] coverage: a pair votes" % name
    if "tie" in expect:
        top = np.nonzero((H["lo"] == expect["tie"]) & (H["hi"] == expect["tie"]))[0]
        assert len(top) == 2 and H["hi"].max() == expect["tie"] and cand[0] == top[0], "[%s] coverage: no exact tie of two cells" % name
    _, dw = E.ht_weights(H, cand[0])
    assert int((~np.isfinite(dw)).sum()) == expect.get("undecided", 0), "[%s] coverage: %d weights are undecided" % (name, (~np.isfinite(dw)).sum())
    return cand[0]


def run_hough_case(name, weights):
    """weights(normalised records, indices) -> the weights.  -> (position of the peak they belong to, the weights)"""
    norm, idx, expect = HT_CASES[name]
    w = weights(norm, idx)
    position = E.check_weights(name, w, hough(name))
    if "all_nan" in expect:
        assert bool(np.isnan(w).all()) == expect["all_nan"], "[%s] rim: %d of %d weights are NaN, the case records %s" % (
            name, np.isnan(w).sum(), len(w), "all" if expect["all_nan"] else "none")
    if expect.get("no_vote"):
        assert np.isfinite(w).all() and (w >= 0).all() and (w <= 1).all(), "[%s] no vote: the weights %r are not finite numbers in [0, 1]" % (name, w)
    return position, w


# ---- PROSAC (lr_prosac_solve, lr_estimate_line_pencils_prosac) ---------------------------------------------------------------
# name -> (normalised fp32 records, indices, T_N, seed, round, what the case asserts).  Line counts are small where T_N is
# large and the other way round: the replay is a Python loop.  Every case is decided at least up to its best iteration.
TOL = Gc.TOL


def _prosac():
    out = {}
    three = N.normalised_f32(segments(300, 101))
    # 9 iterations; then a first chunk that is CUT: the first new bests shrink n_star to the pencil's 70 to 90 lines, the growth
    # of the true state stops there after 163 (653) iterations while the chunk was drawn growing on, and the rest runs in one
    # chunk of a later size
    for T_N, seed in [(-1, 1), (2047, 2), (2048, 3), (2049, 12), (10241, 5)]:
        out["300 lines, T_N %d" % T_N] = (three, np.arange(300, dtype=np.int32), T_N, seed, 0, dict(complete=True, cut=T_N > 0))
    # under half of the lines on any pencil: I_N_best stays below I_N_min and the loop runs all 50 000 iterations.  The first
    # chunk runs to its end (n reaches n_star = 69 only at iteration 2649), the 8192-chunk is cut there, and what is left is
    # one chunk of 47 351 drawn with room for 65 536: eight hypotheses per wavefront
    out["300 lines, T_N 50000"] = (N.normalised_f32(segments(300, 109, on=(0.15, 0.15, 0.1))), np.arange(300, dtype=np.int32), 50000, 9, 0,
                                   dict(complete=True, iterations=50000, wide=True, chunks=[2048, 601, 47351]))
    # The chunk boundaries themselves need a replay that is never cut: sixteen lines in general position under a tolerance of
    # 0.2 degrees, where every hypothesis is supported by its own two lines and no third.  The first valid samples
    # are the only new bests (two or three inliers pass no Imin), n_star stays 16, and I_N_best = 2 < I_N_min = 8 keeps the loop running to T_N: the
    # chunks are the schedule itself.  T_N one short of, at and one past the end of the 2048-chunk; at and one past the ends
    # of the 8192-, the 32 768- and the 65 536-chunk (a chunk that ends at T_N has no successor; one past it, a successor of
    # one sample that is used).
    general = N.normalised_f32(segments(16, 208, on=(0.0, 0.0, 0.0)))
    narrow = np.float32(1.0 - np.cos(np.deg2rad(0.2)))
    for T_N, chunks in [(2047, [2047]), (2048, [2048]), (2049, [2048, 1]), (10240, [2048, 8192]), (10241, [2048, 8192, 1]),
                        (43008, [2048, 8192, 32768]), (43009, [2048, 8192, 32768, 1]), (108544, [2048, 8192, 32768, 65536]),
                        (108545, [2048, 8192, 32768, 65536, 1])]:
        out["16 lines in general position, T_N %d" % T_N] = (general, np.arange(16, dtype=np.int32), T_N, 31, 0,
                                                             dict(complete=True, tol=narrow, chunks=chunks, iterations=T_N, uncut=True))
    out["2 lines"] = (N.normalised_f32(segments(2, 106)), np.arange(2, dtype=np.int32), 100, 6, 0, dict(complete=True))
    out["3 lines"] = (N.normalised_f32(segments(3, 107)), np.arange(3, dtype=np.int32), 100, 7, 1, dict(complete=True))
    # the first line of a pencil six times: the copies share the top weights, and the first samples are pairs of them
    base = segments(200, 110, on=(0.5, 0.1, 0.1), noise=0.0005)
    first = int(np.argmax(N.Model(N._xy(N.normalised_f32(base))).length))
    out["six copies on top"] = (N.normalised_f32(np.concatenate([np.tile(base[first:first + 1], 5), base])), np.arange(205, dtype=np.int32), 500, 8, 0,
                                dict(failed_first=1))
    for n in (4095, 4096):  # the line count from which a new best without a flag row is counted on the GPU
        out["%d lines" % n] = (N.normalised_f32(segments(n, 111)), np.arange(n, dtype=np.int32), 300, 10, 0, dict(complete=True))
    # a line whose anchor is the Hough peak has the weight 0 / 0: NaN sorts last, stably, in the library, the oracle and here
    norm, idx, _ = HT_CASES["peak in the centre, an anchor on it"]
    out["a NaN weight"] = (norm, idx, 500, 13, 0, dict(nan_weights=1))
    out["every other of 600, round 2"] = (N.normalised_f32(segments(600, 112)), np.arange(0, 600, 2, dtype=np.int32), 1500, (1 << 40) + 11, 2, dict(complete=True))
    return out


PROSAC_CASES = _prosac()


def run_prosac_case(name, weights, solve):
    """weights(norm, idx) -> the Hough weights; solve(norm, idx, tol, T_N, seed, rnd) -> dict(h, iterations, n_star, best_iter,
    I_N_best).  -> counts and the paths the case reaches"""
    norm, idx, T_N, seed, rnd, expect = PROSAC_CASES[name]
    w = weights(norm, idx)
    assert int(np.isnan(w).sum()) == expect.get("nan_weights", 0), "[%s] coverage: %d NaN weights" % (name, np.isnan(w).sum())
    tol = expect.get("tol", TOL)
    R = E.prosac_replay(norm, idx, float(tol), T_N, seed, rnd, w)
    res = solve(norm, idx, tol, T_N, seed, rnd)
    counts = E.check_prosac(name, res, R)
    paths = E.prosac_paths(R, seed, rnd)
    counts.update(complete=R["complete"], reason=R["reason"], best_iter=R["best_iter"], iterations=R["iterations"], new_bests=len(R["events"]),
                  chunks=paths["chunks"], wide=paths["wide"], most_in_a_chunk=paths["new_bests"], beyond_cap=paths["beyond_cap"], cuts=paths["cuts"])
    assert counts["h_checked"], "[%s] coverage: the best hypothesis has lines inside the band (%s)" % (name, R["reason"])
    if expect.get("complete"):
        assert R["complete"], "[%s] coverage: the replay stops undecided (%s)" % (name, R["reason"])
    if "iterations" in expect:
        assert R["iterations"] == expect["iterations"], "[%s] coverage: %d iterations" % (name, R["iterations"])
    if "chunks" in expect:  # the chunks as far as they were used; the generated lengths where the schedule was never cut
        assert paths["chunks"] == expect["chunks"], "[%s] coverage: chunks %r, the case needs %r" % (name, paths["chunks"], expect["chunks"])
        assert paths["cuts"] > 0 or paths["drawn"] == expect["chunks"], "[%s] coverage: generated %r" % (name, paths["drawn"])
    if expect.get("uncut"):
        assert paths["cuts"] == 0 and R["n_star"] == len(idx), "[%s] coverage: %d cuts, n_star %d" % (name, paths["cuts"], R["n_star"])
    if expect.get("cut"):
        assert paths["cuts"] >= 1 and paths["chunks"][0] < 2048, "[%s] coverage: the first chunk is not cut (%r)" % (name, paths["chunks"])
    if expect.get("wide"):
        assert paths["wide"], "[%s] coverage: no chunk of 16 384 iterations (%r)" % (name, paths["drawn"])
    if "failed_first" in expect:
        k = sum(c[0] < 0 for c in R["counts"][:3])
        assert k >= expect["failed_first"], "[%s] coverage: %d of the first samples fail the check" % (name, k)
    return counts


# name -> (segments, T_N, seed, max_models, what the case asserts)
PROSAC_PEEL_CASES = {
    "three pencils, T_N 1500": (pencils((120, 90, 60), 130, 2), 1500, 21, 4, dict(rounds=4, complete=True)),
    "three pencils, T_N -1": (pencils((120, 90, 60), 130, 5), -1, 22, 4, dict(rounds=4, complete=True)),
    "max_models 1": (pencils((120, 90, 60), 130, 2), 600, 23, 1, dict(rounds=1, complete=True)),
}


def prosac_chain(name, segs, T_N, seed, max_models, weights, inlier_deg=2.0, garbage_deg=4.0):
    """estimate_line_pencils_prosac through peel_chain's verdicts: the hypothesis of round k is the best sample of the replay
    over the lines still in the game, fed the implementation's weights of those lines"""
    norm = N.normalised_f32(segs)

    def propose(M, obs, k, tol, dtol):
        R = E.prosac_replay(norm, obs, tol, T_N, seed, k, weights(norm, obs.astype(np.int32)), dtol=dtol, model=M)
        if not R["complete"]:
            return 0, None, None, "round %d: the replay stops undecided (%s)" % (k, R["reason"])
        if R["best_iter"] < 0:
            return -1, None, None, ""
        a, b = R["best_pair"]
        p, dp, _ = N.hypotheses(M, np.array([a]), np.array([b]))
        return R["best_iter"], p[0], dp[0], ""

    return N.peel_chain(segs, 0, 0, max_models, inlier_deg, garbage_deg, propose=propose)


def run_prosac_peel_case(name, weights, estimate):
    """estimate(segments, max_models, T_N, seed) -> records with group ids"""
    segs, T_N, seed, mm, expect = PROSAC_PEEL_CASES[name]
    chain = prosac_chain(name, segs, T_N, seed, mm, weights)
    got = estimate(segs, mm, T_N, seed)
    counts = N.check_groups(name, got["group_id"], chain)
    counts.update(grouped=chain["grouped"], reason=chain["reason"])
    assert chain["rounds"] >= expect["rounds"], "[%s] coverage: %d rounds decided (%s), the case needs %d" % (name, chain["rounds"], chain["reason"], expect["rounds"])
    assert chain["complete"] or not expect.get("complete"), "[%s] coverage: the second source stops early (%s)" % (name, chain["reason"])
    return counts


# ---- refine: the pair kernel (lr_refine_lines from 2048 segments up) ---------------------------------------------------
# A designed block of seven segments in integer coordinates (s along a direction, m across it), so that float64 decides
# every pair far from a gate (cos 0.99, offset 0.02 of the longer one's length, overlap -0.5 .. 1.5):
#   A (0, 0)-(100, 0)      B (110, 0)-(160, 0)   collinear, B's end points at 1.1 and 1.6 of A: merged
#   C (400, 0)-(450, 0)    collinear and far (4.0 of A, 5.8 of B): not merged
#   D (0, 5)-(100, 5)      parallel at 0.05 of its length: not merged
#   E (30, 1)-(40, 1)      0.01 in A's frame (merged) -- it would be 0.1 in its own
#   F (200, 10)-(260, 20)  turned by atan(1 / 6): cos 0.9864, fails the direction gate
#   G (200, -30)-(280, -20) turned by atan(1 / 8): cos 0.9923 passes it, the offset (0.3) does not
# Blocks repeat on a staggered grid (columns 500 apart, every other one shifted by 50 across, rows 100 apart: a collinear
# neighbour is 1000 away), 152 of them along x and 152 transposed, along y.  Cutting the list after n segments cuts a block.
_BLOCK = [(0, 0, 100, 0), (110, 0, 160, 0), (400, 0, 450, 0), (0, 5, 100, 5), (30, 1, 40, 1), (200, 10, 260, 20), (200, -30, 280, -20)]
REFINE_SIZES = (2047, 2048, 2049, 2111, 2112, 2113)  # the host / GPU threshold; 33 tiles of 64 less one, exact, and one more


def _refine_lines(n_blocks=152):
    out = []
    for k in range(n_blocks):
        col, row = k % 8, k // 8
        ox, oy = 500 * col, 40 + 100 * row + 50 * (col % 2)
        out += [(ox + a, oy + b, ox + c, oy + d) for a, b, c, d in _BLOCK]
    out += [(4100 + y1, x1, 4100 + y2, x2) for x1, y1, x2, y2 in out]
    lines = rows(*out)
    lines["weight"] = 0.25 + 0.001 * (np.arange(len(lines)) % 7)
    return lines


REFINE_LINES = _refine_lines()
# 300 segments (k, 3900)-(1000 + k, 3900): every pair of them is an edge, 44 850 > 16 x 2048: the first launch's edge list
# overflows, and the kernel runs again with room for the count it reported
_STACK = rows(*[(k, 3900, 1000 + k, 3900) for k in range(300)])
REFINE_OVERFLOW = np.concatenate([REFINE_LINES[:1000], _STACK, REFINE_LINES[1000:1748]])
assert 300 * 299 // 2 > 16 * len(REFINE_OVERFLOW) == 32768


@functools.lru_cache(maxsize=None)
def refine_reference(n):
    """numpy_ref.refine of the first n designed segments (n = 0: the overflow input) -> (merged rows, closest, the input)"""
    import numpy_ref

    lines = REFINE_OVERFLOW if n == 0 else REFINE_LINES[:n]
    ref, closest = numpy_ref.refine(lines)
    return ref, closest, lines


def check_refine(name, got, ref):
    """the merged rows against numpy_ref.refine's, within the bounds test_second_source_cpu.py holds the host loop to: end
    points 5e-3 px, weight 1e-4 relative, error 2e-3"""
    assert len(got) == len(ref), "[%s] rows: %d segments come back, the second source merges to %d" % (name, len(got), len(ref))
    g = np.stack([got["x1"], got["y1"], got["x2"], got["y2"]], 1).astype(np.float64)
    used = np.zeros(len(ref), bool)
    for k in range(len(g)):
        dist = np.minimum(np.abs(ref[:, :4] - g[k]).max(1), np.abs(ref[:, [2, 3, 0, 1]] - g[k]).max(1))
        dist[used] = np.inf
        j = int(np.argmin(dist))
        assert dist[j] < 5e-3, "[%s] row %d: %r has no twin (nearest %r, %.3g px)" % (name, k, got[k], ref[j], dist[j])
        used[j] = True
        assert abs(float(got["weight"][k]) - ref[j, 4]) <= 1e-4 * max(1.0, abs(ref[j, 4])), "[%s] row %d: weight %r, not %r" % (name, k, got["weight"][k], ref[j, 4])
        assert abs(float(got["err"][k]) - ref[j, 5]) <= 2e-3, "[%s] row %d: error %r, not %r" % (name, k, got["err"][k], ref[j, 5])
