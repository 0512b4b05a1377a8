"""The opt-in estimators and the refine pairs (diamond-space accumulator and its peeling, Hough weights, PROSAC, the pair
test of refine) against a second, independent source: tests/numpy_estimators_ref.py, float64 NumPy and Python integers
written from the reference's text and the published diamond-space mapping, which brackets every fp32 decision instead of
reproducing it (and tests/numpy_ref.refine for the pairs).  Here the caps and the "one candidate" / "decided" conditions of
tests/estimator_cases.py are asserted on the second source alone, its checks are applied to the oracle over every case,
and every check is shown to fire on the smallest wrong result a wrong kernel would give.  CPU only;
tests/test_gpu_estimators_second_source.py holds the kernels to the same rules."""
import os
import subprocess

import numpy as np
import pytest

import estimator_cases as Cs
import numpy_estimators_ref as E
import numpy_grouping_ref as N
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_cht(segs, max_models, d):
    return O.estimate_line_pencils_cht(segs, max_models=max_models, d=d) + (None,)


def oracle_prosac_peel(segs, max_models, T_N, seed):
    return O.estimate_line_pencils_prosac(segs, max_models=max_models, T_N=T_N, seed=seed)


# ---- diamond space ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.ACCUMULATOR_CASES))
def test_oracle_accumulator_against_the_second_source(name):
    share = Cs.check_accumulator_case(name)  # the cap and the case's own coverage, before any result is looked at
    cell = Cs.run_accumulator_case(name, O.cht_vanishing_point)
    print(name, "ambiguous share %.4f of %.2f, peak cell %d" % (share, E.AMBIGUITY_CAP, cell))


@pytest.mark.parametrize("name", list(Cs.CHT_PEEL_CASES))
def test_oracle_diamond_peeling_against_the_second_source(name):
    print(name, Cs.run_cht_peel_case(name, oracle_cht))


def test_an_all_zero_accumulator_answers_cell_zero():
    """no proper line drops all three of its segments (estimator_cases.py says why), so the all-zero accumulator is stated on
    the intervals themselves: cell 0 is the peak, and no other cell passes"""
    A = dict(lo=np.zeros(64, np.int64), hi=np.zeros(64, np.int64), d=8)
    E.check_peak("zero", 0, A)
    assert E.peak_candidates(A) == [0]
    with pytest.raises(AssertionError, match=r"\[zero\] peak tie"):
        E.check_peak("zero", 1, A)


def _segment_cells(name, line, seg):
    """the cells one polyline segment of one line surely votes for, and the line's vote"""
    segs, d, _ = Cs.ACCUMULATOR_CASES[name]
    M = N.Model(N._xy(N.normalised_f32(segs)))
    P = E.polyline(M.h[line], M.dh[line])
    ends = [E._cells_of(*P[seg][0], d), E._cells_of(*P[seg][1], d), E._cells_of(*P[seg + 1][0], d), E._cells_of(*P[seg + 1][1], d)]
    assert all(len(e) == 1 for e in ends)
    cells, _ = E.rasterise(*[e[0] for e in ends], d)
    return cells, E.vote_of(M.length[line])[0]


def test_the_accumulator_checks_fail_on_a_wrong_result():
    name = "5 lines"
    segs, d, _ = Cs.ACCUMULATOR_CASES[name]
    _, A = Cs.diamond(name)
    vp, acc = O.cht_vanishing_point(segs, d)
    E.check_accumulator(name, acc, A)
    sure = np.nonzero((A["lo"] == A["hi"]) & (A["lo"] > 0))[0]
    c = int(next(c for c in sure if A["hi"][c + 1] == 0))  # a vote moved to the neighbouring, empty cell
    vote = int(A["lo"][c])
    moved = acc.copy().reshape(-1)
    moved[c] -= vote
    moved[c + 1] += vote
    with pytest.raises(AssertionError, match=r"\[%s\] cell interval" % name):
        E.check_accumulator(name, moved.reshape(d, d), A)
    cells, vote = _segment_cells(name, 0, 1)  # one segment's votes counted twice
    twice = acc.copy().reshape(-1)
    np.add.at(twice, cells, np.uint64(vote))
    with pytest.raises(AssertionError, match=r"\[%s\] cell interval" % name):
        E.check_accumulator(name, twice.reshape(d, d), A)
    # an ambiguous vote counted in both of its cells: every cell inside its interval, the sum is not
    D, _ = Cs.diamond(name)
    both = A["lo"].copy()
    for i in range(len(segs)):
        both[D.of(i)["maybe"][0]] += D.of(i)["maybe"][1] * D.of(i)["weight"][0]
    assert (both <= A["hi"]).all() and both.sum() > A["total_hi"]
    with pytest.raises(AssertionError, match=r"\[%s\] total" % name):
        E.check_accumulator(name, both.reshape(d, d), A)

    name = "128 and 65 steps"  # a polyline cut off after a wavefront's 64 lanes: the 65th vote of two segments is missing
    segs, d, _ = Cs.ACCUMULATOR_CASES[name]
    _, A = Cs.diamond(name)
    vp, acc = O.cht_vanishing_point(segs, d)
    E.check_accumulator(name, acc, A)
    cut = acc.copy()
    for seg in (1, 2):
        cells, vote = _segment_cells(name, 0, seg)
        assert len(cells) == 65
        cut.reshape(-1)[cells[64]] -= np.uint64(vote)
    with pytest.raises(AssertionError, match=r"\[%s\] cell interval" % name):
        E.check_accumulator(name, cut, A)

    name = "mirror images"  # the peak moved to the second of the tied cells
    _, A = Cs.diamond(name)
    tied = np.nonzero(A["lo"] == A["lo"].max())[0]
    E.check_peak(name, tied[0], A)
    with pytest.raises(AssertionError, match=r"\[%s\] peak tie" % name):
        E.check_peak(name, tied[1], A)
    with pytest.raises(AssertionError, match=r"\[%s\] peak beaten" % name):
        E.check_peak(name, int(np.nonzero(A["hi"] < A["lo"].max())[0][0]), A)
    segs, d, _ = Cs.ACCUMULATOR_CASES[name]
    vp, _ = O.cht_vanishing_point(segs, d)
    with pytest.raises(AssertionError, match=r"\[%s\] vanishing point" % name):
        E.check_vanishing_point(name, vp * np.float32(1.0001), A, segs)

    name = "50 000 diagonals"  # the high word of a cell lost
    segs, d, _ = Cs.ACCUMULATOR_CASES[name]
    _, A = Cs.diamond(name)
    vp, acc = O.cht_vanishing_point(segs, d)
    assert int(acc.max()) > 1 << 32
    with pytest.raises(AssertionError, match=r"\[%s\] cell interval" % name):
        E.check_accumulator(name, acc & np.uint64(0xFFFFFFFF), A)


def test_the_peeling_checks_fail_on_a_wrong_result():
    name = "a pencil of 700"
    segs, d, mm, _ = Cs.CHT_PEEL_CASES[name]
    got, models, cells, _ = oracle_cht(segs, mm, d)
    chain = E.cht_chain(name, segs, d, mm, cells)
    N.check_groups(name, got["group_id"], chain)
    ids = got["group_id"].copy()
    ids[np.nonzero(ids == 0)[0][0]] = 1  # one line's group changed
    with pytest.raises(AssertionError, match=r"\[%s\] group id" % name):
        N.check_groups(name, ids, chain)
    with pytest.raises(AssertionError, match=r"\[%s, round 0\] peak beaten" % name):
        E.cht_chain(name, segs, d, mm, [cells[0] + 5] + list(cells[1:]))
    with pytest.raises(AssertionError, match=r"\[%s\] rounds" % name):
        E.cht_chain(name, segs, d, mm, cells[:-1])
    wrong = models.copy()
    wrong[1] = wrong[1] + np.float32(1e-3) * np.abs(wrong[1]).max()
    with pytest.raises(AssertionError, match=r"\[%s\] refit: round 1" % name):
        E.check_models(name, wrong, chain)


# ---- Hough weights ----------------------------------------------------------------------------------------------------------
def test_the_generator_and_the_distribution_are_the_c_plus_plus_librarys(tmp_path):
    """mt19937 by the standard's known answer, and the vote pairs against a stand-alone program that draws them with the
    host compiler's own <random>"""
    assert E.mt19937(10000)[-1] == 4123659995
    exe = str(tmp_path / "ht_vote_pairs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cxx", "ht_vote_pairs.cpp"), "-o", exe])
    sizes = [1, 2, 3, 1000, 20000]
    out = subprocess.run([exe, str(E.HT_PAIRS)] + [str(n) for n in sizes], text=True, capture_output=True, check=True).stdout.split("\n")
    assert out[0] == "4123659995"
    at = 1
    for n in sizes:
        assert out[at] == "n %d" % n
        theirs = np.array([ln.split() for ln in out[at + 1:at + 1 + E.HT_PAIRS]], np.int64)
        a, b = E.vote_pairs(n)
        assert (theirs[:, 0] == a).all() and (theirs[:, 1] == b).all(), n
        at += 1 + E.HT_PAIRS


@pytest.mark.parametrize("name", list(Cs.HT_CASES))
def test_oracle_hough_weights_against_the_second_source(name):
    want = Cs.check_hough_case(name)  # exactly one candidate, and the case's own coverage, on the second source alone
    position, w = Cs.run_hough_case(name, O.get_weights_fixed)
    assert position == want
    print(name, "peak (u %d, v %d), %d open pairs" % (position % 65, position // 65, Cs.hough(name)["open"]))


def test_no_vote_never_hands_the_sort_a_nan():
    """the all-zero accumulator's point is beyond the rim; the root of its radicand, 0 give or take an ulp, was NaN where the
    ulp fell below zero, and every weight with it.  With the radicand of the accumulator nobody voted for taken as zero, the
    weights are numbers and the PROSAC solve that sorts them ends with nothing found -- for the copies of one line,
    whatever their direction"""
    for k in range(24):
        a = np.pi * k / 24
        p = np.array([[0.3 * np.cos(a) + 0.1, 0.3 * np.sin(a) - 0.05]])
        norm = Cs._normalised(np.tile(-p, (4, 1)), np.tile(p, (4, 1)))
        idx = np.arange(4, dtype=np.int32)
        w = O.get_weights_fixed(norm, idx)
        assert np.isfinite(w).all() and (w >= 0).all() and (w <= 1).all(), (k, w)
        E.check_weights("copies at %d/24 pi" % k, w, E.ht_accumulator(norm, idx))
        res = O.prosac_solve(norm, idx, Cs.TOL, 50, 1, 0)
        assert res["best_iter"] == -1 and res["I_N_best"] == 0 and np.isfinite(res["h"]).all()


def test_the_weight_checks_fail_on_a_wrong_result():
    name = "1000 lines"
    norm, idx, _ = Cs.HT_CASES[name]
    H = Cs.hough(name)
    w = O.get_weights_fixed(norm, idx)
    E.check_weights(name, w, H)
    off = w.copy()
    k = int(np.argmax((w > 0.2) & (w < 0.8)))
    off[k] += np.float32(1e-3)  # one weight moved by 1e-3
    with pytest.raises(AssertionError, match=r"\[%s\] weight: line %d" % (name, k)):
        E.check_weights(name, off, H)
    with pytest.raises(AssertionError, match=r"\[%s\] weight" % name):
        E.check_weights(name, np.where(np.arange(len(w)) == 5, np.float32(np.nan), w), H)
    name = "two cells tie"  # the weights against the second of the tied cells
    norm, idx, expect = Cs.HT_CASES[name]
    H = Cs.hough(name)
    tied = np.nonzero(H["lo"] == expect["tie"])[0]
    second, _ = E.ht_weights(H, int(tied[1]))
    with pytest.raises(AssertionError, match=r"\[%s\] weight" % name):
        E.check_weights(name, second.astype(np.float32), H)


# ---- PROSAC -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.PROSAC_CASES))
def test_oracle_prosac_against_the_second_source(name):
    print(name, Cs.run_prosac_case(name, O.get_weights_fixed, O.prosac_solve))


@pytest.mark.parametrize("name", list(Cs.PROSAC_PEEL_CASES))
def test_oracle_prosac_peeling_against_the_second_source(name):
    print(name, Cs.run_prosac_peel_case(name, O.get_weights_fixed, oracle_prosac_peel))


def test_the_prosac_checks_fail_on_a_wrong_result():
    name = "300 lines, T_N 2049"
    norm, idx, T_N, seed, rnd, _ = Cs.PROSAC_CASES[name]
    R = E.prosac_replay(norm, idx, float(Cs.TOL), T_N, seed, rnd, O.get_weights_fixed(norm, idx))
    good = O.prosac_solve(norm, idx, Cs.TOL, T_N, seed, rnd)
    E.check_prosac(name, good, R)
    for key, wrong in [("best_iter", good["best_iter"] + 1), ("I_N_best", good["I_N_best"] - 1), ("iterations", good["iterations"] - 1),
                       ("n_star", good["n_star"] + 1), ("h", good["h"][[1, 0, 2]])]:
        with pytest.raises(AssertionError, match=r"\[%s\] %s" % (name, key)):
            E.check_prosac(name, dict(good, **{key: wrong}), R)
    name = "three pencils, T_N 1500"
    segs, T_N, seed, mm, _ = Cs.PROSAC_PEEL_CASES[name]
    chain = Cs.prosac_chain(name, segs, T_N, seed, mm, O.get_weights_fixed)
    ids = oracle_prosac_peel(segs, mm, T_N, seed)["group_id"].copy()
    N.check_groups(name, ids, chain)
    ids[np.nonzero(ids == 1)[0][0]] = -1
    with pytest.raises(AssertionError, match=r"\[%s\] group id" % name):
        N.check_groups(name, ids, chain)


# ---- refine ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0,) + Cs.REFINE_SIZES)
def test_oracle_refine_against_the_second_source(n):
    ref, closest, lines = Cs.refine_reference(n)
    assert closest > 1e-3, "a pair within %.1e of a gate: float64 does not decide it" % closest
    assert len(ref) < len(lines) - 500  # (the blocks do merge)
    Cs.check_refine("%d segments" % len(lines), O.refine_lines(lines), ref)


def test_the_refine_check_fails_on_a_dropped_edge():
    """the result a pair kernel that misses the edge (A, E) of the first block would lead to: E stays a segment of its own"""
    ref, _, lines = Cs.refine_reference(2048)
    apart = lines.copy()
    apart["y1"][4] += 3000.0
    apart["y2"][4] += 3000.0
    got = O.refine_lines(apart)
    moved = np.nonzero((got["x1"] == apart["x1"][4]) & (got["y1"] == apart["y1"][4]) & (got["x2"] == apart["x2"][4]) & (got["y2"] == apart["y2"][4]))[0]
    assert len(moved) == 1
    got[moved[0]] = O.refine_lines(lines[4:5])[0]
    with pytest.raises(AssertionError, match=r"\[edge\] rows"):
        Cs.check_refine("edge", got, ref)
    shifted = O.refine_lines(lines)
    shifted["x2"][0] += np.float32(0.01)
    with pytest.raises(AssertionError, match=r"\[edge\] row 0"):
        Cs.check_refine("edge", shifted, ref)
