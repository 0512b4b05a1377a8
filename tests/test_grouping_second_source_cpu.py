"""The vanishing-point grouping (A19-A22: sampling, RANSAC scoring, peeling) against a second, independent source:
tests/numpy_grouping_ref.py, a float64 NumPy restatement written from the reference's text that brackets every fp32
decision instead of reproducing it.  Here its checks are applied to the oracle, over every case of
tests/grouping_cases.py; the checks are shown to fire on wrong results; and the seeds of the random-size cases are proven
to leave nothing open.  CPU only; tests/test_gpu_grouping_second_source.py holds the kernels to the same rules."""
import numpy as np
import pytest

import grouping_cases as Cs
import numpy_grouping_ref as N
import oracle_lib as O


def oracle_solve(norm, idx, tol, n_iter, seed, rnd):
    return O.ransac_best(norm, idx, tol, n_iter, seed, rnd)


def oracle_estimate(segs, max_models, n_iter, seed):
    return O.estimate_line_pencils(segs, max_models=max_models, n_iter=n_iter, seed=seed)[0]


def test_sampling_rule():
    """the integer restatement, its array form and the oracle's sample_pair draw the same pairs"""
    for seed, rnd, n, n_iter in [(0, 0, 2, 50), (1, 3, 3, 600), ((1 << 40) + 5, 3, 64, 300), ((1 << 64) - 1, 4, 1025, 300), (7, 0, 130, 65569)]:
        a, b = N.sample_pairs(seed, rnd, n_iter, n)
        assert (a < b).all() and a.min() >= 0 and b.max() < n
        for it in list(range(min(n_iter, 300))) + [n_iter - 1]:
            assert N.sample_pair(seed, rnd, it, n) == (a[it], b[it]) == O.sample_pair(seed, rnd, it, n), (seed, rnd, it, n)


def test_normalisation_is_the_oracles():
    """normalised_f32 does the five fp32 operations of the text: the oracle's normalised records, bit for bit"""
    for name in ("1023 lines", "2 lines", "pencil and ten copies of a stray"):
        segs = Cs.PEEL_CASES[name][0]
        assert N.normalised_f32(segs).tobytes() == O.normalize_lines(segs)[0].tobytes(), name


@pytest.mark.parametrize("name", list(Cs.RANSAC_CASES))
def test_oracle_solve_against_the_second_source(name):
    counts = Cs.run_ransac_case(name, oracle_solve)
    print(name, counts)


@pytest.mark.parametrize("name", list(Cs.PEEL_CASES))
def test_oracle_peeling_against_the_second_source(name):
    counts = Cs.run_peel_case(name, oracle_estimate)
    print(name, counts)


def test_the_checks_fail_on_a_wrong_result():
    """each check fires on a result that is wrong, and names the case and the check"""
    name = "511 lines, 300 hypotheses"
    norm, idx, n_iter, seed, rnd, _ = Cs.RANSAC_CASES[name]
    S = Cs.ransac_intervals(name)
    good = oracle_solve(norm, idx, Cs.TOL, n_iter, seed, rnd)
    N.check_ransac(name, good, S)
    with pytest.raises(AssertionError, match=r"\[%s\] score interval" % name):
        N.check_ransac(name, dict(good, score=np.float32(good["score"]) * np.float32(1 + 2.0 ** -12)), S)
    worse = int(np.nonzero((S["valid"] == 1) & (S["hi"] < 0.5 * S["lo"][good["iter"]]) & (S["lo"] > 0))[0][0])
    with pytest.raises(AssertionError, match=r"\[%s\] surely better" % name):
        N.check_ransac(name, dict(iter=worse, score=np.float32(S["lo"][worse]), best_h=S["p"][worse].astype(np.float32)), S)
    with pytest.raises(AssertionError, match=r"\[%s\] hypothesis" % name):
        N.check_ransac(name, dict(good, best_h=good["best_h"][[1, 0, 2]]), S)
    with pytest.raises(AssertionError, match=r"\[%s\] surely better: nothing returned" % name):
        N.check_ransac(name, dict(iter=-1, score=0.0, best_h=np.zeros(3, np.float32)), S)

    name = "three lines, 600 hypotheses"
    norm, idx, n_iter, seed, rnd, _ = Cs.RANSAC_CASES[name]
    S = Cs.ransac_intervals(name)
    good = oracle_solve(norm, idx, Cs.TOL, n_iter, seed, rnd)
    later = int(np.nonzero(S["key"] == S["key"][good["iter"]])[0][1])
    with pytest.raises(AssertionError, match=r"\[%s\] same pair earlier" % name):
        N.check_ransac(name, dict(good, iter=later), S)

    name = "65 lines, 513 hypotheses"  # eleven later iterations with the winner's inliers, of other pairs
    norm, idx, n_iter, seed, rnd, _ = Cs.RANSAC_CASES[name]
    S = Cs.ransac_intervals(name)
    good = oracle_solve(norm, idx, Cs.TOL, n_iter, seed, rnd)
    later = int(np.nonzero((S["tie"] == good["iter"]) & (S["key"] != S["key"][good["iter"]]))[0][0])
    with pytest.raises(AssertionError, match=r"\[%s\] same inliers earlier" % name):
        N.check_ransac(name, dict(iter=later, score=good["score"], best_h=S["p"][later].astype(np.float32)), S)

    name = "1025 lines"
    segs = Cs.PEEL_CASES[name][0]
    chain = Cs.peel_chain(name)
    ids = oracle_estimate(*Cs.PEEL_CASES[name][:1], *[Cs.PEEL_CASES[name][k] for k in (3, 1, 2)])["group_id"]
    N.check_groups(name, ids, chain)
    assert len(segs) == len(ids) and chain["complete"]
    lost = ids.copy()
    lost[np.nonzero(ids == 1)[0][0]] = -1
    swapped = np.where(ids == 0, 2, np.where(ids == 2, 0, ids))
    for wrong in (lost, swapped):
        with pytest.raises(AssertionError, match=r"\[%s\] group id" % name):
            N.check_groups(name, wrong, chain)
    # ... and where the chain stops early, an id of a decided round on a line it does not know to be in it
    part = dict(chain, settled=chain["settled"] & (chain["ids"] != 3), rounds=3)
    stray = ids.copy()
    stray[np.nonzero(ids == 3)[0][0]] = 1
    N.check_groups(name, ids, part)
    with pytest.raises(AssertionError, match=r"\[%s\] group id" % name):
        N.check_groups(name, stray, part)
