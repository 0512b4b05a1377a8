"""The opt-in estimators' kernels (cht_votes_kernel<false|true>, cht_peak_kernel, ht_votes_kernel, ht_weights_kernel,
prosac_count_kernel<2|8>, prosac_records_kernel, prosac_record_flags_kernel, prosac_flags_kernel with the chunked host
replay around them) and refine_pairs_kernel against the second source tests/numpy_estimators_ref.py (and numpy_ref.refine),
through the Context, at the edges where they can go wrong: the vote kernel's 512-line workgroup and stride of four lines,
polyline segments of 64, 65 and 128 steps, votes taken back over several workgroups, a cell beyond 2^32, 64 cells under
1024 peak threads, exact ties in both accumulators, zero coefficients, a peak on the rim and the accumulator nobody voted
for, the chunk boundaries of the PROSAC replay and its wide count kernel, NaN weights, ragged 64 x 64 pair tiles and an edge
list that overflows.  The cases, and what each is for, are in tests/estimator_cases.py.  Every case is also compared with
the oracle bit for bit, in an assertion of its own, so that a failure says which source disagreed."""
import numpy as np
import pytest

import estimator_cases as Cs
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L

    L.lib()
    assert L.device_count() > 0, "GPU tests need a GPU"
    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def _same_records(name, got, ref):
    assert len(got) == len(ref) and got.tobytes() == ref.tobytes(), "[%s] oracle: the records differ" % name


@pytest.mark.parametrize("name", list(Cs.ACCUMULATOR_CASES))
def test_accumulator_against_the_second_source(ctx, name):
    got = {}

    def vanishing_point(segs, d):
        got["vp"], got["acc"] = ctx.cht_vanishing_point(segs, d)
        return got["vp"], got["acc"]

    cell = Cs.run_accumulator_case(name, vanishing_point)
    print(name, "peak cell", cell)
    segs, d, _ = Cs.ACCUMULATOR_CASES[name]
    vp, acc = O.cht_vanishing_point(segs, d)
    bad = np.nonzero((got["acc"] != acc).reshape(-1))[0]
    assert len(bad) == 0, "[%s] oracle: %d cells differ, first %d" % (name, len(bad), bad[0])
    assert got["vp"].tobytes() == vp.tobytes(), "[%s] oracle: vanishing point %r, the oracle's %r" % (name, got["vp"], vp)


@pytest.mark.parametrize("name", list(Cs.CHT_PEEL_CASES))
def test_diamond_peeling_against_the_second_source(ctx, name):
    got = {}

    def estimate(segs, mm, d):
        got["r"] = ctx.estimate_line_pencils_cht(segs, max_models=mm, d=d)
        return got["r"]

    print(name, Cs.run_cht_peel_case(name, estimate))
    segs, d, mm, _ = Cs.CHT_PEEL_CASES[name]
    ref, ref_m, ref_c = O.estimate_line_pencils_cht(segs, max_models=mm, d=d)
    lines, models, cells, _ = got["r"]
    assert list(cells) == list(ref_c), "[%s] oracle: cells %r, the oracle's %r" % (name, cells, ref_c)
    _same_records(name, lines, ref)


def test_the_estimator_of_a_frame_call_is_the_stand_alone_one(ctx):
    """lr_set_estimator(3, d) and find_line_segment_groups once, on a 257 x 131 frame: the groups are those of the stand-alone
    entry on the same lines, which are held to the second source"""
    from librectify_amd import synth

    img = synth.frame(257, 131, 3, bars=20)
    ctx.set_estimator(3, 64)
    try:
        got = ctx.find_line_segment_groups(img, 2.57)
    finally:
        ctx.set_estimator(0)
    assert len(got) >= 8
    segs = got.copy()
    segs["group_id"] = -1
    import numpy_estimators_ref as E
    import numpy_grouping_ref as N

    assert Cs.diamond_share(segs, 64) <= E.AMBIGUITY_CAP  # the cap, before the estimator's result is looked at
    lines, models, cells, votes = ctx.estimate_line_pencils_cht(segs, d=64)
    _same_records("frame", lines, got)
    chain = E.cht_chain("frame", segs, 64, 4, cells)
    assert chain["complete"], chain["reason"]
    print("frame", len(got), "lines", N.check_groups("frame", got["group_id"], chain), chain["reason"])
    E.check_models("frame", models, chain)


@pytest.mark.parametrize("name", list(Cs.HT_CASES))
def test_hough_weights_against_the_second_source(ctx, name):
    want = Cs.check_hough_case(name)
    position, w = Cs.run_hough_case(name, ctx.ht_weights)
    assert position == want
    norm, idx, _ = Cs.HT_CASES[name]
    ref = O.get_weights_fixed(norm, idx)
    assert w.tobytes() == ref.tobytes(), "[%s] oracle: %d weights differ" % (name, (w != ref).sum())


def test_no_vote_never_hands_the_librarys_sort_a_nan(ctx):
    """copies of one line through lr_prosac_solve: the weights of the accumulator nobody voted for reach
    stable_order_descending as numbers, every sample fails its check, nothing is found"""
    for k in range(24):
        a = np.pi * k / 24
        p = np.array([[0.3 * np.cos(a) + 0.1, 0.3 * np.sin(a) - 0.05]])
        norm = Cs._normalised(np.tile(-p, (4, 1)), np.tile(p, (4, 1)))
        idx = np.arange(4, dtype=np.int32)
        w = ctx.ht_weights(norm, idx)
        assert np.isfinite(w).all() and (w >= 0).all() and (w <= 1).all(), (k, w)
        res = ctx.prosac_solve(norm, idx, Cs.TOL, 50, 1, 0)
        assert res["best_iter"] == -1 and res["I_N_best"] == 0 and np.isfinite(res["h"]).all(), (k, res)


@pytest.mark.parametrize("name", list(Cs.PROSAC_CASES))
def test_prosac_against_the_second_source(ctx, name):
    got = {}

    def solve(*a):
        got.update(ctx.prosac_solve(*a))
        return got

    print(name, Cs.run_prosac_case(name, ctx.ht_weights, solve))
    norm, idx, T_N, seed, rnd, _ = Cs.PROSAC_CASES[name]
    ref = O.prosac_solve(norm, idx, Cs.PROSAC_CASES[name][5].get("tol", Cs.TOL), T_N, seed, rnd)
    for k in ("iterations", "n_star", "best_iter", "I_N_best"):
        assert got[k] == ref[k], "[%s] oracle: %s %d, the oracle's %d" % (name, k, got[k], ref[k])
    assert np.abs(got["h"] - ref["h"]).max() <= 1e-5, "[%s] oracle: h %r, the oracle's %r" % (name, got["h"], ref["h"])


@pytest.mark.parametrize("name", list(Cs.PROSAC_PEEL_CASES))
def test_prosac_peeling_against_the_second_source(ctx, name):
    got = {}

    def estimate(segs, mm, T_N, seed):
        got["lines"] = ctx.estimate_line_pencils_prosac(segs, max_models=mm, T_N=T_N, seed=seed)
        return got["lines"]

    print(name, Cs.run_prosac_peel_case(name, ctx.ht_weights, estimate))
    segs, T_N, seed, mm, _ = Cs.PROSAC_PEEL_CASES[name]
    _same_records(name, got["lines"], O.estimate_line_pencils_prosac(segs, max_models=mm, T_N=T_N, seed=seed))


@pytest.mark.parametrize("n", Cs.REFINE_SIZES)
def test_refine_pairs_against_the_second_source(ctx, n):
    ref, closest, lines = Cs.refine_reference(n)
    assert closest > 1e-3
    got = ctx.refine_lines(lines)
    Cs.check_refine("%d segments" % n, got, ref)
    _same_records("%d segments" % n, got, O.refine_lines(lines))


def test_refine_edge_list_overflows_and_the_kernel_runs_again(L):
    """a context of its own, whose edge list starts at 16 n = 32 768: the 44 850 edges of the stack do not fit, the kernel
    counts them all and is launched again with room for them; then a plain call on the same context"""
    ref, closest, lines = Cs.refine_reference(0)
    c = L.Context(0)
    try:
        got = c.refine_lines(lines)
        Cs.check_refine("overflow", got, ref)
        _same_records("overflow", got, O.refine_lines(lines))
        ref2, _, lines2 = Cs.refine_reference(2049)
        Cs.check_refine("after the overflow", c.refine_lines(lines2), ref2)
    finally:
        c.close()


def test_the_context_still_answers_a_plain_ransac_call(ctx):
    """after the estimators took turns and their buffers grew (50 000 lines, 65 536-iteration chunks, an estimator set and
    reset): a RANSAC solve and a peeling of the grouping second source's cases, on the same context"""
    import grouping_cases as Gc

    Gc.run_ransac_case("513 lines, 513 hypotheses", lambda *a: ctx.ransac_best(*a))
    Gc.run_peel_case("1025 lines", lambda s, mm, n_iter, seed: ctx.estimate_line_pencils(s, max_models=mm, n_iter=n_iter, seed=seed))
