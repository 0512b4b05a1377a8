"""The grouping kernels (lines_bbox_kernel, pencil_model_kernel, ransac_score_kernel<4|8>, peel_kernel) against the
float64 second source tests/numpy_grouping_ref.py, through ctx.ransac_best and ctx.estimate_line_pencils, at the edges
where they can go wrong: the 512-line LDS chunk and the wavefront (511 / 512 / 513, 63 / 64 / 65 lines), hypothesis counts
that end inside a wavefront, more workgroups than best-slots, eight hypotheses per wavefront with a ragged last workgroup,
ideal points, failed sample checks, NaN errors, decisions inside the band, exact ties; the second trip of the peel kernel's
1024-wide loops, more than 2048 staged inliers, a round without a winner, every max_models.  The cases, and what each is
for, are in tests/grouping_cases.py.  Every case is also compared with the oracle bit for bit, in an assertion of its own,
so that a failure says which source disagreed."""
import numpy as np
import pytest

import grouping_cases as Cs
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


@pytest.mark.parametrize("name", list(Cs.RANSAC_CASES))
def test_solve_against_the_second_source(ctx, name):
    got = {}

    def solve(norm, idx, tol, n_iter, seed, rnd):
        got.update(ctx.ransac_best(norm, idx, tol, n_iter, seed, rnd))
        return got

    counts = Cs.run_ransac_case(name, solve)
    print(name, counts)
    norm, idx, n_iter, seed, rnd, _ = Cs.RANSAC_CASES[name]
    ref = O.ransac_best(norm, idx, Cs.TOL, n_iter, seed, rnd)
    assert got["iter"] == ref["iter"], "[%s] oracle: iteration %d, the oracle's %d" % (name, got["iter"], ref["iter"])
    assert np.float32(got["score"]).tobytes() == np.float32(ref["score"]).tobytes(), "[%s] oracle: score %r, the oracle's %r" % (name, got["score"], ref["score"])
    assert got["best_h"].tobytes() == ref["best_h"].tobytes(), "[%s] oracle: hypothesis %r, the oracle's %r" % (name, got["best_h"], ref["best_h"])


@pytest.mark.parametrize("name", list(Cs.PEEL_CASES))
def test_peeling_against_the_second_source(ctx, name):
    got = {}

    def estimate(segs, max_models, n_iter, seed):
        got["lines"] = ctx.estimate_line_pencils(segs, max_models=max_models, n_iter=n_iter, seed=seed)
        return got["lines"]

    counts = Cs.run_peel_case(name, estimate)
    print(name, counts)
    segs, n_iter, seed, mm, _ = Cs.PEEL_CASES[name]
    ref, _ = O.estimate_line_pencils(segs, max_models=mm, n_iter=n_iter, seed=seed)
    bad = np.nonzero(got["lines"]["group_id"] != ref["group_id"])[0]
    assert len(bad) == 0, "[%s] oracle: %d group ids differ, first at line %d" % (name, len(bad), bad[0])
    for k in ("x1", "y1", "x2", "y2", "weight", "err"):
        assert got["lines"][k].tobytes() == segs[k].tobytes(), "[%s] %s came back changed" % (name, k)


def test_six_models_are_refused_and_the_context_goes_on(L, ctx):
    """max_models = 6 is beyond what the device buffers hold (kMaxPeelModels): an error, and the next call is served"""
    segs = Cs.PEEL_CASES["max_models 5"][0]
    with pytest.raises(L.LibrectifyError, match="max_models"):
        ctx.estimate_line_pencils(segs, max_models=6, n_iter=300, seed=56)
    Cs.run_peel_case("max_models 5", lambda s, mm, n_iter, seed: ctx.estimate_line_pencils(s, max_models=mm, n_iter=n_iter, seed=seed))
    Cs.run_ransac_case("3 lines, 15 hypotheses", lambda *a: ctx.ransac_best(*a))
