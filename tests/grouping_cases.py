"""The cases of the grouping second-source tests (test_grouping_second_source_cpu.py holds the oracle to them,
test_gpu_grouping_second_source.py the kernels) and the two drivers that run a solver through numpy_grouping_ref's checks.
What each case is for is said where it is built.  Whether a case is decided depends on the second source alone, so the
seeds below were chosen on the CPU; the CPU module asserts that they still decide.  Test infrastructure only."""
import functools

import numpy as np

import numpy_grouping_ref as N

LINE_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("weight", "<f4"), ("err", "<f4"), ("group_id", "<i4")])
TOL = np.float32(1.0 - np.cos(np.deg2rad(2.0)))  # the inlier tolerance a caller of lr_ransac_best passes (config.h: 2 degrees)
VPS = np.array([[3100.0, 400.0], [-2200.0, 700.0], [450.0, -5000.0]])


def records(p1, p2):
    out = np.zeros(len(p1), LINE_DTYPE)
    out["x1"], out["y1"], out["x2"], out["y2"] = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    out["weight"], out["err"], out["group_id"] = 0.25, 0.5, -1
    return out


def segments(n, seed, on=(0.2, 0.2, 0.2), noise=0.004, size=1000.0):
    """n segments in a size x size frame: fractions `on` of them on the three pencils VPS (turned by N(0, noise) rad),
    the rest uniform; in random order"""
    rng = np.random.RandomState(seed)
    which = rng.choice(4, n, p=list(on) + [1.0 - sum(on)])
    c = rng.uniform(0.05, 0.95, (n, 2)) * size
    half = rng.uniform(0.03, 0.15, n) * size / 2
    to_vp = VPS[np.minimum(which, 2)] * (size / 1000.0) - c
    ang = np.where(which < 3, np.arctan2(to_vp[:, 1], to_vp[:, 0]) + rng.normal(0, noise, n), rng.uniform(0, np.pi, n))
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    return records(c - d, c + d)


# ---- one solve: lr_ransac_best ----------------------------------------------------------------------------------------------
# name -> (normalised fp32 records, indices, n_iter, seed, round, what the case asserts of its own coverage)
def _sizes():
    """Line counts around the wavefront (63 / 64 / 65) and the 512-line LDS chunk (one chunk, exactly two, two and a line);
    hypothesis counts that end inside a wavefront's four (1, 15, 17) and beyond the 32 slots (513 = 33 workgroups); rounds
    0 and 3; a seed above 2^32; every other line as `indices` in two of them.  expect: decided."""
    out = {}
    for n, n_iter, rnd, seed, every_other in [(2, 1, 0, 1, False), (3, 15, 3, 1, False), (63, 16, 0, 2, False), (64, 17, 3, (1 << 40) + 5, False),
                                              (65, 513, 0, 1, False), (511, 300, 3, 1, False), (512, 300, 0, (7 << 32) + 1, False),
                                              (513, 513, 3, 1, True), (1024, 200, 0, 1, False), (1025, 333, 3, 2, True)]:
        norm = N.normalised_f32(segments(n, 100 + n))
        idx = np.arange(n, dtype=np.int32)[::2] if every_other else np.arange(n, dtype=np.int32)
        out["%d lines, %d hypotheses" % (n, n_iter)] = (norm, idx, n_iter, seed, rnd, dict(decided=True))
    # eight hypotheses per wavefront (n_iter >= 65536), whole and with a ragged last workgroup (65569 = 2049 x 32 + 1)
    norm = N.normalised_f32(segments(130, 230))
    for n_iter in (65536, 65569):
        out["130 lines, %d hypotheses" % n_iter] = (norm, np.arange(130, dtype=np.int32), n_iter, 3, 0, dict(decided=True))
    return out


def _content():
    out = {}
    rng = np.random.RandomState(5)
    # integer coordinates, horizontal and vertical: h = (0, hy, hz) and (hx, 0, hz), so p.z of two of a family is exactly 0
    y = rng.permutation(900)[:60] + 50.0
    x0 = rng.randint(50, 500, 60).astype(np.float64)
    hor = records(np.stack([x0, y], 1), np.stack([x0 + rng.randint(30, 300, 60), y], 1))
    x = rng.permutation(900)[:60] + 50.0
    y0 = rng.randint(50, 500, 60).astype(np.float64)
    ver = records(np.stack([x, y0], 1), np.stack([x, y0 + rng.randint(30, 300, 60)], 1))
    mix = np.concatenate([hor, ver, segments(80, 11)])[rng.permutation(200)]
    out["horizontal and vertical families"] = (N.normalised_f32(mix), np.arange(200, dtype=np.int32), 600, 4, 0, dict(ideal=60))
    # a parallel family at 30 degrees: p.z is what rounding leaves
    c = rng.uniform(100, 900, (80, 2))
    d = np.array([np.cos(np.pi / 6), np.sin(np.pi / 6)]) * rng.uniform(20, 80, 80)[:, None]
    mix = np.concatenate([records(c - d, c + d), segments(120, 12)])[rng.permutation(200)]
    out["parallel family at 30 degrees"] = (N.normalised_f32(mix), np.arange(200, dtype=np.int32), 600, 5, 0, dict(ideal=40))
    # five lines twenty times each among a hundred others: samples of two copies fail the sample check
    base = segments(105, 13)
    mix = np.concatenate([np.tile(base[:5], 20), base[5:]])[rng.permutation(200)]
    out["five lines twenty times"] = (N.normalised_f32(mix), np.arange(200, dtype=np.int32), 600, 6, 0, dict(invalid=10))
    # one line seventy times: no sample is valid, nothing scores
    out["one line seventy times"] = (N.normalised_f32(np.tile(segments(1, 14), 70)),
                                     np.arange(70, dtype=np.int32), 300, 7, 0, dict(invalid=300, nothing=True))
    # two copies and one other line
    two = segments(2, 16)
    out["two copies and one other"] = (N.normalised_f32(two[[0, 0, 1]]), np.arange(3, dtype=np.int32), 50, 8, 0, dict(invalid=5, later_draws=5))
    # a star: segments p, -p (normalised coordinates) share the midpoint (0, 0); two of them meet there exactly, so v = 0
    ang = rng.uniform(0, np.pi, 100)
    p = (np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0.05, 0.4, 100)[:, None]).astype(np.float32).astype(np.float64)
    others = N.normalised_f32(segments(100, 17))
    star = np.concatenate([records(-p, p), others])[rng.permutation(200)]
    out["star through one midpoint"] = (star, np.arange(200, dtype=np.int32), 600, 9, 0, dict(nan=1000))
    # a pencil, every other line of it turned about its midpoint by the tolerance angle: decisions inside the band
    c = rng.uniform(100, 900, (100, 2))
    to_vp = VPS[0] - c
    a = np.arctan2(to_vp[:, 1], to_vp[:, 0]) + np.where(np.arange(100) % 2 == 1, np.arccos(1.0 - float(TOL)), 0.0)
    d = np.stack([np.cos(a), np.sin(a)], 1) * rng.uniform(30, 80, 100)[:, None]
    mix = np.concatenate([records(c - d, c + d), segments(100, 18, on=(0.0, 0.3, 0.3))])[rng.permutation(200)]
    out["pencil turned by the tolerance"] = (N.normalised_f32(mix), np.arange(200, dtype=np.int32), 600, 10, 0, dict(in_band=200))
    # three lines, 600 draws of three pairs: exact ties in every workgroup, the lowest draw must win
    out["three lines, 600 hypotheses"] = (N.normalised_f32(segments(3, 19)), np.arange(3, dtype=np.int32), 600, 11, 0, dict(later_draws=100, decided=True))
    return out


RANSAC_CASES = {}
RANSAC_CASES.update(_sizes())
RANSAC_CASES.update(_content())


@functools.lru_cache(maxsize=None)
def ransac_intervals(name):
    norm, idx, n_iter, seed, rnd, _ = RANSAC_CASES[name]
    return N.score_intervals(N.Model(N._xy(norm)), idx, float(TOL), n_iter, seed, rnd)


def run_ransac_case(name, solve):
    """solve(lines_norm, indices, tol, n_iter, seed, rnd) -> dict(iter, score, best_h).  Checks it, asserts the case's own
    coverage from the second source, returns the counts."""
    norm, idx, n_iter, seed, rnd, expect = RANSAC_CASES[name]
    S = ransac_intervals(name)
    res = solve(norm, idx, TOL, n_iter, seed, rnd)
    counts = dict(N.coverage(S), **N.check_ransac(name, res, S))
    for k, v in expect.items():
        if k == "decided":
            assert counts["decided"], "[%s] coverage: the second source does not decide the winner (%d rivals)" % (name, counts["rivals"])
        elif k == "nothing":
            assert res["iter"] == -1 and N.winner(S) == (-1, True), "[%s] coverage: something scored" % name
        else:
            assert counts[k] >= v, "[%s] coverage: %s is %d, the case needs %d" % (name, k, counts[k], v)
    return counts


# ---- the peeling: lr_estimate_line_pencils ----------------------------------------------------------------------------------
# name -> (segments, n_iter, seed, max_models, what the case asserts)
def _peel():
    out = {}
    # the 1024-wide loops of the peel kernel: one trip short, exact, one line into the second, two trips and a line
    for n, s in [(1023, 4), (1024, 2), (1025, 2), (2049, 4)]:
        out["%d lines" % n] = (segments(n, 300 + n + s), 300, 40 + n, 4, dict(complete=True))
    # the inliers' staging: 2048 in LDS, the rest through memory
    out["2600 lines, more than 2048 inliers"] = (segments(2600, 503, on=(0.88, 0.02, 0.02), noise=0.002), 300, 51, 4, dict(complete=True, inliers0=(2049, 2600)))
    out["2600 lines, just below 2048 inliers"] = (segments(2600, 503, on=(0.765, 0.05, 0.05), noise=0.002), 300, 52, 4, dict(complete=True, inliers0=(1946, 2047)))
    # a pencil and ten copies of a stray line: round 1 has no valid sample, its refit runs over all 70 lines
    rng = np.random.RandomState(6)
    c = rng.uniform(100, 900, (60, 2))
    to_vp = VPS[0] - c
    d = to_vp / np.linalg.norm(to_vp, axis=1)[:, None] * rng.uniform(20, 70, 60)[:, None]
    stray = records(np.array([[200.0, 300.0]]), np.array([[260.0, 420.0]]))
    out["pencil and ten copies of a stray"] = (np.concatenate([records(c - d, c + d), np.tile(stray, 10)]), 300, 53, 4, dict(no_winner_round=1, rounds=2))
    out["no hypotheses"] = (segments(200, 503), 0, 54, 4, dict(no_winner_round=0, rounds=1))
    out["one hypothesis"] = (segments(200, 501), 1, 55, 4, dict(complete=True))
    for mm in (0, 1, 4, 5):
        out["max_models %d" % mm] = (segments(300, 505), 300, 56, mm, dict(complete=True))
    for n in (0, 1, 2):
        out["%d lines" % n] = (segments(5, 506)[:n], 300, 57, 4, dict(complete=True))
    return out


PEEL_CASES = _peel()


@functools.lru_cache(maxsize=None)
def peel_chain(name):
    segs, n_iter, seed, mm, _ = PEEL_CASES[name]
    return N.peel_chain(segs, n_iter, seed, mm)


def run_peel_case(name, estimate):
    """estimate(segments, max_models, n_iter, seed) -> records with group ids.  Every round the chain decided is compared."""
    segs, n_iter, seed, mm, expect = PEEL_CASES[name]
    chain = peel_chain(name)
    got = estimate(segs, mm, n_iter, seed)
    assert len(got) == len(segs), "[%s] %d lines came back for %d" % (name, len(got), len(segs))
    counts = N.check_groups(name, got["group_id"], chain)
    counts.update(winners=chain["winners"], winner_inliers=chain["winner_inliers"], grouped=chain["grouped"], reason=chain["reason"])
    if expect.get("complete"):
        assert chain["complete"], "[%s] coverage: the second source stops early (%s)" % (name, chain["reason"])
    if "rounds" in expect:
        assert chain["rounds"] >= expect["rounds"], "[%s] coverage: %d rounds decided (%s), the case needs %d" % (name, chain["rounds"], chain["reason"], expect["rounds"])
    if "no_winner_round" in expect:
        k = expect["no_winner_round"]
        assert chain["winners"][k] == -1 and chain["winner_inliers"][k] == 0, "[%s] coverage: round %d has a winner" % (name, k)
    if "inliers0" in expect:
        lo, hi = expect["inliers0"]
        assert lo <= chain["winner_inliers"][0] <= hi, "[%s] coverage: %d inliers of the first winner, not in [%d, %d]" % (name, chain["winner_inliers"][0], lo, hi)
        assert int((got["group_id"] == 0).sum()) == chain["grouped"][0]  # (the count from the result itself)
    return counts
