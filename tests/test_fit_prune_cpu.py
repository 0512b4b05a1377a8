"""The bound behind the fit threshold (kernels_fit.hip: component_offsets_kernel; frame.hip: fit_min_for), held against the
second source: a segment fitted to an 8-connected set of n pixels is at most (n - 1) * sqrt(2) long, so a component of
n <= floor(ml / 1.4157) pixels never passes `length > ml` and a fused frame may leave its fit out.

Sets of 2 .. 64 pixels -- diagonal chains (the extremal case), staircases, L-shapes, random walks, blobs -- get random
positive weights and go through oracle_lib.fit_line_parameters twice: near the origin (coordinates below 128, where the
relative bound of 1e-4 is about the geometry), and at origins all over a 4K frame, where the float rounding of the ends
is largest (coordinates up to 4096 are 2.4e-4 to 4.9e-4 apart in float32: the ends of a 2-pixel chain are off by 1.7e-4
there, 1.2e-4 of its length).  The threshold is held against both; the far sets have an absolute allowance instead."""
import math

import numpy as np

import oracle_lib as O

SQRT2 = math.sqrt(2.0)
N_RANGE = range(2, 65)
STEPS8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def length_bound_size(ml):
    """the largest n that the bound rules out for this min_length: floor(max(ml, 5) / 1.4157)"""
    ml = float(np.float32(ml))
    ml = ml if ml > 5.0 else 5.0  # (a NaN is the floor, as fmaxf makes it in filter_lines_kernel)
    return int(math.floor(ml / 1.4157))


def fit_min(ml):
    """frame.hip: fit_min_for -- never below the size threshold (floods of up to 5 pixels are no components at all)"""
    return max(5, length_bound_size(ml))


def _diagonal(n, rng, anti=False):
    i = np.arange(n)
    return [(int(a), int(-b if anti else b)) for a, b in zip(i, i)]


def _staircase(n, rng):
    # runs of 1 .. 3 straight steps between diagonal steps, one orientation per set
    dr, dc = [(1, 1), (1, -1), (-1, 1), (-1, -1)][rng.integers(4)]
    straight = (dr, 0) if rng.integers(2) else (0, dc)
    px = [(0, 0)]
    while len(px) < n:
        for _ in range(int(rng.integers(1, 4))):
            if len(px) < n:
                px.append((px[-1][0] + straight[0], px[-1][1] + straight[1]))
        if len(px) < n:
            px.append((px[-1][0] + dr, px[-1][1] + dc))
    return px


def _l_shape(n, rng):
    # two arms from a corner, each along one of the eight directions (two different ones)
    a, b = rng.choice(8, 2, replace=False)
    na = int(rng.integers(0, n))
    px = [(0, 0)]
    for k in range(1, na + 1):
        px.append((STEPS8[a][0] * k, STEPS8[a][1] * k))
    k = 1
    while len(px) < n:
        p = (STEPS8[b][0] * k, STEPS8[b][1] * k)
        k += 1
        if p not in px:
            px.append(p)
    return px


def _random_walk(n, rng):
    seen = {(0, 0)}
    order = [(0, 0)]
    cur = (0, 0)
    while len(order) < n:
        s = STEPS8[rng.integers(8)]
        cur = (cur[0] + s[0], cur[1] + s[1])
        if cur not in seen:
            seen.add(cur)
            order.append(cur)
    return order


def _blob(n, rng):
    seen = {(0, 0)}
    order = [(0, 0)]
    while len(order) < n:
        base = order[rng.integers(len(order))]
        s = STEPS8[rng.integers(8)]
        p = (base[0] + s[0], base[1] + s[1])
        if p not in seen:
            seen.add(p)
            order.append(p)
    return order


def _is_8_connected(px):
    todo, seen, allp = [px[0]], {px[0]}, set(px)
    while todo:
        r, c = todo.pop()
        for dr, dc in STEPS8:
            q = (r + dr, c + dc)
            if q in allp and q not in seen:
                seen.add(q)
                todo.append(q)
    return len(seen) == len(allp) == len(px)


def _length(px, rng, far):
    """segment length of the set, as filter_lines computes it (float32), with random weights at a random origin"""
    a = np.asarray(px, np.int64)
    a = a - a.min(axis=0) + (np.array([rng.integers(0, 2160 - 70), rng.integers(0, 3840 - 140)]) if far else rng.integers(0, 64, 2))
    order = np.lexsort((a[:, 1], a[:, 0]))  # row-major, the order of the detector's component lists
    a = a[order]
    w = rng.uniform(0.01, 1.0, len(a)).astype(np.float32)
    l = O.fit_line_parameters(a[:, 0], a[:, 1], w)
    dx = np.float32(l["x2"]) - np.float32(l["x1"])
    dy = np.float32(l["y2"]) - np.float32(l["y1"])
    return float(np.sqrt(np.float32(dx * dx + dy * dy)))


def _sets():
    rng = np.random.default_rng(20240607)
    out = []  # (kind, n, length near the origin, length somewhere in a 4K frame)
    for n in N_RANGE:
        for anti in (False, True):  # the exact chains for every n
            px = _diagonal(n, rng, anti)
            out.append(("diagonal", n, _length(px, rng, False), _length(px, rng, True)))
        for kind, gen, reps in (("staircase", _staircase, 10), ("L", _l_shape, 10), ("walk", _random_walk, 16), ("blob", _blob, 16)):
            for _ in range(reps):
                px = gen(n, rng)
                assert len(px) == n and _is_8_connected(px), (kind, n)
                out.append((kind, n, _length(px, rng, False), _length(px, rng, True)))
    return out


SETS = None


def sets():
    global SETS
    if SETS is None:
        SETS = _sets()
    return SETS


def test_segment_length_is_bounded_by_the_chain_of_the_component():
    s = sets()
    assert len(s) > 3000
    worst = {}
    worst_far = 0.0
    for kind, n, length, length_far in s:
        bound = (n - 1) * SQRT2
        ratio = length / bound
        worst[kind] = max(worst.get(kind, 0.0), ratio)
        assert length <= bound * (1.0 + 1e-4), (kind, n, length, bound)
        # Anywhere in a 4K frame: centroid, projections and ends are each a few roundings of numbers below 4096 (spacing
        # at most 4.9e-4): a hundredth of a pixel is twenty of them, and a hundredth of the margin the threshold leaves.
        worst_far = max(worst_far, length_far - bound)
        assert length_far <= bound + 1e-2, (kind, n, length_far, bound)
    print("largest length / ((n - 1) * sqrt(2)) by kind:", {k: round(v, 6) for k, v in sorted(worst.items())})
    print("largest length - (n - 1) * sqrt(2) at 4K coordinates: %.2e px" % worst_far)
    # the chains are the extremal case: their length IS the bound, up to rounding
    assert worst["diagonal"] > 1.0 - 1e-4
    assert max(worst.values()) == worst["diagonal"] or max(worst.values()) <= 1.0 + 1e-4


def test_no_component_at_or_below_the_fit_threshold_passes_the_length_test():
    s = sets()
    n = np.array([e[1] for e in s] * 2)
    length = np.array([e[2] for e in s] + [e[3] for e in s], np.float32)
    # a grid from 5 to 200, and the values where the threshold steps (the tightest ml for every n: just above n * 1.4157)
    steps = np.array([k * 1.4157 for k in range(4, 142)])
    grid = np.unique(np.concatenate([np.arange(5.0, 200.001, 0.25), steps, np.nextafter(steps, np.inf), steps + 1e-3]).astype(np.float32))
    grid = grid[(grid >= 5.0) & (grid <= 200.0)]
    fm = np.array([length_bound_size(m) for m in grid])
    assert fm.min() == 3 and fm.max() >= 141 and set(range(3, 65)) <= set(fm.tolist())
    pruned = n[:, None] <= fm[None, :]
    passes = length[:, None] > grid[None, :]
    bad = np.argwhere(pruned & passes)
    assert len(bad) == 0, "set %s of %d px, length %r, passes ml %r with threshold %d" % (
        s[bad[0][0] % len(s)][0], n[bad[0][0]], length[bad[0][0]], grid[bad[0][1]], fm[bad[0][1]])
    # how close it gets: the largest length / ml over every (set, ml) the threshold prunes
    ratio = np.where(pruned, length[:, None] / grid[None, :], 0.0).max()
    print("largest length / ml among pruned (set, ml) pairs: %.6f over %d pairs" % (ratio, int(pruned.sum())))
    assert ratio < 1.0


def test_the_threshold_is_the_size_floor_for_short_min_lengths():
    for ml in (-1.0, 0.0, 1.0, 5.0, 7.0, 8.49, float("nan")):
        assert fit_min(ml) == 5, ml
    assert fit_min(8.5) == 6 and fit_min(38.4) == 27 and fit_min(19.2) == 13
