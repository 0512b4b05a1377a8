"""Fused frames leave out the fit of components too small to pass their length test (kernels_fit.hip:
component_offsets_kernel, frame.hip: fit_min_for).  Nothing a caller sees may move: a context that prunes and one that
fits everything (lr_set_estimator(ctx, 0, 0)) live side by side here and must return the same records, transforms and counters, with
`min_length` swept so that the threshold crosses every component size the frames have.  Small frames only; the bound
itself is held against the oracle in test_fit_prune_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWEEP = [round(0.37 * k, 2) for k in range(int(80 / 0.37) + 1)]  # 0 .. 79.92


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L

    L.lib()
    assert L.device_count() > 0, "GPU tests need a GPU"
    return L


@pytest.fixture(scope="module")
def pair(L):
    """(a context that prunes, one that fits every component)"""
    prune = L.Context(0)
    plain = L.Context(0)
    plain.set_estimator(0, 0)
    for c in (prune, plain):
        c.set_seed(0)
        c.set_batch_streams(5)
    yield prune, plain
    prune.close()
    plain.close()


def fit_min(ml):
    """frame.hip: fit_min_for"""
    ml = float(np.float32(ml))
    return max(5, int(np.floor((ml if ml > 5.0 else 5.0) / 1.4157)))


def stroke_frame(W=480, H=420, seed=5):
    """diagonal strokes of one pixel's width and 3 .. 60 pixels' length, alternately falling and rising, on a flat ground"""
    img = np.full((H, W), 0.2, np.float32)
    x = y = 6
    row_h = 0
    for k in range(3, 61):
        if x + k + 6 > W:
            x, y, row_h = 6, y + row_h + 8, 0
        i = np.arange(k)
        img[y + (i if k % 2 else k - 1 - i), x + i] = 0.9
        x += k + 8
        row_h = max(row_h, k)
    assert y + row_h + 6 <= H
    return img + np.random.RandomState(seed).normal(0, 0.003, (H, W)).astype(np.float32)


def few_small_components_frame():
    """three short strokes on a flat ground: a handful of components, none of more than twenty pixels"""
    img = np.full((48, 64), 0.2, np.float32)
    for x0, y0 in ((8, 8), (30, 12), (44, 30)):
        i = np.arange(7)
        img[y0 + i, x0 + i] = 0.9
    return img


def counts(L, c):
    w = c.download(L.BUF_COUNTS)
    return dict(components=int(w[1]), px=int(w[2]), fitted=int(w[12]), fitted_px=int(w[13]))


def same_lines(a, b):
    return len(a) == len(b) and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _sweep_frames():
    from librectify_amd import synth

    f = {("bars333", s): synth.frame(333, 190, s) for s in (1, 2, 3)}
    f.update({("bars480", s): synth.frame(480, 270, s, bars=8) for s in (1, 2, 3)})
    f[("strokes", 5)] = stroke_frame()
    return f


SWEEP_FRAMES = _sweep_frames()


@pytest.mark.parametrize("key", list(SWEEP_FRAMES), ids=lambda k: "%s-%d" % k)
def test_min_length_sweep_equals_the_unpruned_context(L, pair, key):
    prune, plain = pair
    img = SWEEP_FRAMES[key]
    h, w = img.shape
    d = [c.device_upload(img) for c in pair]
    try:
        pruned_some = kept_some = 0
        sizes_crossed = set()
        for ml in SWEEP:
            got = []
            for c, p in zip(pair, d):
                lines = c.find_line_segment_groups_device(p, w, h, ml).copy()
                got.append((lines, L.compute_rectification_transform(lines, w, h).as_array(), c.stage_counters(), counts(L, c)))
            (la, ta, ca, na), (lb, tb, cb, nb) = got
            assert same_lines(la, lb), (key, ml, len(la), len(lb))
            assert ta.tobytes() == tb.tobytes(), (key, ml)
            assert ca == cb, (key, ml, ca, cb)
            assert ca["components"] == na["components"] == nb["components"] and ca["labelled_px"] == na["px"] == nb["px"]
            assert nb["fitted"] == nb["components"] and nb["fitted_px"] == nb["px"], (key, ml, nb)
            assert na["fitted"] <= na["components"] and na["fitted_px"] <= na["px"]
            if fit_min(ml) == 5:
                assert na["fitted"] == na["components"] and na["fitted_px"] == na["px"], (key, ml, na)
            pruned_some += na["fitted"] < na["components"]
            kept_some += len(la) > 0
            sizes_crossed.add(na["fitted"])
        print(key, "calls that pruned: %d of %d; with lines: %d; distinct fitted counts: %d" % (pruned_some, len(SWEEP), kept_some, len(sizes_crossed)))
        assert pruned_some > len(SWEEP) // 2 and kept_some > 0 and len(sizes_crossed) > 8
    finally:
        for c, p in zip(pair, d):
            c.device_free(p)


def test_fewer_fitted_than_two_components_is_not_the_raw_count_exit(L, pair):
    """interface.cpp:50-54 leaves on fewer than two RAW segments; the frame has a few, all below the threshold, so none is
    fitted: an empty result in both contexts, by the length test, and equal counters."""
    img = few_small_components_frame()
    res = []
    for c in pair:
        lines = c.find_line_segment_groups(img, 60.0)
        res.append((lines, c.stage_counters(), counts(L, c)))
    (la, ca, na), (lb, cb, nb) = res
    assert len(la) == 0 and len(lb) == 0
    assert ca == cb
    assert 2 <= na["components"] <= 8 and na["components"] == nb["components"] == nb["fitted"], (na, nb)
    assert na["fitted"] == 0 and na["fitted_px"] == 0, na
    # with a short min_length the same frame has its lines, the same in both
    la, lb = (c.find_line_segment_groups(img, 5.0) for c in pair)
    assert len(la) >= 2 and same_lines(la, lb)


@pytest.mark.parametrize("ml", [0.0, 5.0])
def test_no_pruning_at_the_floor(L, pair, ml):
    prune, _ = pair
    assert fit_min(ml) == 5
    for key in (("bars333", 1), ("strokes", 5)):
        prune.find_line_segment_groups(SWEEP_FRAMES[key], ml)
        n = counts(L, prune)
        assert n["components"] > 20 and n["fitted"] == n["components"] and n["fitted_px"] == n["px"], (key, n)


def _batch_frames():
    from librectify_amd import synth

    W, H = 320, 200
    f = [synth.frame(W, H, 40 + i, bars=b) for i, b in enumerate((6, 12, 24, 40, 12, 24))]
    f += [synth.long_bar_frame(W, H, 3, K=6), synth.long_bar_frame(W, H, 4, K=10)]
    f += [synth.region_frame(W, H, 4), synth.region_frame(W, H, 500), synth.ramp_frame(W, H, 5)]
    f += [stroke_frame()[:H, :W].copy(), np.full((H, W), 0.25, np.float32), synth.frame(W, H, 60, bars=24, noise=0.0)]
    assert len(f) == 14
    return [np.ascontiguousarray(x, np.float32) for x in f]


def test_batches_over_five_lanes_equal_the_unpruned_context(L, pair):
    frames = np.stack(_batch_frames())
    B, H, W = frames.shape
    for ml in (3.2, 17.0, 41.5):
        res = [c.find_line_segment_groups_batch_host(frames, ml, capacity=2048, num_threads=4) for c in pair]
        (oa, na, ta), (ob, nb, tb) = res
        assert (na == nb).all(), (ml, na, nb)
        assert na.max() <= 2048
        for b in range(B):
            assert oa[b][: na[b]].tobytes() == ob[b][: nb[b]].tobytes(), (ml, b)
        assert bytes(ta) == bytes(tb), ml
    assert na.max() > 0
    # a frame table: every frame with a min_length of its own (-1: the call's)
    own = [-1.0, 0.0, 5.0, 8.5, 9.0, 12.0, 17.3, 23.0, 29.9, 38.4, 47.0, 55.5, 64.0, 79.0]
    res = []
    for c in pair:
        d = c.device_upload(frames)
        try:
            rows = [(d + b * H * W * 4, W, H, W, own[b]) for b in range(B)]
            res.append(c.find_line_segment_groups_frames_device(rows, L.PIX_F32, 21.0, capacity=2048))
        finally:
            c.device_free(d)
    (la, ta), (lb, tb) = res
    for b in range(B):
        assert same_lines(la[b], lb[b]), (b, own[b], len(la[b]), len(lb[b]))
        assert bytes(ta[b]) == bytes(tb[b]), b
    assert sum(len(x) for x in la) > 0


def test_raw_segments_after_a_pruned_frame_are_all_there(L, pair):
    """after a fused frame lr_stage_fit fits every component of the label image again: all raw segments, one for one those
    of the staged route on the context that never prunes"""
    prune, plain = pair
    img = SWEEP_FRAMES[("bars480", 2)]
    prune.find_line_segment_groups(img, 30.0)
    n = counts(L, prune)
    assert n["fitted"] < n["components"], n
    raw = prune.stage_fit()
    plain.stage_filter_host(img)
    plain.stage_seeds()
    plain.stage_flood()
    want = plain.stage_fit()
    assert len(raw) == n["components"] == len(want) and same_lines(raw, want)
    assert counts(L, prune)["fitted"] == n["components"]


def test_second_laps_equal_the_unpruned_context(L, pair):
    """the hooks of test_second_laps_of_the_one_wait_pipeline_are_exact: a seed sort too small, a flood with one blind round --
    the stages after the flood run again, with the frame's threshold"""
    from librectify_amd import synth

    img = synth.frame(640, 480, 5)
    ml = 30.0
    for c in pair:
        c.set_flood_just_in_time(False)
    try:
        first = [c.find_line_segment_groups(img, ml) for c in pair]
        assert same_lines(*first) and len(first[0]) > 0
        n_seeds = pair[0].stage_counters()["seeds"]
        assert pair[0].stage_counters()["flood_rounds"] >= 3
        for cap, blind in [(n_seeds // 3, None), (None, 1), (n_seeds // 2, 1)]:
            got = []
            for c in pair:
                if cap:
                    c.set_seed_capacity(cap)
                if blind:
                    c.set_flood_blind_rounds(blind)
                got.append(c.find_line_segment_groups(img, ml))
                assert c.stage_counters()["frame_laps"] >= 2, (cap, blind, c.stage_counters())
            assert same_lines(got[0], got[1]) and same_lines(got[0], first[0]), (cap, blind)
            na, nb = (counts(L, c) for c in pair)
            assert na["components"] == nb["components"] and na["px"] == nb["px"] and na["fitted"] < nb["fitted"], (na, nb)
    finally:
        for c in pair:
            c.set_flood_just_in_time(True)
