"""The set-up of a flood walk (kernels_flood.hip: explore_body, explore_seed, flood_partial_commit_kernel and the entry loops
of the second tier and of the re-walks from logs) issues its loads a round trip at a time: the control block's words together,
the seed's words from one packed record, the words at the seed pixel together, bytes through the aligned word that holds them,
the per-lane constants from a table.  Nothing of that may show in a result: label image, seed sizes and segment records
against the CPU oracle bit for bit, on the frame geometries at which a word-wise byte fetch or a partial tile can go wrong,
and on one small frame for every branch the set-up can take (the stage counters prove that the branch ran)."""
import numpy as np
import pytest

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


def _assert_lines_equal(a, b):
    assert len(a) == len(b), (len(a), len(b))
    if len(a):
        av = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint32).reshape(len(a), 7)
        bv = np.frombuffer(np.ascontiguousarray(b).tobytes(), np.uint32).reshape(len(b), 7)
        bad = np.nonzero((av != bv).any(axis=1))[0]
        assert len(bad) == 0, "first mismatch at %d: %s vs %s" % (bad[0], a[bad[0]], b[bad[0]])


def _sizes(label, n_seeds):
    """pixels each seed's flood claimed, from a label image (-1: nobody's)"""
    return np.bincount(label[label >= 0].ravel(), minlength=n_seeds).astype(np.int32)


_REFS = {}


def _reference(key, img):
    """the oracle's answer for a frame, worked out once a session and left alone"""
    if key not in _REFS:
        h, w = img.shape
        seg = O.find_line_segments(img)
        groups = O.find_line_segment_groups(img, float(max(w, h)) / 100.0, seed=0)[0]
        _REFS[key] = (seg, groups)
    return _REFS[key]


def _check_frame(L, ctx, key, img):
    """stage by stage (stage_flood), then the full call; returns the flood's counters"""
    h, w = img.shape
    seg, groups = _reference(key, img)
    ctx.stage_filter_host(img)
    n = ctx.stage_seeds()
    assert n == seg["n_seeds"], (key, n, seg["n_seeds"])
    ctx.stage_flood()
    used = ctx.stage_counters()
    used["dead_seeds"] = 0
    lab = ctx.download(L.BUF_LABEL)
    bad = np.argwhere(lab != seg["label"])
    assert len(bad) == 0, "%s: %d label mismatches, first at %s: gpu %d oracle %d" % (
        key, len(bad), bad[0], lab[tuple(bad[0])], seg["label"][tuple(bad[0])])
    if n:
        size = ctx.download(L.BUF_SEED_SIZE)
        np.testing.assert_array_equal(size, _sizes(seg["label"], n), err_msg=str(key))
        used["dead_seeds"] = int((size == 0).sum())
    _assert_lines_equal(ctx.stage_fit(), seg["lines"])
    ctx.set_seed(0)
    _assert_lines_equal(ctx.find_line_segment_groups(img, float(max(w, h)) / 100.0), groups)
    return used


# ---- frame geometry ---------------------------------------------------------------------------------------------------
# 5x5: one tile, one seedable pixel; 8x8: exactly a tile; 9x7: a partial tile in each direction; 61x45 and 333x190: widths
# that are no multiple of 4 (61 = 4 * 15 + 1, 333 = 4 * 83 + 1), so that from row to row a seed pixel's direction-mask
# byte sits at each of the four offsets of its aligned word, and several tiles with ragged last ones.
GEOMETRY = ((5, 5), (8, 8), (9, 7), (61, 45), (333, 190))


def _random_frame(w, h, seed):
    """blurred noise: strong enough for seeds everywhere, smooth enough for floods of more than a pixel"""
    rng = np.random.RandomState(1000 * w + seed)
    a = rng.standard_normal((h + 8, w + 8))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for _ in range(2):
        a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, a)
        a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, a)
    a = a[4:-4, 4:-4]
    return (0.5 + 0.35 * a / max(1e-9, np.abs(a).max())).astype(np.float32)


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("size", GEOMETRY, ids=lambda s: "%dx%d" % s)
def test_frame_geometry(L, ctx, size, seed):
    """Random content, eight frames a size."""
    w, h = size
    img = _random_frame(w, h, seed)
    _check_frame(L, ctx, ("random", w, h, seed), img)


@pytest.mark.parametrize("last", (False, True), ids=("first", "last"))
@pytest.mark.parametrize("size", GEOMETRY, ids=lambda s: "%dx%d" % s)
def test_strongest_seed_at_the_ends_of_the_seedable_area(L, ctx, size, last):
    """The strongest seed -- seed 0, record 0, whose tier byte is byte 0 of its word -- at the lowest pixel index a seed can
    have, and at the highest.  The detector's seeds keep two pixels from the border (the 5x5 filter; a 5x5 frame has the one
    seedable pixel 12), so pixel 0 and the frame's last pixel cannot be seeds in any frame that goes through stage_seeds:
    the ends are (2, 2) and (h - 3, w - 3).  A bright 2x2 corner on faint noise puts the frame's largest gradient there."""
    w, h = size
    rng = np.random.RandomState(w * h)
    img = (0.5 + 0.01 * rng.standard_normal((h, w))).astype(np.float32)
    img[0:2, 0:2] = np.float32(0.95)
    if last:
        img = np.ascontiguousarray(img[::-1, ::-1])
    want = (h - 3) * w + (w - 3) if last else 2 * w + 2
    _check_frame(L, ctx, ("corner", w, h, last), img)
    assert ctx.download(L.BUF_SEED_IDX)[0] == want
    rec = ctx.download(L.BUF_SEED_REC)
    assert rec[0, 0] == want


# ---- the packed record ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", GEOMETRY + ((640, 360),), ids=lambda s: "%dx%d" % s)
def test_packed_seed_record_equals_the_seed_arrays(L, ctx, size):
    """After stage_flood the record of every seed is {seed_idx, seed_bin, bits of seed_thr, 0}, bit for bit."""
    from librectify_amd import synth

    w, h = size
    img = synth.frame(w, h, 72) if w >= 64 else _random_frame(w, h, 3)
    ctx.stage_filter_host(img)
    n = ctx.stage_seeds()
    ctx.stage_flood()
    rec = ctx.download(L.BUF_SEED_REC)
    assert rec.shape == (n, 4) and rec.dtype == np.uint32 and n > 0
    np.testing.assert_array_equal(rec[:, 0], ctx.download(L.BUF_SEED_IDX).view(np.uint32))
    np.testing.assert_array_equal(rec[:, 1], ctx.download(L.BUF_SEED_BIN).view(np.uint32))
    np.testing.assert_array_equal(rec[:, 2], ctx.download(L.BUF_SEED_THR).view(np.uint32))
    assert not rec[:, 3].any()


# ---- one case per branch of the set-up ----------------------------------------------------------------------------------
def _run(L, ctx, key, img):
    return _check_frame(L, ctx, key, img)


def test_seeds_dead_at_their_pixel(L, ctx):
    """Most seeds of a dense frame sit on ground a stronger seed's flood takes, and a list entry of theirs ends at the label
    of their own pixel.  `_random_frame(333, 190, 0)`: 1 514 seeds, 22 of them without a flood of their own (seed sizes
    that are zero), several rounds.  (No counter counts that exit itself: the zero sizes and the rounds are what shows.)"""
    used = _run(L, ctx, ("random", 333, 190, 0), _random_frame(333, 190, 0))
    assert used["dead_seeds"] > 0 and used["flood_rounds"] >= 2, used


def test_seeds_that_own_ground_from_a_partial_commit(L, ctx):
    """A blocked seed's partial commit labels the part of its footprint that is surely its own, and its next exploration starts
    from a pixel that carries its own index (`own`).  `synth.frame(160, 90, 70)` is the smallest frame of the search
    (160x90 .. 640x360, seeds 70-73, at the parent commit) on which the partial commits change what is walked: 2 078 pixels
    with them, 2 147 without -- the counter that shows they ran.  Labels and records are the oracle's either way."""
    from librectify_amd import synth

    img = synth.frame(160, 90, 70)
    walked = {}
    try:
        for on in (True, False):
            ctx.set_flood_partial_commits(on)
            walked[on] = _run(L, ctx, ("bars", 160, 90, 70), img)["walked_px"]
    finally:
        ctx.set_flood_partial_commits(True)
    assert walked[True] < walked[False], walked


@pytest.mark.parametrize("name", ("long_bars", "regions"))
def test_rewalks_from_logs(L, ctx, name):
    """Seeds with a log walk a budget of tiles and then turn to the log, or -- with a log that an earlier round has cut down
    and that is still twice the budget long -- go on the list at once.  `synth.long_bar_frame(240, 135, 3, K=6)` is the smallest
    frame of the search at the parent commit with re-walks from logs (14 of them, three rounds: budgeted ones, a cut-down log
    needs a third round that uses it); `synth.region_frame(160, 90, 4)` has 50 over seven rounds, logs that were cut down in
    one round and come up again in the next among them.  (`synth.frame(640, 360, 72)`, the frame of profiles/batch_refactor.txt,
    has 25; bars need 480x270 for any.)  The counter does not tell direct from budgeted."""
    from librectify_amd import synth

    img = synth.long_bar_frame(240, 135, 3, K=6) if name == "long_bars" else synth.region_frame(160, 90, 4)
    used = _run(L, ctx, (name, "logs"), img)
    assert used["log_rewalks"] > 0 and used["log_give_ups"] == 0, used
    if name == "regions":
        assert used["flood_rounds"] >= 4, used


def test_hand_over_to_the_second_tier(L, ctx):
    """Walks that outgrow the first tier's table travel to the second with their table and frontier (and a seed marked in an
    earlier round skips the first tier).  `synth.ramp_frame(160, 90, 5)`: the smallest frame of the search at the parent commit
    with walks in the second tier, 117 of them over two rounds."""
    from librectify_amd import synth

    used = _run(L, ctx, ("ramp", 160, 90, 5), synth.ramp_frame(160, 90, 5))
    assert used["second_tier_seeds"] > 0 and used["ordered_tail_seeds"] == 0, used


def test_a_frame_after_which_the_calm_hint_drops_the_second_tier(L, ctx):
    """After a frame whose walks all stayed in the first tier the blind rounds go without the second tier's launch, and a walk
    that outgrows the first tier there counts as unfinished (`quiet`).  A calm frame of bars, then `synth.region_frame(480,
    270, 500)` on the same context: the smallest pair of the search at the parent commit with such walks (408; none at
    320x180 and below, none after the calm frame on frames of long bars up to 640x360)."""
    from librectify_amd import synth

    calm = synth.frame(480, 270, 4, bars=8)
    used = _run(L, ctx, ("calm", 480, 270), calm)
    assert used["second_tier_seeds"] == 0 and used["quiet_round_misses"] == 0, used
    used = _run(L, ctx, ("regions", 480, 270, 500), synth.region_frame(480, 270, 500))
    assert used["quiet_round_misses"] > 0 and used["second_tier_seeds"] > 0, used


def test_a_giant_step_leaves_seeds_marked_as_finished(L, ctx):
    """The giant step labels the lowest active seed's flood between two rounds and marks the seeds it finished (tier bit 3): the
    round behind it reads that mark from the tier byte's word.  A noiseless radial gradient at 1280x720 (the frame of
    test_giant_steps_label_what_the_slab_walk_and_the_oracle_label: sixteen rings, a chain of steps); the search at the parent
    commit found no giant step on any synthetic frame up to 640x360 -- a flood has to outgrow the second tier's 1 024 tiles."""
    yy, xx = np.mgrid[0:720, 0:1280].astype(np.float64)
    img = (1.0 - np.hypot(xx - 640, yy - 360) / np.hypot(640, 360)).astype(np.float32)
    used = _run(L, ctx, ("radial", 1280, 720), img)
    assert used["giant_steps"] >= 8 and used["slabs"] == 0, used
