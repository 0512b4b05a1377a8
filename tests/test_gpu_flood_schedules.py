"""The parallel flood under chosen schedules (lr_set_flood_schedule): the order of every round's active list -- as is,
reversed, three permutations -- and the number of workgroups that walk it -- each launch's own grid, seven, ONE (a serial
round: its walks one after the other in list order).  The flood is exact because a round's result depends neither on the
order nor on the concurrency of its walks (DESIGN.md section 7 and its table of list readers); here both are variables.  Every
case compares the label image, the seed sizes, the records of stage_fit and the full call with the CPU oracle bit for bit,
no tolerances, and `scheduled_rounds` proves that the rounds were enqueued under the hook (0 under the as-is schedule).

The frames are the smallest ones the repository knows to reach each branch (test_gpu_flood_prologue.py found them); each keeps
that module's coverage assertion.  Which counters may be asserted under every schedule follows DESIGN.md section 7: a walk's
footprint, and so whether it outgrows a tier, is logged, is blocked or dies, is a function of the labels at the round's start;
what depends on arrival is who gets a place in a list that is FULL (second tier, re-walk list: 8 192 entries, log buffer) and
the round in which a seed that waits for its blocker is let go (the survivors pass may read the blocker's state of the same
pass).  The lists of 8 192 entries stay far from full on these frames, so `> 0` holds for every schedule; one frame,
`synth.region_frame(480, 270, 500)`, does fill the log buffer (65 536 records), and there the split between second-tier walks
and re-walks from logs moves with the schedule (4 468 / 2 955 as is, 2 464 / 4 659 as is at width 7) while pixels walked,
rounds and quiet-round misses do not.  Rounds and pixels walked are asserted equal to the as-is schedule's only where no walk
reaches the second tier (nothing waits for a blocker, nothing fills).

A failure names its (order, seed, width): at width 1 that is a deterministic reproducer.

Time on the MI355X: the module's eighteen cases 3.7 s, the oracle's answers (once a frame) included.  The slowest case is the
quiet rounds' pair at 480x270, 1.45 s for its ten schedules (0.27 s a schedule at width 7); the second tier's ramp 0.53 s
(88 ms a serial schedule), the serial 333x190 cases 13 ms a schedule and 0.14 s a case (no permutation seed had to go), a
storage hook's 800x450 frame 0.19 s.
"""
import time

import pytest

import test_gpu_flood_prologue as P

pytestmark = pytest.mark.gpu

ORDERS = ((0, 0), (1, 0), (2, 1), (2, 2), (2, 3))  # (order, permutation seed): as is, reversed, three permutations


def _schedules(widths=(0, 7, 1), orders=ORDERS):
    return [(o, s, w) for w in widths for o, s in orders]


ALL = _schedules()
WIDE = _schedules(widths=(0, 7))  # 480x270: a serial round over lists of thousands of entries would make the case slow
PERMUTED_SERIAL = (2, 1, 1)


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
    c.set_flood_schedule(0, 0, 0)
    c.close()


def _under(L, ctx, frames, schedules):
    """frames: [(key, img), ...], run in that order on the one context under each schedule (the hook stays set for all of
    them).  Returns {schedule: [counters per frame]}; every schedule runs, and the failures are reported together."""
    used, failures = {}, []
    try:
        for sch in schedules:
            ctx.set_flood_schedule(*sch)
            hooked = sch[0] != 0 or sch[2] != 0
            t0 = time.perf_counter()
            try:
                row = []
                for key, img in frames:
                    u = P._check_frame(L, ctx, key, img)
                    assert (u["scheduled_rounds"] > 0) == hooked, (key, u)
                    row.append(u)
                used[sch] = row
                print("schedule (order %d, seed %d, width %d): %.0f ms; %s" % (sch + ((time.perf_counter() - t0) * 1e3,
                      [{k: u[k] for k in ("seeds", "flood_rounds", "walked_px", "scheduled_rounds", "second_tier_seeds", "slabs",
                                          "ordered_tail_seeds", "log_rewalks", "log_give_ups", "quiet_round_misses", "dead_seeds")}
                       for u in row])))
            except AssertionError as e:
                failures.append("schedule (order, seed, width) = %s: %s" % (sch, str(e)[:600]))
    finally:
        ctx.set_flood_schedule(0, 0, 0)
    assert not failures, "%d of %d schedules failed:\n%s" % (len(failures), len(schedules), "\n".join(failures))
    return used


# ---- frame geometry -----------------------------------------------------------------------------------------------------
# (the sizes of test_gpu_flood_prologue.py: one tile, exactly a tile, partial tiles, widths that are no multiple of 4; lists of
# 0 or 1 entries at 5x5 -- the permutation's smallest lengths -- up to 1 514 at 333x190)
@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("size", P.GEOMETRY, ids=lambda s: "%dx%d" % s)
def test_frame_geometry_under_every_schedule(L, ctx, size, seed):
    w, h = size
    used = _under(L, ctx, [(("random", w, h, seed), P._random_frame(w, h, seed))], ALL)
    if (w, h, seed) == (333, 190, 0):
        # dead seeds over several rounds (test_seeds_dead_at_their_pixel): the zero sizes are the oracle's, so they are there
        # under every schedule; no walk of this frame reaches the second tier, so the rounds are the same too
        asis = used[(0, 0, 0)][0]
        assert asis["dead_seeds"] > 0 and asis["flood_rounds"] >= 2 and asis["second_tier_seeds"] == 0, asis
        for sch, (u,) in used.items():
            assert u["dead_seeds"] == asis["dead_seeds"] and u["flood_rounds"] == asis["flood_rounds"], (sch, u, asis)


# ---- one frame per branch ---------------------------------------------------------------------------------------------
def test_partial_commits_that_change_the_walk_under_every_schedule(L, ctx):
    """`synth.frame(160, 90, 70)`: fewer pixels walked with the partial commits than without (as is).  No walk of the frame
    reaches the second tier and no list fills, so every round's outcome is a function of the labels at its start: the pixels
    walked are the as-is schedule's under every schedule, with the partial commits and without."""
    from librectify_amd import synth

    img = synth.frame(160, 90, 70)
    walked = {}
    try:
        for on in (True, False):
            ctx.set_flood_partial_commits(on)
            walked[on] = _under(L, ctx, [(("bars", 160, 90, 70), img)], ALL)
    finally:
        ctx.set_flood_partial_commits(True)
    asis = {on: walked[on][(0, 0, 0)][0] for on in (True, False)}
    assert asis[True]["walked_px"] < asis[False]["walked_px"], asis
    assert asis[True]["second_tier_seeds"] == 0 and asis[False]["second_tier_seeds"] == 0, asis
    for on in (True, False):
        for sch, (u,) in walked[on].items():
            assert u["walked_px"] == asis[on]["walked_px"] and u["flood_rounds"] == asis[on]["flood_rounds"], (on, sch, u, asis[on])


@pytest.mark.parametrize("name", ("long_bars", "regions"))
def test_rewalks_from_logs_under_every_schedule(L, ctx, name):
    """`synth.long_bar_frame(240, 135, 3, K=6)` and `synth.region_frame(160, 90, 4)`.  Whether a seed turns to its log is its
    own walk's business (a log of its last finished walk, a budget of tiles), and the re-walk list holds 8 192 entries against
    some dozens here: re-walks under every schedule.  Then every log through the fall-back path (set_flood_logs(2)) on the
    permuted serial schedule."""
    from librectify_amd import synth

    img = synth.long_bar_frame(240, 135, 3, K=6) if name == "long_bars" else synth.region_frame(160, 90, 4)
    used = _under(L, ctx, [((name, "logs"), img)], ALL)
    asis = used[(0, 0, 0)][0]
    assert asis["log_rewalks"] > 0 and asis["log_give_ups"] == 0, asis
    if name == "regions":
        assert asis["flood_rounds"] >= 4, asis
    for sch, (u,) in used.items():
        assert u["log_rewalks"] > 0 and u["log_give_ups"] == 0, (sch, u)
    try:
        ctx.set_flood_logs(2)
        (u,) = _under(L, ctx, [((name, "logs"), img)], [PERMUTED_SERIAL])[PERMUTED_SERIAL]
    finally:
        ctx.set_flood_logs(1)
    assert u["log_give_ups"] == u["log_rewalks"] > 0, u  # (the hook: every log the slow way)


def test_hand_over_to_the_second_tier_under_every_schedule(L, ctx):
    """`synth.ramp_frame(160, 90, 5)`: a walk outgrows the first tier's table whatever runs beside it, and 117 such walks are far
    from the 8 192 the second tier's list holds (which seeds find THAT list full would depend on arrival): second-tier walks
    and no ordered tail under every schedule.  Their number is not asserted equal: a seed whose long walk was blocked waits for
    its blocker, and the survivors pass may see the blocker's state of the same pass or of the one before."""
    from librectify_amd import synth

    used = _under(L, ctx, [(("ramp", 160, 90, 5), synth.ramp_frame(160, 90, 5))], ALL)
    for sch, (u,) in used.items():
        assert u["second_tier_seeds"] > 0 and u["ordered_tail_seeds"] == 0, (sch, u)


def test_the_calm_hints_quiet_rounds_under_every_schedule(L, ctx):
    """The path of the recorded mismatch (docs/jpeg_decode_bounds.md): a calm frame of bars, then `synth.region_frame(480, 270,
    500)` on the same context, whose blind rounds go without the second tier's launch; the hook is set for both frames.  Widths 0
    and 7 only.  A walk that outgrows the first tier in a quiet round does so whatever the schedule, so the misses are there
    under every schedule (408 under each of the ten); how many walks reach the second tier afterwards depends on who got a log
    while the log buffer had room (see the module's text), so that count is only held above zero."""
    from librectify_amd import synth

    frames = [(("calm", 480, 270), synth.frame(480, 270, 4, bars=8)), (("regions", 480, 270, 500), synth.region_frame(480, 270, 500))]
    used = _under(L, ctx, frames, WIDE)
    for sch, (calm, regions) in used.items():
        assert calm["second_tier_seeds"] == 0 and calm["quiet_round_misses"] == 0, (sch, calm)
        assert regions["quiet_round_misses"] > 0 and regions["second_tier_seeds"] > 0, (sch, regions)


@pytest.mark.parametrize("mode", (6, 7))
def test_storage_hooks_under_a_permuted_serial_schedule(L, ctx, mode):
    """The long bars of test_flood_storage_hooks_on_bars_and_long_bars_equal_the_oracle (`synth.long_bar_frame(W, H, 3, K=24)`,
    there at 1920x1080) at the smallest size at which the hooks do anything: 800x450 has one walk of the second tier that
    outgrows the 200 tiles the hooks leave its team (none at 640x360 and below; the test's other frame, `synth.frame(W, H, 7)`,
    has no walk in the second tier at any size up to 1920x1080, so the hooks change nothing on it).  Mode 6: the team moves
    into a slab (slabs: 1).  Mode 7: there is no slab, the walk counts as unfinished under a barrier and comes back to the
    second tier in the next round (hand-overs to the second tier: 2 against 1 in the default mode).  Both under the permuted
    serial schedule (order 2, seed 1, width 1), 49 ms of flood; the modes have no waiting line (it belongs to the default
    mode's rule for giants), so the counters are the as-is schedule's."""
    from librectify_amd import synth

    key, img = ("long_bars", 800, 450, 3, 24), synth.long_bar_frame(800, 450, 3, K=24)
    try:
        ctx.set_flood_mode(1)
        plain = P._check_frame(L, ctx, key, img)
        assert plain["scheduled_rounds"] == 0 and plain["slabs"] == 0, plain
        ctx.set_flood_mode(mode)
        (u,) = _under(L, ctx, [(key, img)], [PERMUTED_SERIAL])[PERMUTED_SERIAL]
    finally:
        ctx.set_flood_mode(1)
    if mode == 6:
        assert u["slabs"] > 0 and u["ordered_tail_seeds"] == 0, u
    else:
        assert u["slabs"] == 0 and u["second_tier_seeds"] > plain["second_tier_seeds"] > 0, (u, plain)


def test_the_lanes_of_a_batch_call_ignore_the_hook(L, ctx):
    """include/librectify_amd.h: the hook is for single calls and stage calls.  With a permuted serial schedule set, a batch call
    of three small frames over two lanes gives the oracle's records, and the caller's own context -- lane 0 of the call --
    has enqueued no round under the hook; the single call behind it has."""
    import numpy as np

    from librectify_amd import synth

    frames = np.stack([synth.frame(160, 90, 70 + i) for i in range(3)])
    try:
        ctx.set_seed(0)
        ctx.find_line_segment_groups(frames[0], 1.6)  # (as is: the counter starts from 0 whatever ran before)
        ctx.set_flood_schedule(*PERMUTED_SERIAL)
        ctx.set_batch_streams(2)
        out, n, _ = ctx.find_line_segment_groups_batch_host(frames, 1.6, num_threads=2, capacity=1024)
        assert ctx.stage_counters()["scheduled_rounds"] == 0, ctx.stage_counters()
        for b in range(3):
            P._assert_lines_equal(out[b][: n[b]], P._reference(("bars", 160, 90, 70 + b), frames[b])[1])
        ctx.find_line_segment_groups(frames[0], 1.6)
        assert ctx.stage_counters()["scheduled_rounds"] > 0, ctx.stage_counters()
    finally:
        ctx.set_flood_schedule(0, 0, 0)
        ctx.set_batch_streams(5)  # (the default)
