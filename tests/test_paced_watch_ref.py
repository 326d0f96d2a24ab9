"""The paced watching restatement (tests/paced_watch_ref.py) on the CPU: planted copies at the three slopes of the pattern
are reported at their spans at cost 0.0 however the lane is cut, the events are paced_ref.spot_all's picks and keep the
slope bounds; on integer frames, where ties are real, every cut gives the whole's events; a NaN source frame costs a
bounded stretch under the paced pattern and the rest of the lane under the symmetric one."""
import numpy as np
import pytest

import paced_ref
import paced_watch_ref
import spot_all_ref
import watch_ref

UNEVEN = [0, 3, 3, 51, 66, 67, 120, 131, 200, 301, 305, 306, 400]            # 12 pushes, one of them empty
CUTS = {"whole": [0, 400], "uneven": UNEVEN, "ones": list(range(401))}


def _events(per_push, flushed):
    return [e for evs in per_push for e in evs] + [e for p in sorted(flushed) for e in flushed[p]]


@pytest.fixture(scope="module")
def planted():
    return paced_watch_ref.planted()


@pytest.mark.parametrize("cut", list(CUTS))
def test_planted_copies_are_reported_at_their_spans_at_cost_zero(planted, cut):
    lane, targets, spans = planted
    for t, b in enumerate(targets):
        fb = b.shape[0]
        cuts = CUTS[cut]
        per_push, bests, flushed, rep = paced_watch_ref.watch(lane, b, cuts, max_cost=1e-9 * fb, flush_after=(len(cuts) - 2,))
        got = _events(per_push, flushed)
        assert got == [spans[t]]
        # ... which is the offline pick of the same profile, and the best
        n, cost, start, end = paced_ref.spot_all(lane, b, 4, max_cost=1e-9 * fb)
        picks = sorted(((float(cost[k]), int(start[k]), int(end[k])) for k in range(int(n))), key=lambda e: e[2])
        assert got == picks and bests[-1] == spans[t] == paced_ref.spot(lane, b)
        lo, hi = paced_ref.span_bounds(fb)
        assert all(lo <= e - s + 1 <= hi for _, s, e in got)
    assert [s[2] - s[1] + 1 for s in spans] == [2 * 9 - 1, 11, 10 // 2]       # the three slopes


def test_the_push_that_emits_an_event_does_not_depend_on_the_cuts(planted):
    lane, targets, _ = planted
    for b in targets:
        ones = paced_watch_ref.watch(lane, b, CUTS["ones"], max_cost=1e-9 * b.shape[0])[0]
        row = {e: p for p, evs in enumerate(ones) for e in evs}              # with one-frame pushes: push p consumes row p
        for cuts in (CUTS["whole"], UNEVEN):
            per_push = paced_watch_ref.watch(lane, b, cuts, max_cost=1e-9 * b.shape[0])[0]
            for p, evs in enumerate(per_push):
                assert all(cuts[p] <= row[e] < cuts[p + 1] for e in evs)
            assert sum(len(v) for v in per_push) == len(row) == 1


def test_integer_frames_every_cut_gives_the_whole_and_ties_are_real():
    rng = np.random.default_rng(0x17E6)
    lane = rng.integers(0, 3, size=(300, 3)).astype(np.float64)
    cut_lists = [[0, 300], list(range(301)), [0, 1, 3, 64, 65, 129, 130, 130, 257, 300], list(range(0, 300, 7)) + [300]]
    replaced = 0
    for fb in range(1, 12):
        b = rng.integers(0, 3, size=(fb, 3)).astype(np.float64)
        delta, s = paced_watch_ref.whole_profile(lane, b, True)
        assert delta.shape == (300,) and np.array_equal(delta, paced_ref.profile(lane, b, True)[0])
        whole = None
        for cuts in cut_lists:
            per_push, bests, flushed, rep = watch_ref.drive(delta, s, cuts, flush_after=(len(cuts) - 2,))
            got = _events(per_push, flushed)
            whole = got if whole is None else whole
            assert got == whole and bests[-1] == paced_ref.spot(lane, b, True)
            for p in range(len(cuts) - 1):                                   # the best after a push is the prefix's spot
                assert bests[p] == paced_ref.spot(lane[:cuts[p + 1]], b, True)
        lo, hi = paced_ref.span_bounds(fb)
        assert len(whole) >= 3 and all(lo <= e - st + 1 <= hi for _, st, e in whole)
        assert all(x[2] < y[1] for x, y in zip(whole, whole[1:]))            # disjoint, ends ascending
        replaced += rep.stats["replaced"]
    assert replaced > 0


def test_a_nan_source_frame_costs_a_bounded_stretch_paced_and_the_rest_of_the_lane_symmetric():
    lane, target = paced_watch_ref.nan_case()
    fb = target.shape[0]
    delta, s = paced_watch_ref.whole_profile(lane, target)
    lo = paced_ref.span_bounds(fb)[0]
    assert np.isinf(delta[:lo - 1]).all()                                   # no path ends before the shortest span does
    # the poisoned rows: a NaN E(i-1,j-1) is kept as P (NaN fails every <), so the NaN of row 100 runs down the diagonals
    # and leaves through the end column by row 100 + Fb - 1; a NaN second diagonal or a NaN H is passed over
    bad = np.flatnonzero(~np.isfinite(delta[lo - 1:])) + lo - 1
    assert bad.size and bad.min() == 100 and bad.max() <= 100 + fb - 1
    cuts = [0, 90, 101, 102, 125, 400]
    per_push, bests, flushed, _ = watch_ref.drive(delta, s, cuts, max_cost=1e-9 * fb, flush_after=(len(cuts) - 2,))
    assert _events(per_push, flushed) == [(0.0, 120, 130)] and bests[-1] == (0.0, 120, 130)
    sym = spot_all_ref.profile(lane, target)[0]
    assert np.isfinite(sym[:100]).all() and not np.isfinite(sym[100:]).any()
    assert _events(*watch_ref.watch(lane, target, cuts, max_cost=1e-9 * fb, flush_after=(len(cuts) - 2,))[0:3:2]) == []
