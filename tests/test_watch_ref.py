"""The watching restatement (tests/watch_ref.py) against itself and against brute force, without a device: split
invariance, the consequences (3) - (5) of DESIGN.md section 2 "Watching", and the planted-copies case in which the causal
rule and ssym_dtw_spot_all's greedy agree.  Every detection case asserts that the rule was exercised: at least 3 events,
a replacement in step 3, and a candidate rejected by `last`.  (s(i) came out non-decreasing in every trial, and then a
candidate can only be rejected by `last` after a flush: the cases flush in mid-stream and go on.)"""
import numpy as np
import pytest

import spot_all_ref
import watch_ref
from dtw_path_ref import local_costs

FRAMES = 200
FLUSH_ROWS = (70, 140, FRAMES)           # the lane is flushed after these many rows, and goes on
CASES = [("int", 0, None), ("int", 1, 0.3), ("int", 3, 0.3), ("real", 0, None), ("real", 1, None), ("real", 5, None)]


def _case(kind, seed):
    rng = np.random.default_rng(0x3A7C0 + seed)
    fb, dim = int(rng.integers(3, 12)), 3
    if kind == "int":
        return rng.integers(0, 3, size=(FRAMES, dim)).astype(float), rng.integers(0, 3, size=(fb, dim)).astype(float), True
    return rng.standard_normal((FRAMES, dim)), rng.standard_normal((fb, dim)), False


def _cuts(step_or_list):
    """Cuts that contain every flush row: a fixed step, or a given list."""
    base = list(range(0, FRAMES, step_or_list)) if isinstance(step_or_list, int) else list(step_or_list)
    return sorted(base + list(FLUSH_ROWS))           # (a flush row that a step also hits: an empty push)


def _run(delta, s, cuts, limit):
    """{rows consumed when emitted: events} with flush events keyed (rows, 'flush'), and the best by rows consumed."""
    flush_after = {p for p in range(len(cuts) - 1) if cuts[p + 1] in FLUSH_ROWS and (p + 2 == len(cuts) or cuts[p + 2] != cuts[p + 1])}
    per_push, bests, flushed, rep = watch_ref.drive(delta, s, cuts, limit, flush_after)
    return per_push, bests, flushed, rep, flush_after


def _timeline(delta, s, cuts, limit):
    """Every event with the number of rows consumed when it was emitted (flush events marked), and the best by rows."""
    per_push, bests, flushed, rep, _ = _run(delta, s, cuts, limit)
    events, best_at = [], {}
    for p in range(len(cuts) - 1):
        events += [(ev, "push") for ev in per_push[p]]
        best_at[cuts[p + 1]] = bests[p]
        events += [(ev, "flush", cuts[p + 1]) for ev in flushed.get(p, [])]
    return events, best_at, rep


@pytest.mark.parametrize("kind,seed,quantile", CASES)
def test_split_invariance_and_the_consequences(kind, seed, quantile):
    a, b, squared = _case(kind, seed)
    delta, s = watch_ref.whole_profile(a, b, squared)
    limit = None if quantile is None else float(np.quantile(delta, quantile))
    whole_events, whole_best, rep = _timeline(delta, s, _cuts(FRAMES), limit)
    st = rep.stats
    assert st["events"] >= 3 and st["replaced"] >= 1 and st["rejected_by_last"] >= 1, st        # nothing vacuous
    rng = np.random.default_rng(seed)
    random_cuts = np.sort(rng.integers(0, FRAMES + 1, size=30)).tolist()
    random_cuts = [0] + random_cuts[:10] + random_cuts[9:11] + random_cuts[10:] + [FRAMES]        # with empty pushes
    for cuts in (_cuts(1), _cuts(63), _cuts(64), _cuts(65), _cuts(random_cuts)):
        events, best_at, _ = _timeline(delta, s, cuts, limit)
        assert [e[0] for e in events] == [e[0] for e in whole_events]
        assert [e[1:] for e in events if e[1] == "flush"] == [e[1:] for e in whole_events if e[1] == "flush"]
        for rows, best in best_at.items():                     # the best after n rows: spot_ref's rule on the prefix
            want = (np.inf, watch_ref.NO_MATCH, watch_ref.NO_MATCH)
            if rows:
                end = int(np.argmin(delta[:rows]))
                want = (float(delta[end]), int(s[end]), end)
            assert best == want
    # (6) an event is emitted by the push that consumes the first row i with s(i) > pend.end: one frame at a time, the
    # rows consumed at emission name that row
    cuts = _cuts(1)
    per_push, _, flushed, _, _ = _run(delta, s, cuts, limit)
    for p, evs in enumerate(per_push):
        for cost, start, end in evs:
            i = cuts[p + 1] - 1
            assert s[i] > end and not (s[end + 1:i] > end).any()
    # (3) disjoint spans, ascending ends
    spans = [e[0] for e in whole_events]
    for (c0, s0, e0), (c1, s1, e1) in zip(spans, spans[1:]):
        assert s0 <= e0 < s1 <= e1
    # (4) every cost is the plain DTW cost of its cut, by brute force
    for cost, start, end in spans:
        c = local_costs(a[start:end + 1], b, squared)
        D = np.full((c.shape[0] + 1, c.shape[1] + 1), np.inf)
        D[0, 0] = 0.0
        for i in range(c.shape[0]):
            for j in range(c.shape[1]):
                D[i + 1, j + 1] = c[i, j] + min(D[i, j + 1], D[i + 1, j], D[i, j])
        assert np.float64(cost).view(np.uint64) == np.float64(D[-1, -1]).view(np.uint64)
    # (5) of a run of overlapping candidates the first least is reported: between two emissions, the rows that were
    # candidates hold no smaller cost than the event's, and none equal to it at a smaller end
    last, lo = None, 0
    bound = np.inf if limit is None else limit
    for ev in whole_events:
        cost, start, end = ev[0]
        hi = ev[2] if ev[1] == "flush" else int(np.argmax((s > end) & (np.arange(FRAMES) > end)))   # rows lo ... hi - 1 competed
        cand = [i for i in range(lo, hi) if np.isfinite(delta[i]) and delta[i] <= bound and (last is None or s[i] > last)]
        assert cand and min(delta[i] for i in cand) == cost and min(i for i in cand if delta[i] == cost) == end
        last, lo = end, hi


def test_planted_copies_agree_with_the_offline_greedy():
    rng = np.random.default_rng(0x91A7)
    tgt = rng.integers(1, 4, size=(6, 3)).astype(float)
    rec = rng.integers(5, 9, size=(150, 3)).astype(float)            # noise that no target frame equals
    for at in (10, 50, 90, 144):
        rec[at:at + 6] = tgt
    delta, s = watch_ref.whole_profile(rec, tgt, True)
    per_push, _, flushed, rep = watch_ref.drive(delta, s, [0, 40, 40, 99, 150], 1e-9, flush_after=(3,))
    events = [e for evs in per_push for e in evs] + flushed[3]
    picks = sorted(spot_all_ref.select(delta, s, 8, 1e-9), key=lambda x: x[2])
    assert events == picks and [e[1:] for e in events] == [(10, 15), (50, 55), (90, 95), (144, 149)]
    assert [len(x) for x in per_push] == [1, 0, 1, 1] and len(flushed[3]) == 1      # the last plant waits for the flush


def test_the_rule_is_not_the_offline_greedy():
    # a cheap span that overlaps one already emitted is rejected, where the greedy would prefer it
    delta = np.array([5.0, 4.0, 9.0, 1.0, 9.0])
    s = np.array([0, 0, 2, 1, 4])
    per_push, _, flushed, rep = watch_ref.drive(delta, s, [0, 5], None, flush_after=(0,))
    assert per_push[0] == [(4.0, 0, 1), (9.0, 2, 2)] and flushed[0] == [(9.0, 4, 4)]
    assert (1.0, 1, 3) not in per_push[0] + flushed[0] and rep.stats["rejected_by_last"] >= 1
    assert spot_all_ref.select(delta, s, 1)[0] == (1.0, 1, 3)


def test_a_target_without_frames_and_an_empty_lane():
    per_push, bests, flushed, rep = watch_ref.watch(np.zeros((5, 2)), np.zeros((0, 2)), [0, 3, 5], flush_after=(1,))
    assert per_push == [[], []] and flushed == {1: []} and bests[-1] == (np.inf, watch_ref.NO_MATCH, watch_ref.NO_MATCH)
    per_push, bests, flushed, _ = watch_ref.watch(np.zeros((0, 2)), np.zeros((3, 2)), [0, 0], flush_after=(0,))
    assert per_push == [[]] and flushed == {0: []}


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf"), 1e200])
def test_a_non_finite_frame_in_the_lane_or_the_target(value):
    """whole_profile is the end column of the cell-by-cell loop in the oracle's comparison order (NaN mask, then bits);
    neither NaN nor +inf is ever a candidate or a best, however the lane is cut."""
    from dtw_path_ref import cumulative_loop, same_floats
    for kind, seed in (("real", 0), ("int", 1)):
        a0, b0, squared = _case(kind, seed)
        delta0, _ = watch_ref.whole_profile(a0, b0, squared)
        assert same_floats(delta0, cumulative_loop(local_costs(a0, b0, squared), free_start=True)[:, -1])
        for side, frame in (("src", 0), ("src", 100), ("src", FRAMES - 1), ("tgt", 0), ("tgt", b0.shape[0] - 1)):
            a, b = a0.copy(), b0.copy()
            (a if side == "src" else b)[frame, 1] = value
            delta, s = watch_ref.whole_profile(a, b, squared)
            loop = cumulative_loop(local_costs(a, b, squared), free_start=True)[:, -1]
            assert np.array_equal(np.isnan(delta), np.isnan(loop)) and same_floats(delta, loop)
            runs = [watch_ref.drive(delta, s, cuts, None, flush_after=(len(cuts) - 2,)) for cuts in ([0, FRAMES], list(range(FRAMES + 1)))]
            events = [[e for evs in r[0] for e in evs] + r[2][len(r[0]) - 1] for r in runs]
            assert events[0] == events[1] and all(np.isfinite(e[0]) for e in events[0])
            best = runs[1][1][-1]
            if side == "tgt":
                assert events[0] == [] and best == (np.inf, watch_ref.NO_MATCH, watch_ref.NO_MATCH)
                assert np.isnan(delta).all() if np.isnan(value) and frame else np.isposinf(delta).all()
            elif np.isnan(value):
                assert np.isnan(delta[frame:]).all() and all(e[2] < frame for e in events[0]) and (len(events[0]) >= 1) == (frame > 0)
            else:
                assert np.isposinf(delta[frame]) and np.isfinite(np.delete(delta, frame)).all()
                assert frame == FRAMES - 1 or any(e[1] > frame for e in events[0])
                assert same_floats(np.delete(delta, frame)[:frame], delta0[:frame])
