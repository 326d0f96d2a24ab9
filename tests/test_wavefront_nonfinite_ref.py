"""What the restatements make of the cases of tests/test_gpu_wavefront_nonfinite.py (tests/nonfinite_cases.py), without
a device: the conditions that keep the GPU file from passing vacuously, and the behaviour DESIGN.md section 2 states for
a non-finite feature.  A NaN source frame ends spotting for the rest of the source when the target has two or more frames
(`up` carries the NaN down) and costs a one-frame target that row alone; a NaN target frame leaves no end at all; +-inf
and an overflowing value cost the row (or every end, in a target) and nothing else."""
import numpy as np
import pytest

import nonfinite_cases as nc
from dtw_path_ref import cumulative_loop, local_costs, same_floats
from spot_ref import NO_MATCH

NONE = (nc.INF, NO_MATCH, NO_MATCH)
SRC_CASES = [c for c in nc.CASES if c[3] == "src"]
TGT_CASES = [c for c in nc.CASES if c[3] == "tgt"]


def _picks(case, s, t):
    count, cost, start, end = case.spot_all(s, t)
    assert np.isinf(cost[count:]).all() and (start[count:] == NO_MATCH).all() and (end[count:] == NO_MATCH).all()
    return [(float(cost[m]), int(start[m]), int(end[m])) for m in range(count)]


def _events(case, t, cuts=nc.PUSHES):
    per_push, bests, flushed, _ = case.watch(t, cuts)
    return [e for evs in per_push for e in evs] + flushed[len(cuts) - 2], bests[-1]


@pytest.mark.parametrize("case", SRC_CASES, ids=nc.ident)
def test_a_poisoned_source_row(case):
    c = nc.get(case)
    r, nan = c.frame, np.isnan(c.value)
    delta, _ = c.profile(0, 0)
    one, _ = c.profile(0, 1)
    plants = [(0.0,) + p for p in nc.PLANTS]
    picks, picks_one = _picks(c, 0, 0), _picks(c, 0, 1)
    events, best = _events(c, 0)
    events_one, _ = _events(c, 1)
    assert all(np.isfinite(x[0]) for x in picks + picks_one + events + events_one)
    # something real is found in every case: the test cannot pass on "none" everywhere.  (A NaN in row 0 leaves the
    # 70-frame target no end at all, by the definition; there the one-frame target is what is found.)
    assert len(picks) + len(events) >= 1 or (nan and r == 0 and len(picks_one) + len(events_one) >= 1)
    assert len(picks_one) == nc.K and len(events_one) >= 1
    if nan:
        # the row and every later end are NaN, no span reaches the row, and the plants before it are found
        assert np.isnan(delta[r:]).all() and np.isfinite(delta[:r]).all()
        assert all(x[2] < r for x in picks + events) and best == c.spot(0, 0)
        assert [p for p in plants if p[2] < r] == [p for p in picks if p[0] == 0.0] == [e for e in events if e[0] == 0.0]
        assert (len(picks) >= 1) == (r > 0) and (c.spot(0, 0) == NONE) == (r == 0)
        # one frame: column 0 restarts, the rows after the NaN are alive again
        assert np.isnan(one[r]) and np.isfinite(np.delete(one, r)).all()
        assert r == 129 or any(x[2] > r for x in picks_one) and any(x[2] > r for x in events_one)
    else:
        # +inf in the row and nowhere else: both plants are found, the one behind the row included
        for d in (delta, one):
            assert np.isposinf(d[r]) and np.isfinite(np.delete(d, r)).all()
        assert picks[:2] == plants and [e for e in events if e[0] == 0.0] == plants
        assert c.spot(0, 0) == plants[0] and best == plants[0]
    # one frame at a time around the row: the same events, whatever the cuts
    assert _events(c, 0, c.cuts_around())[0] == events and _events(c, 1, c.cuts_around())[0] == events_one
    # the fold over sources prefers the clean second source exactly when the NaN has cost the poisoned one its plants
    assert c.spot_best(0)[0] == (1 if nan and r < nc.PLANTS[0][1] else 0) and np.isfinite(c.spot_best(0)[1])
    # plain pairs: the cut that holds the row has no finite cost, the clean ones have
    src, tgt, pairs = c.plain_pairs()
    for s, t in pairs:
        cost, path, fmap = c.align(src[s], tgt[t])
        assert np.isfinite(cost) == (s != 0) and (path.shape[0] > 0) == (s != 0)
        if s == 0:
            assert np.isnan(cost) == nan and (nan or np.isposinf(cost))
    assert c.align(src[1], tgt[0])[0] == 0.0


@pytest.mark.parametrize("case", TGT_CASES, ids=nc.ident)
def test_a_poisoned_target_column(case):
    c = nc.get(case)
    j, nan = c.frame, np.isnan(c.value)
    for s in (0, 1):
        delta, _ = c.profile(s, 0)
        # NaN only where the last column itself holds the value; +inf everywhere else -- never a finite end
        assert np.isnan(delta).all() if nan and j == 69 else np.isposinf(delta).all()
        assert c.spot(s, 0) == NONE and _picks(c, s, 0) == []
        assert np.isfinite(c.profile(s, 1)[0]).all()                     # the clean one-frame target is untouched
    events, best = _events(c, 0)
    assert events == [] and best == NONE and _events(c, 0, c.cuts_around()) == ([], NONE)
    assert c.spot_best(0) == (NO_MATCH,) + NONE and c.spot_best(1)[0] != NO_MATCH
    src, tgt, pairs = c.plain_pairs()
    for s, t in pairs:
        cost, path, fmap = c.align(src[s], tgt[t])
        assert np.isfinite(cost) == (t == 1) and (path.shape[0] > 0) == (t == 1)
        if t == 0:
            # plain DTW: column 0 accumulates, so a NaN in it runs down `up`; the last cell is NaN if the last column
            # holds the value or row 0 carries it there, else +inf
            assert np.isnan(cost) or np.isposinf(cost)
            assert nan or np.isposinf(cost)


def test_a_best_span_lies_strictly_after_the_poisoned_row():
    seen = 0
    for case in SRC_CASES:
        c = nc.get(case)
        if not np.isnan(c.value):
            cost, start, end = c.spot(0, 0)
            seen += int(end != NO_MATCH and start > c.frame)
    assert seen >= 1, seen


def test_the_comparison_order_is_exercised():
    """Over the cases: profile entries that are NaN in the restatement, and entries that are +inf where np.minimum would
    have given NaN -- and both are what the cell-by-cell loop in the oracle's order gives."""
    nans = infs_where_minimum_had_nan = 0
    for case in nc.CASES:
        c = nc.get(case)
        if not np.isnan(c.value) or c.dim != nc.DIMS[0]:
            continue
        delta, _ = c.profile(0, 0)
        old = nc.profile_np_minimum(c.sources[0], c.targets[0], c.squared)
        loop = cumulative_loop(local_costs(c.sources[0], c.targets[0], c.squared), free_start=True)[:, -1]
        assert np.array_equal(np.isnan(delta), np.isnan(loop)) and same_floats(delta, loop), nc.ident(case)
        nans += int(np.count_nonzero(np.isnan(delta)))
        infs_where_minimum_had_nan += int(np.count_nonzero(np.isposinf(delta) & np.isnan(old)))
    assert nans >= 1 and infs_where_minimum_had_nan >= 1, (nans, infs_where_minimum_had_nan)
