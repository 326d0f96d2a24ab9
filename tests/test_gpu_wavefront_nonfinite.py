"""One non-finite feature through the four entry points of the DTW wavefront -- ssym_dtw_spot / ssym_spot_queries,
ssym_dtw_spot_all, the spotter, ssym_dtw_align -- against the restatements, which state the oracle's comparison order
(dtw_path_ref.min3).  The cases and what the restatements make of them are tests/nonfinite_cases.py's; that the cases are
not vacuous is asserted without a device in tests/test_wavefront_nonfinite_ref.py.  Floats are compared by NaN mask and
then bit for bit: a NaN's sign and payload are the processor's own.  Outputs are sentinel-filled where the call is made
through ctypes."""
import numpy as np
import pytest

import nonfinite_cases as nc
from dtw_path_ref import same_floats
from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments
from test_gpu_watch import NO, _W, _check_split

pytestmark = pytest.mark.gpu


def _sets(e, src, tgt, dim):
    sf, so = pack_segments(src, dim)
    tf, to = pack_segments(tgt, dim)
    return e.dictionary(sf, so, dim), e.queries(tf, to, dim)


@pytest.mark.parametrize("case", nc.CASES, ids=nc.ident)
def test_spot_spot_queries_spot_all_and_align(case):
    c = nc.get(case)
    e = Engine(metric="dtw", dtype="f64", squared=c.squared)
    d, q = _sets(e, c.sources, c.targets, c.dim)
    si, ti = np.repeat(np.arange(2, dtype=np.uint32), 2), np.tile(np.arange(2, dtype=np.uint32), 2)

    # ssym_dtw_spot: NaN never wins, +inf never wins
    cost, start, end = e.dtw_spot(d, q, si, ti)
    for p in range(4):
        want = c.spot(int(si[p]), int(ti[p]))
        assert same_floats(cost[p], want[0]) and (int(start[p]), int(end[p])) == want[1:], (p, cost[p], start[p], end[p], want)
    # ssym_spot_queries: the fold over the poisoned and the clean source
    idx, cost, start, end = e.spot_queries(d, q)
    for t in range(2):
        want = c.spot_best(t)
        assert (int(idx[t]), int(start[t]), int(end[t])) == (want[0], want[2], want[3]) and same_floats(cost[t], want[1]), (t, want)

    # ssym_dtw_spot_all, K = 4: counts, spans, padding
    count, cost, start, end = e.dtw_spot_all(d, q, si, ti, max_spots=nc.K)
    for p in range(4):
        want = c.spot_all(int(si[p]), int(ti[p]))
        assert int(count[p]) == want[0], (p, count[p], want[0])
        assert same_floats(cost[p], want[1]) and not np.isnan(cost[p]).any(), (p, cost[p], want[1])
        assert np.array_equal(start[p], want[2]) and np.array_equal(end[p], want[3]), (p, start[p], end[p], want)
        assert np.isposinf(cost[p, want[0]:]).all() and (end[p, want[0]:] == NO).all()

    # ssym_dtw_align on plain pairs cut from the same data
    src, tgt, pairs = c.plain_pairs()
    d2, q2 = _sets(e, src, tgt, c.dim)
    cost, length, paths, maps = e.dtw_align(d2, q2, [s for s, _ in pairs], [t for _, t in pairs])
    finite = 0
    for p, (s, t) in enumerate(pairs):
        want_cost, want_path, want_map = c.align(src[s], tgt[t])
        assert np.isnan(cost[p]) == np.isnan(want_cost) and same_floats(cost[p], want_cost), (p, cost[p], want_cost)
        assert int(length[p]) == want_path.shape[0], (p, length[p])
        assert np.array_equal(paths[p].astype(np.int64), want_path) and np.array_equal(maps[p].astype(np.int64), want_map), p
        if not np.isfinite(want_cost):
            assert length[p] == 0 and paths[p].shape[0] == 0 and maps[p].size == 0 and not np.isfinite(cost[p])
        finite += int(np.isfinite(want_cost))
    assert 1 <= finite < len(pairs)                       # both branches are taken in every case
    e.close()


@pytest.mark.parametrize("case", nc.CASES, ids=nc.ident)
def test_spotter(case):
    c = nc.get(case)
    prof = {(0, t): c.profile(0, t) for t in range(2)}
    for cuts in (nc.PUSHES, c.cuts_around()):
        w = _W(c.targets, c.dim, squared=c.squared)
        _check_split(w, [c.sources[0]], [cuts], prof)     # profile (mask, then bits), events, best, flush
        cost, start, end = w.sp.best()
        for t in range(2):
            want = c.spot(0, t)
            assert same_floats(cost[0, t], want[0]) and (int(start[0, t]), int(end[0, t])) == want[1:]
        w.close()


def test_one_frame_target_lives_again_after_a_nan_row_where_two_frames_do_not():
    """The difference DESIGN.md states: column 0 restarts in every row, every other column takes the NaN from `up`."""
    rng = np.random.default_rng(0x1F2)
    dim = 13
    lane = rng.standard_normal((130, dim)).astype(np.float32).astype(np.float64)
    lane[64, dim - 1] = np.nan
    tgt = [lane[100:101].copy(), lane[100:102].copy()]
    w = _W(tgt, dim, max_cost=0.0)
    rc, n, pd, ps, _ = w.push([lane])
    assert rc == nat.SSYM_OK
    one, two = pd[0][0], pd[0][1]
    assert np.isnan(one[64]) and np.isfinite(np.delete(one, 64)).all() and one[100] == 0.0
    assert np.isfinite(two[:64]).all() and np.isnan(two[64:]).all()
    w.sp.flush(0)
    cost, start, end = w.sp.best()
    assert (cost[0, 0], int(start[0, 0]), int(end[0, 0])) == (0.0, 100, 100) and end[0, 1] < 64 and np.isfinite(cost[0, 1])
    w.close()
    w = _W(tgt, dim, max_cost=0.0)
    _check_split(w, [lane], [[0, 64, 65, 66, 130]])
    w.close()
