"""The paced step pattern on the GPU (ssym_dtw_spot_step, ssym_spot_queries_step, ssym_dtw_spot_all_step with
SSYM_STEP_PACED) against the numpy restatement (tests/paced_ref.py), bit for bit: costs by ==, starts, ends and counts
equal.  Chunk and hand-off edges (both hand-off rows: skips that cross rows 62 -> 64 and 63 -> 65, a repeat across rows
63 and 64), ring and target edges, every DIMR and its padding, every way of listing pairs, occurrences, the symmetric
step as the old calls, the tripled target, non-finite features, and the limits.  Outputs are sentinel-filled where the
call is made through ctypes."""
import numpy as np
import pytest

import paced_ref
import spot_all_ref
from dtw_path_ref import same_floats
from soundsym_amd import HOP, Engine, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

SENT32, SENTF = 0xDEADBEEF, -12345.5
NO = nat.NO_MATCH
PACED, SYMMETRIC = nat.STEP_PACED, nat.STEP_SYMMETRIC


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class _Sets:
    """An engine with a resident dictionary and query set made from lists of [frames, dim] arrays; the restatement's
    profile of a pair is computed once."""

    def __init__(self, src, tgt, dim, squared=False, band=-1, metric="dtw"):
        self.src, self.tgt, self.dim, self.squared = src, tgt, dim, squared
        self.e = Engine(metric=metric, dtype="f64", band=band, squared=squared)
        sf, so = pack_segments(src, dim, np.float64)
        tf, to = pack_segments(tgt, dim, np.float64)
        self.d, self.q = self.e.dictionary(sf, so, dim), self.e.queries(tf, to, dim)
        self._prof = {}

    def close(self):
        self.e.close()

    def profile(self, s, t):
        if (s, t) not in self._prof:
            self._prof[(s, t)] = paced_ref.profile(np.asarray(self.src[s], np.float64), np.asarray(self.tgt[t], np.float64),
                                                   self.squared)
        return self._prof[(s, t)]

    def _empty(self, s, t):
        return self.src[s].shape[0] == 0 or self.tgt[t].shape[0] == 0

    def ref(self, s, t):
        """(cost, start, end) of the restatement."""
        if self._empty(s, t):
            return (float("inf"), NO, NO)
        delta, st = self.profile(s, t)
        end, cost = paced_ref.first_end(delta)
        return (float("inf"), NO, NO) if end == NO else (cost, int(st[end]), end)

    def ref_all(self, s, t, k, limit=None):
        """(count, cost [k], start [k], end [k]) of the restatement."""
        if self._empty(s, t):
            return spot_all_ref.padded([], k)
        return spot_all_ref.padded(spot_all_ref.select(*self.profile(s, t), k, limit), k)


def _spot(sets, src_idx, tgt_idx=None, base=0, step=PACED, device=False):
    """ssym_dtw_spot_step through ctypes into sentinel-filled outputs (one pair more than listed)."""
    src = np.ascontiguousarray(src_idx, dtype=np.uint32)
    tgt = None if tgt_idx is None else np.ascontiguousarray(tgt_idx, dtype=np.uint32)
    n = src.size
    cost = np.full(n + 1, SENTF)
    start = np.full(n + 1, SENT32, dtype=np.uint32)
    end = np.full(n + 1, SENT32, dtype=np.uint32)
    args = [sets.e.ctx, sets.d.ptr, sets.q.ptr, src.ctypes.data, None if tgt is None else tgt.ctypes.data, n, base, step]
    if device:
        import torch
        ds, de = (torch.from_numpy(x.view(np.int32)).cuda() for x in (start, end))
        dc = torch.from_numpy(cost).cuda()
        rc = nat.lib().ssym_dtw_spot_step(*args, dc.data_ptr(), ds.data_ptr(), de.data_ptr(), nat.OUT_DEVICE)
        torch.cuda.synchronize()
        start, end = (x.cpu().numpy().view(np.uint32) for x in (ds, de))
        cost = dc.cpu().numpy()
    else:
        rc = nat.lib().ssym_dtw_spot_step(*args, cost.ctypes.data, start.ctypes.data, end.ctypes.data, 0)
    return rc, cost, start, end


def _spot_all(sets, src_idx, tgt_idx=None, base=0, k=8, max_cost=None, step=PACED, device=False):
    """ssym_dtw_spot_all_step through ctypes into sentinel-filled outputs (one pair more than listed)."""
    src = np.ascontiguousarray(src_idx, dtype=np.uint32)
    tgt = None if tgt_idx is None else np.ascontiguousarray(tgt_idx, dtype=np.uint32)
    n = src.size
    count = np.full(n + 1, SENT32, dtype=np.uint32)
    cost = np.full((n + 1, k), SENTF)
    start = np.full((n + 1, k), SENT32, dtype=np.uint32)
    end = np.full((n + 1, k), SENT32, dtype=np.uint32)
    mc = None if max_cost is None else np.ascontiguousarray(max_cost, dtype=np.float64)
    args = [sets.e.ctx, sets.d.ptr, sets.q.ptr, src.ctypes.data, None if tgt is None else tgt.ctypes.data, n, base, step, k,
            None if mc is None else mc.ctypes.data]
    if device:
        import torch
        dn, ds, de = (torch.from_numpy(x.view(np.int32)).cuda() for x in (count, start, end))
        dc = torch.from_numpy(cost).cuda()
        rc = nat.lib().ssym_dtw_spot_all_step(*args, dn.data_ptr(), dc.data_ptr(), ds.data_ptr(), de.data_ptr(), nat.OUT_DEVICE)
        torch.cuda.synchronize()
        count, start, end = (x.cpu().numpy().view(np.uint32) for x in (dn, ds, de))
        cost = dc.cpu().numpy()
    else:
        rc = nat.lib().ssym_dtw_spot_all_step(*args, count.ctypes.data, cost.ctypes.data, start.ctypes.data, end.ctypes.data, 0)
    return rc, count, cost, start, end


def _untouched(out):
    return all(((x == SENTF) if x.dtype == np.float64 else (x == SENT32)).all() for x in out[1:])


def _check(sets, src_idx, tgt_idx, out, base=0):
    """Every pair of an ssym_dtw_spot_step call equal to the restatement; the entry beyond the pairs untouched; no
    reported cost is NaN, and a cost is finite exactly where a span is reported.  Returns the spans found."""
    rc, cost, start, end = out
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(sets.e.ctx)
    n = len(src_idx)
    assert cost[n] == SENTF and start[n] == SENT32 and end[n] == SENT32
    found = 0
    for p in range(n):
        t = p if tgt_idx is None else int(tgt_idx[p])
        want = (float("inf"), NO, NO) if int(src_idx[p]) == NO else sets.ref(int(src_idx[p]) - base, t)
        assert _bits(cost[p]) == _bits(want[0]) and (int(start[p]), int(end[p])) == want[1:], (p, cost[p], start[p], end[p], want)
        assert np.isfinite(cost[p]) == (int(end[p]) != NO)
        if int(end[p]) != NO:
            lo, hi = paced_ref.span_bounds(sets.tgt[t].shape[0])
            assert lo <= int(end[p]) - int(start[p]) + 1 <= hi                    # consequence 1
            found += 1
    return found


def _check_all(sets, src_idx, tgt_idx, out, k, base=0, max_cost=None):
    rc, count, cost, start, end = out
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(sets.e.ctx)
    n = len(src_idx)
    assert count[n] == SENT32 and (cost[n] == SENTF).all() and (start[n] == SENT32).all() and (end[n] == SENT32).all()
    total = 0
    for p in range(n):
        t = p if tgt_idx is None else int(tgt_idx[p])
        limit = None if max_cost is None else float(np.asarray(max_cost).reshape(-1)[p])
        want = spot_all_ref.padded([], k) if int(src_idx[p]) == NO else sets.ref_all(int(src_idx[p]) - base, t, k, limit)
        assert int(count[p]) == want[0], (p, int(count[p]), want[0])
        assert np.array_equal(_bits(cost[p]), _bits(want[1])), (p, cost[p], want[1])
        assert np.array_equal(start[p], want[2]) and np.array_equal(end[p], want[3]), (p, start[p], end[p], want)
        # spans disjoint and within consequence 1's bounds
        lo, hi = paced_ref.span_bounds(max(sets.tgt[t].shape[0], 1))
        taken = np.zeros(sets.src[int(src_idx[p]) - base].shape[0] + 1, dtype=int) if want[0] else None
        for m in range(want[0]):
            assert lo <= int(end[p, m]) - int(start[p, m]) + 1 <= hi and np.isfinite(cost[p, m])
            taken[int(start[p, m]):int(end[p, m]) + 1] += 1
        assert taken is None or taken.max() <= 1
        total += want[0]
    return total


def _all_pairs(n_src, n_tgt):
    return np.repeat(np.arange(n_src, dtype=np.uint32), n_tgt), np.tile(np.arange(n_tgt, dtype=np.uint32), n_src)


def _ints(rng, f, dim):
    return rng.integers(0, 3, size=(f, dim)).astype(np.float64)            # {0, 1, 2}: exact sums, real ties


def _reals(rng, f, dim):
    return rng.standard_normal((f, dim)).astype(np.float32).astype(np.float64)


def _distinct(rng, f, dim):
    """Frames no two of which are equal, far apart: a planted copy is the only place a target costs 0."""
    x = rng.integers(100, 200, size=(f, dim)).astype(np.float64)
    x[:, 0] = 1000.0 + 7.0 * np.arange(f)
    return x


SRC_FRAMES = [1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 130, 200]


# ---- 1. chunk and hand-off edges -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,squared", [("int", True), ("real", False)])
def test_a_five_frame_target_against_every_source_length(kind, squared):
    rng = np.random.default_rng(0x9AC1 + squared)
    mk = _ints if kind == "int" else _reals
    s = _Sets([mk(rng, f, 13) for f in SRC_FRAMES], [mk(rng, 5, 13)], 13, squared=squared)
    si, ti = _all_pairs(len(SRC_FRAMES), 1)
    found = _check(s, si, ti, _spot(s, si, ti))
    assert found == len(SRC_FRAMES) - 2                                    # 5 frames need 3: sources of 1 and 2 have no spot
    total = _check_all(s, si, ti, _spot_all(s, si, ti, k=8), 8)
    assert total > found
    s.close()


@pytest.mark.parametrize("first", [62, 63])
def test_a_decimated_target_whose_skips_cross_the_chunk_edge(first):
    """Consequence 3 across the hand-off: a target equal to every second source frame from `first` - 4 on, so one of
    its skips goes from row `first` to row `first` + 2 (62 -> 64: through bound2; 63 -> 65: through bound1 into lane 1's
    second diagonal)."""
    rng = np.random.default_rng(0xDEC + first)
    for frames in (66, 130, 200):
        src = _distinct(rng, frames, 13)
        rows = np.arange(first - 4, first + 3, 2)                          # ..., first, first + 2
        assert first in rows and first + 2 in rows
        s = _Sets([src], [src[rows]], 13, squared=True)
        out = _spot(s, [0], [0])
        _check(s, [0], [0], out)
        assert (out[1][0], int(out[2][0]), int(out[3][0])) == (0.0, int(rows[0]), int(rows[-1]))
        assert int(out[3][0]) - int(out[2][0]) + 1 == 2 * rows.size - 1
        s.close()


def test_a_doubled_target_across_rows_63_and_64():
    """Consequence 4 across the hand-off: every frame of source rows 61 ... 66 twice, so the path repeats in rows 63 and
    64 and steps from the one to the other."""
    rng = np.random.default_rng(0xD0B)
    src = _distinct(rng, 130, 13)
    tgt = np.repeat(src[61:67], 2, axis=0)
    s = _Sets([src], [tgt], 13, squared=True)
    out = _spot(s, [0], [0])
    _check(s, [0], [0], out)
    assert (out[1][0], int(out[2][0]), int(out[3][0])) == (0.0, 61, 66) and 66 - 61 + 1 == tgt.shape[0] // 2
    s.close()


# ---- 2. ring and target edges --------------------------------------------------------------------------------------------

TGT_FRAMES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 2048]


@pytest.mark.parametrize("kind,squared", [("int", True), ("real", False)])
def test_every_target_length_against_a_300_frame_source(kind, squared):
    rng = np.random.default_rng(0x71E + squared)
    mk = _ints if kind == "int" else _reals
    src = [mk(rng, 300, 3), mk(rng, 1, 3)]
    s = _Sets(src, [mk(rng, f, 3) for f in TGT_FRAMES], 3, squared=squared)
    si, ti = _all_pairs(2, len(TGT_FRAMES))
    out = _spot(s, si, ti)
    found = _check(s, si, ti, out)
    # 300 source frames hold targets of up to 599 frames; the one-frame source holds Fb = 1 and Fb = 2 (a single repeat)
    assert found == len(TGT_FRAMES) - 1 + 2
    assert int(out[3][len(TGT_FRAMES) + 1]) == 0 and int(out[2][len(TGT_FRAMES) + 1]) == 0
    _check_all(s, si, ti, _spot_all(s, si, ti, k=3), 3)
    s.close()


# ---- 3. dim ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 13, 14, 15, 16, 17, 40, 41, 64])
def test_padding_edges_of_every_dimr(dim):
    rng = np.random.default_rng(0xD1B + dim)
    for mk, squared in ((_ints, True), (_reals, False)):
        s = _Sets([mk(rng, 130, dim), mk(rng, 70, dim)], [mk(rng, 9, dim), mk(rng, 70, dim)], dim, squared=squared)
        si, ti = _all_pairs(2, 2)
        assert _check(s, si, ti, _spot(s, si, ti)) == 4
        assert _check_all(s, si, ti, _spot_all(s, si, ti, k=4), 4) >= 6
        s.close()


# ---- 4. pair lists --------------------------------------------------------------------------------------------------------

def test_pairings_index_base_no_match_empty_segments_device_outputs_and_the_fold():
    rng = np.random.default_rng(0x9A14)
    dim = 13
    mk = lambda f: rng.integers(-3, 4, size=(f, dim)).astype(np.float64)
    src = [mk(f) for f in (30, 0, 90, 1, 150, 64, 0, 77, 5)]
    tgt = [mk(f) for f in (10, 0, 33, 1, 80, 64, 7)]
    s = _Sets(src, tgt, dim, squared=True)
    first = np.array([3, 0, 8, 8, 1, 2, 5], dtype=np.uint32)
    a = _spot(s, first)                                                # tgt_idx = NULL: pair p uses target p
    b = _spot(s, first, np.arange(7, dtype=np.uint32))
    _check(s, first, None, a)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    _check(s, first[:3], None, _spot(s, first[:3]))                    # fewer pairs than targets
    # repeats, any pairing, SSYM_NO_MATCH, index_base = 1
    si = np.array([5, 5, 9, NO, 1, 5, NO, 9, 2, 7], dtype=np.uint32)
    ti = np.array([6, 6, 0, 2, 5, 6, 0, 0, 4, 1], dtype=np.uint32)
    out = _spot(s, si, ti, base=1)
    _check(s, si, ti, out, base=1)
    for p in (3, 6, 8, 9):                                             # no match, no match, empty source, empty target
        assert np.isposinf(out[1][p]) and out[2][p] == NO and out[3][p] == NO
    dev = _spot(s, si, ti, base=1, device=True)
    assert dev[0] == nat.SSYM_OK
    assert np.array_equal(_bits(dev[1]), _bits(out[1])) and np.array_equal(dev[2], out[2]) and np.array_equal(dev[3], out[3])
    alls = _spot_all(s, si, ti, base=1, k=5)
    _check_all(s, si, ti, alls, 5, base=1)
    adev = _spot_all(s, si, ti, base=1, k=5, device=True)
    assert adev[0] == nat.SSYM_OK and np.array_equal(_bits(adev[2]), _bits(alls[2]))
    for x, y in zip((alls[1], alls[3], alls[4]), (adev[1], adev[3], adev[4])):
        assert np.array_equal(x, y)
    # occurrence 0 is ssym_dtw_spot_step's result
    assert np.array_equal(_bits(alls[2][:-1, 0]), _bits(out[1][:-1]))
    assert np.array_equal(alls[3][:-1, 0], out[2][:-1]) and np.array_equal(alls[4][:-1, 0], out[3][:-1])
    # the Python layer: host and device
    cost, start, end = s.e.dtw_spot(s.d, s.q, si, ti, index_base=1, step="paced")
    assert np.array_equal(_bits(cost), _bits(out[1][:-1])) and np.array_equal(start, out[2][:-1]) and np.array_equal(end, out[3][:-1])
    dcost, dstart, dend = s.e.dtw_spot_device(s.d, s.q, si, ti, index_base=1, step="paced")
    assert dcost.is_cuda and np.array_equal(_bits(dcost.cpu().numpy()), _bits(cost))
    assert np.array_equal(dstart.cpu().numpy().view(np.uint32), start) and np.array_equal(dend.cpu().numpy().view(np.uint32), end)
    count, cost, start, end = s.e.dtw_spot_all(s.d, s.q, si, ti, index_base=1, max_spots=5, step="paced")
    assert np.array_equal(count, alls[1][:-1]) and np.array_equal(_bits(cost), _bits(alls[2][:-1]))
    dcount, dcost, dstart, dend = s.e.dtw_spot_all_device(s.d, s.q, si, ti, index_base=1, max_spots=5, step="paced")
    assert np.array_equal(dcount.cpu().numpy().view(np.uint32), count) and np.array_equal(_bits(dcost.cpu().numpy()), _bits(cost))
    tm = s.e.timings()
    assert tm["n_pairs"] == si.size and tm["main_ms"] > 0 and tm["main_launches"] == 1
    # ssym_spot_queries_step: the fold of the per-pair results, on the host and in device memory
    m = len(tgt)
    for base in (0, 1):
        idx = np.full(m + 1, SENT32, dtype=np.uint32)
        cost = np.full(m + 1, SENTF)
        start, end = np.full(m + 1, SENT32, dtype=np.uint32), np.full(m + 1, SENT32, dtype=np.uint32)
        rc = nat.lib().ssym_spot_queries_step(s.e.ctx, s.d.ptr, s.q.ptr, base, PACED, idx.ctypes.data, cost.ctypes.data,
                                              start.ctypes.data, end.ctypes.data, 0)
        assert rc == nat.SSYM_OK and idx[m] == SENT32 and cost[m] == SENTF and start[m] == SENT32 and end[m] == SENT32
        for t in range(m):
            best = (NO, float("inf"), NO, NO)
            for k in range(len(src)):
                c, st, en = s.ref(k, t)
                if c < best[1]:
                    best = (k + base, c, st, en)
            assert (int(idx[t]), int(start[t]), int(end[t])) == (best[0], best[2], best[3]) and _bits(cost[t]) == _bits(best[1]), t
            assert (best[0] == NO) == (tgt[t].shape[0] == 0)
    pidx, pcost, pstart, pend = s.e.spot_queries(s.d, s.q, step="paced")
    assert np.array_equal(pidx + np.where(pidx == NO, 0, 1).astype(np.uint32), idx[:m]) and np.array_equal(_bits(pcost), _bits(cost[:m]))
    s.close()


def test_more_pairs_than_workgroups_reuse_the_hand_off_rows():
    """Workgroup b of a grid of g walks pairs b, b + g, ...: a 130-frame source (both hand-off rows written twice) is
    followed by a 3-frame one, and by another 130-frame one whose first chunk must read neither row."""
    rng = np.random.default_rng(0x5108)
    dim = 3
    frames = np.array([130, 3, 130, 3, 200])
    src = [_ints(rng, f, dim) for f in frames]
    tgt = [_ints(rng, f, dim) for f in (1, 2, 3, 4, 5)]
    s = _Sets(src, tgt, dim, squared=True)
    n = 5000
    assert n > 2 * 8 * 256                            # 8 workgroups per CU, 256 CUs: every workgroup walks several pairs
    si = rng.integers(0, 5, size=n).astype(np.uint32)
    ti = rng.integers(0, 5, size=n).astype(np.uint32)
    fa = frames[si]
    for cus in (64, 256, 304):
        g = 8 * cus
        assert np.count_nonzero((fa[:-g] >= 130) & (fa[g:] == 3)) >= 100, cus
    found = _check(s, si, ti, _spot(s, si, ti))
    assert found > n // 2
    total = _check_all(s, si, ti, _spot_all(s, si, ti, k=4), 4)
    assert total > found
    s.close()


# ---- 5. occurrences -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 64])
def test_occurrences_with_thresholds_that_admit_none_some_and_all(k):
    rng = np.random.default_rng(0x0CC + k)
    src = [_ints(rng, f, 3) for f in (200, 65, 7)]
    tgt = [_ints(rng, f, 3) for f in (1, 4, 9)]
    s = _Sets(src, tgt, 3, squared=True)
    si, ti = _all_pairs(3, 3)
    free = _spot_all(s, si, ti, k=k)
    total = _check_all(s, si, ti, free, k)
    assert total >= si.size - 1                                      # (9 frames need 5 source frames: every pair has a spot)
    one = _spot(s, si, ti)
    _check(s, si, ti, one)
    assert np.array_equal(_bits(free[2][:-1, 0]), _bits(one[1][:-1])) and np.array_equal(free[4][:-1, 0], one[3][:-1])
    least = one[1][:-1]
    for limits, what in ((least - 1.0, "none"), (least + 1.0, "some"), (np.full(si.size, np.inf), "all")):
        out = _spot_all(s, si, ti, k=k, max_cost=limits)
        got = _check_all(s, si, ti, out, k, max_cost=limits)
        if what == "none":
            assert got == 0 and (out[1][:-1] == 0).all() and np.isposinf(out[2][:-1]).all() and (out[4][:-1] == NO).all()
        elif what == "all":
            assert got == total
        else:
            assert si.size <= got <= total                           # at least every pair's best span
    s.close()


def test_three_plants_found_three_times_with_a_threshold_per_frame():
    rng = np.random.default_rng(0x50A12)
    nc = 5
    tgt_f = rng.standard_normal((8, nc))
    long_f = rng.standard_normal((20, nc))

    def recording(frames, plants, name):
        f = 6.0 + rng.standard_normal((frames, nc))                   # noise away from the targets' frames
        for at, what in plants:
            f[at:at + what.shape[0]] = what
        return Sound(rng.standard_normal(frames * HOP), 8000.0, f.reshape(-1), name, ncoeffs=nc)

    e = Engine(metric="dtw", dtype="f64")
    d = SoundDictionary(engine=e)
    d.sounds = [recording(200, ((10, tgt_f), (60, tgt_f), (120, tgt_f), (150, long_f)), "rec")]
    targets = [Sound(rng.standard_normal(8 * HOP), 8000.0, tgt_f.reshape(-1), "t", ncoeffs=nc),
               Sound(rng.standard_normal(20 * HOP), 8000.0, long_f.reshape(-1), "l", ncoeffs=nc)]
    # one threshold for targets of 8 and of 20 frames: a mean per-frame distance
    lists = d.spot_all(targets, max_spots=6, step="paced", max_cost_per_frame=0.5)
    assert [(sp.source_index, sp.start_frame, sp.end_frame, sp.cost, sp.cost_per_frame) for sp in lists[0]] == \
        [(0, 10, 17, 0.0, 0.0), (0, 60, 67, 0.0, 0.0), (0, 120, 127, 0.0, 0.0)]
    assert [(sp.start_frame, sp.end_frame, sp.cost_per_frame) for sp in lists[1]] == [(150, 169, 0.0)]
    # without a threshold the list goes on, every span within the pattern's bounds, cost_per_frame = cost / frames
    feats = d.sounds[0].mfcc_arrays()
    free = d.spot_all(targets, max_spots=6, step="paced")
    for t, frames in enumerate((8, 20)):
        count, cost, start, end = paced_ref.spot_all(feats, targets[t].mfcc_arrays(), 6)
        assert [(sp.cost, sp.start_frame, sp.end_frame) for sp in free[t]] == \
            sorted((float(cost[m]), int(start[m]), int(end[m])) for m in range(count))
        lo, hi = paced_ref.span_bounds(frames)
        for sp in free[t]:
            assert lo <= sp.num_frames() <= hi and sp.cost_per_frame == sp.cost / frames
    assert len(free[0]) > 3
    per_target = d.spot_all(targets, indices=[0, 0], max_spots=6, step="paced", max_cost_per_frame=[0.5, -1.0])
    assert len(per_target[0]) == 3 and per_target[1] == []
    seq = SoundSequence.new(targets).spot_all_in_dictionary(d, max_spots=6, step="paced", max_cost_per_frame=0.5)
    assert [[(sp.start_frame, sp.end_frame) for sp in x] for x in seq] == [[(sp.start_frame, sp.end_frame) for sp in x] for x in lists]
    best = d.spot(targets, step="paced")
    assert [(sp.start_frame, sp.end_frame, sp.cost, sp.cost_per_frame) for sp in best] == [(10, 17, 0.0, 0.0), (150, 169, 0.0, 0.0)]
    assert [sp.end_frame for sp in SoundSequence.new(targets).spot_in_dictionary(d, step="paced")] == [17, 169]
    assert d.spot(targets)[0].cost_per_frame is None and d.spot_all(targets, max_spots=1)[0][0].cost_per_frame is None
    e.close()


# ---- 6. the symmetric step is the old call ---------------------------------------------------------------------------------

def test_symmetric_step_is_the_existing_calls_bit_for_bit():
    rng = np.random.default_rng(0x5E77)
    dim = 13
    src = [_reals(rng, f, dim) for f in (130, 0, 64, 7)]
    tgt = [_reals(rng, f, dim) for f in (9, 70, 0, 1)]
    s = _Sets(src, tgt, dim)
    si = np.array([0, 2, NO, 3, 1, 0, 0, 2], dtype=np.uint32)
    ti = np.array([0, 1, 0, 3, 0, 2, 1, 0], dtype=np.uint32)
    out = _spot(s, si, ti, step=SYMMETRIC)
    cost, start, end = s.e.dtw_spot(s.d, s.q, si, ti)
    assert out[0] == nat.SSYM_OK and np.array_equal(_bits(out[1][:-1]), _bits(cost))
    assert np.array_equal(out[2][:-1], start) and np.array_equal(out[3][:-1], end) and out[1][-1] == SENTF
    limits = np.full(si.size, 40.0)
    alls = _spot_all(s, si, ti, k=4, max_cost=limits, step=SYMMETRIC)
    count, cost, start, end = s.e.dtw_spot_all(s.d, s.q, si, ti, max_spots=4, max_cost=limits)
    assert alls[0] == nat.SSYM_OK and np.array_equal(alls[1][:-1], count) and np.array_equal(_bits(alls[2][:-1]), _bits(cost))
    assert np.array_equal(alls[3][:-1], start) and np.array_equal(alls[4][:-1], end) and count.sum() > 0
    m = len(tgt)
    idx, qc = np.full(m, SENT32, dtype=np.uint32), np.full(m, SENTF)
    qs, qe = np.full(m, SENT32, dtype=np.uint32), np.full(m, SENT32, dtype=np.uint32)
    rc = nat.lib().ssym_spot_queries_step(s.e.ctx, s.d.ptr, s.q.ptr, 0, SYMMETRIC, idx.ctypes.data, qc.ctypes.data,
                                          qs.ctypes.data, qe.ctypes.data, 0)
    widx, wcost, wstart, wend = s.e.spot_queries(s.d, s.q)
    assert rc == nat.SSYM_OK and np.array_equal(idx, widx) and np.array_equal(_bits(qc), _bits(wcost))
    assert np.array_equal(qs, wstart) and np.array_equal(qe, wend)
    s.close()


# ---- 7. consequence 5 -------------------------------------------------------------------------------------------------------

def test_a_tripled_target_costs_more_than_zero_where_the_symmetric_pattern_gives_zero():
    rng = np.random.default_rng(0x7819)
    src = _distinct(rng, 130, 13)
    tgt = np.repeat(src[60:68], 3, axis=0)                             # across the chunk edge
    s = _Sets([src], [tgt], 13, squared=True)
    out = _spot(s, [0], [0])
    _check(s, [0], [0], out)
    assert out[1][0] > 0.0 and np.isfinite(out[1][0])
    cost, start, end = s.e.dtw_spot(s.d, s.q, [0], [0])
    assert (cost[0], int(start[0]), int(end[0])) == (0.0, 60, 67)
    s.close()


# ---- 8. non-finite features -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e200])
@pytest.mark.parametrize("squared", [True, False])
def test_a_non_finite_value_in_a_source_or_a_target_frame(value, squared):
    rng = np.random.default_rng(0xBAD8)
    dim = 13
    base_src, base_tgt = _reals(rng, 130, dim), _reals(rng, 9, dim)
    src, tgt = [base_src], [base_tgt]
    for row in (10, 63, 64, 65):
        a = base_src.copy()
        a[row, dim - 1] = value
        src.append(a)
    for col in (0, 4, 8):
        b = base_tgt.copy()
        b[col, 2] = value
        tgt.append(b)
    s = _Sets(src, tgt, dim, squared=squared)
    si, ti = _all_pairs(len(src), len(tgt))
    rc, cost, start, end = _spot(s, si, ti)
    assert rc == nat.SSYM_OK and not np.isnan(cost[:-1]).any()
    for p in range(si.size):
        want = s.ref(int(si[p]), int(ti[p]))
        assert same_floats(cost[p], want[0]) and (int(start[p]), int(end[p])) == want[1:], (p, cost[p], start[p], end[p], want)
        assert np.isfinite(cost[p]) == (int(end[p]) != NO)
        if int(ti[p]) >= 1:
            assert int(end[p]) == NO and np.isposinf(cost[p])          # a poisoned target frame: every path takes it
        else:
            assert np.isfinite(cost[p])                                # a poisoned source frame can be skipped or avoided
    out = _spot_all(s, si, ti, k=4)
    assert out[0] == nat.SSYM_OK and not np.isnan(out[2][:-1]).any()
    for p in range(si.size):
        want = s.ref_all(int(si[p]), int(ti[p]), 4)
        assert int(out[1][p]) == want[0] and same_floats(out[2][p], want[1]), (p, out[2][p], want[1])
        assert np.array_equal(out[3][p], want[2]) and np.array_equal(out[4][p], want[3])
        assert np.isfinite(out[2][p, :want[0]]).all() and np.isposinf(out[2][p, want[0]:]).all()
    # the profile itself has NaN and +inf entries in these cases: the strict < comparisons were exercised
    kinds = [s.profile(k, 0)[0] for k in range(1, len(src))]
    assert all((~np.isfinite(d)).any() for d in kinds)
    s.close()


# ---- 9. limits --------------------------------------------------------------------------------------------------------------

def test_limits_and_an_unknown_step():
    rng = np.random.default_rng(0x2049)
    mk = lambda f: rng.integers(-2, 3, size=(f, 2)).astype(np.float64)
    s = _Sets([mk(50), mk(1100)], [mk(2048), mk(2049), mk(3)], 2, squared=True)
    zero = np.zeros(1, dtype=np.uint32)
    si, ti = np.array([1, 0], np.uint32), np.array([0, 2], np.uint32)               # at the limit
    assert _check(s, si, ti, _spot(s, si, ti)) == 2
    for call in (_spot, _spot_all):
        out = call(s, zero, np.array([1], np.uint32))
        assert out[0] == nat.SSYM_E_UNSUPPORTED and b"2048" in nat.lib().ssym_last_error(s.e.ctx) and _untouched(out)
        out = call(s, zero, zero, step=7)
        assert out[0] == nat.SSYM_E_INVALID and b"step" in nat.lib().ssym_last_error(s.e.ctx) and _untouched(out)
        assert call(s, zero, np.array([1], np.uint32), step=SYMMETRIC)[0] == nat.SSYM_OK      # 2049 frames: the old limit holds
    m = 3
    idx, qc = np.full(m, SENT32, dtype=np.uint32), np.full(m, SENTF)
    for step, want in ((PACED, nat.SSYM_E_UNSUPPORTED), (7, nat.SSYM_E_INVALID)):
        rc = nat.lib().ssym_spot_queries_step(s.e.ctx, s.d.ptr, s.q.ptr, 0, step, idx.ctypes.data, qc.ctypes.data,
                                              idx.ctypes.data, idx.ctypes.data, 0)
        assert rc == want and (idx == SENT32).all() and (qc == SENTF).all()
    with pytest.raises(nat.SsymError):
        s.e.dtw_spot(s.d, s.q, [0], [1], step="paced")
    s.close()
    wide = _Sets([np.zeros((3, 65))], [np.zeros((3, 65))], 65)
    out = _spot(wide, zero)
    assert out[0] == nat.SSYM_E_UNSUPPORTED and _untouched(out)
    wide.close()


@pytest.mark.parametrize("kw", [dict(band=0), dict(band=32), dict(metric="refcos")])
def test_banded_and_refcos_contexts_are_refused(kw):
    rng = np.random.default_rng(1)
    s = _Sets([rng.standard_normal((50, 12))], [rng.standard_normal((6, 12))], 12, **kw)
    zero = np.zeros(1, dtype=np.uint32)
    for call in (_spot, _spot_all):
        out = call(s, zero)
        assert out[0] == nat.SSYM_E_UNSUPPORTED and _untouched(out)
        assert (b"refcos" if "metric" in kw else b"band") in nat.lib().ssym_last_error(s.e.ctx)
    idx, qc = np.full(1, SENT32, dtype=np.uint32), np.full(1, SENTF)
    rc = nat.lib().ssym_spot_queries_step(s.e.ctx, s.d.ptr, s.q.ptr, 0, PACED, idx.ctypes.data, qc.ctypes.data,
                                          idx.ctypes.data, idx.ctypes.data, 0)
    assert rc == nat.SSYM_E_UNSUPPORTED and idx[0] == SENT32 and qc[0] == SENTF
    s.close()
