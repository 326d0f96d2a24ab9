"""ssym_dtw_spot_all on the GPU against the numpy restatement (tests/spot_all_ref.py), bit for bit: counts, costs, starts,
ends and padding slots, at every shape edge of the kernel (64-row chunks, the 64-step refill, one chunk, one column,
the padding edges of every DIMR, the grid stride with its reused profile slots), with real ties, through every way of
listing pairs, against ssym_dtw_spot and ssym_pair_matrix(exact = 1), through SoundDictionary.spot_all, and every error
the header lists.  Outputs are sentinel-filled before every call."""
import numpy as np
import pytest

import spot_all_ref
import wave_lds
from soundsym_amd import HOP, Engine, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

SENT32, SENTF = 0xDEADBEEF, -12345.5
NO = nat.NO_MATCH


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class _Sets:
    """An engine with a resident dictionary and query set made from lists of [frames, dim] arrays.  `profiles` (shared
    between the sets of one test: the features decide it, not the engine) keeps every pair's end-column profile."""

    def __init__(self, src, tgt, dim, dtype="f64", band=-1, squared=False, metric="dtw", profiles=None):
        self.src, self.tgt, self.dim, self.squared = src, tgt, dim, squared
        npd = np.float32 if dtype == "f32" else np.float64
        self.e = Engine(metric=metric, dtype=dtype, band=band, squared=squared)
        sf, so = pack_segments(src, dim, npd)
        tf, to = pack_segments(tgt, dim, npd)
        self.d, self.q = self.e.dictionary(sf, so, dim), self.e.queries(tf, to, dim)
        self._prof = {} if profiles is None else profiles
        self._picks = {}

    def close(self):
        self.e.close()

    def ref(self, s, t, k, limit=None):
        """(count, cost [k], start [k], end [k]) of the restatement; the profile is computed once per pair."""
        a, b = np.asarray(self.src[s], np.float64), np.asarray(self.tgt[t], np.float64)
        if a.shape[0] == 0 or b.shape[0] == 0:
            return spot_all_ref.padded([], k)
        if (s, t) not in self._prof:
            self._prof[(s, t)] = spot_all_ref.profile(a, b, self.squared)
        if (s, t, k, limit) not in self._picks:
            self._picks[(s, t, k, limit)] = spot_all_ref.padded(spot_all_ref.select(*self._prof[(s, t)], k, limit), k)
        return self._picks[(s, t, k, limit)]


def _raw(sets, src_idx, tgt_idx=None, base=0, k=8, max_cost=None, device=False, null=()):
    """ssym_dtw_spot_all through ctypes into sentinel-filled outputs (one pair more than listed):
    (rc, count [n + 1], cost [n + 1, k], start [n + 1, k], end [n + 1, k])."""
    src = np.ascontiguousarray(src_idx, dtype=np.uint32)
    tgt = None if tgt_idx is None else np.ascontiguousarray(tgt_idx, dtype=np.uint32)
    n = src.size
    rows = max(k, 1)
    count = np.full(n + 1, SENT32, dtype=np.uint32)
    cost = np.full((n + 1, rows), SENTF)
    start = np.full((n + 1, rows), SENT32, dtype=np.uint32)
    end = np.full((n + 1, rows), SENT32, dtype=np.uint32)
    mc = None if max_cost is None else np.ascontiguousarray(max_cost, dtype=np.float64)
    L = nat.lib()
    args = [sets.e.ctx, sets.d.ptr, sets.q.ptr, src.ctypes.data, None if tgt is None else tgt.ctypes.data, n, base, k,
            None if mc is None else mc.ctypes.data]
    if device:
        import torch
        dn, ds, de = (torch.from_numpy(x.view(np.int32)).cuda() for x in (count, start, end))
        dc = torch.from_numpy(cost).cuda()
        rc = L.ssym_dtw_spot_all(*args, dn.data_ptr(), dc.data_ptr(), ds.data_ptr(), de.data_ptr(), nat.OUT_DEVICE)
        torch.cuda.synchronize()
        count, start, end = (x.cpu().numpy().view(np.uint32) for x in (dn, ds, de))
        cost = dc.cpu().numpy()
    else:
        ptr = lambda name, arr: None if name in null else arr.ctypes.data
        rc = L.ssym_dtw_spot_all(*args, ptr("count", count), ptr("cost", cost), ptr("start", start), ptr("end", end), 0)
    return rc, count, cost, start, end


def _untouched(out):
    _, count, cost, start, end = out
    return (count == SENT32).all() and (cost == SENTF).all() and (start == SENT32).all() and (end == SENT32).all()


def _check(sets, src_idx, tgt_idx, out, k, base=0, max_cost=None):
    """Every pair of a call equal to the restatement, padding included; the row beyond the pairs untouched.  Returns
    (occurrences in all, pairs whose list holds two equal costs)."""
    rc, count, cost, start, end = out
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(sets.e.ctx)
    n = len(src_idx)
    assert count[n] == SENT32 and (cost[n] == SENTF).all() and (start[n] == SENT32).all() and (end[n] == SENT32).all()
    total = ties = 0
    for p in range(n):
        t = p if tgt_idx is None else int(tgt_idx[p])
        limit = None if max_cost is None else float(np.asarray(max_cost).reshape(-1)[p])
        if int(src_idx[p]) == NO:
            want = spot_all_ref.padded([], k)
        else:
            want = sets.ref(int(src_idx[p]) - base, t, k, limit)
        assert int(count[p]) == want[0], (p, int(count[p]), want[0])
        assert np.array_equal(_bits(cost[p]), _bits(want[1])), (p, cost[p], want[1])
        assert np.array_equal(start[p], want[2]) and np.array_equal(end[p], want[3]), (p, start[p], end[p], want)
        total += want[0]
        ties += int(np.unique(want[1][:want[0]]).size < want[0])
    return total, ties


def _all_pairs(n_src, n_tgt):
    return np.repeat(np.arange(n_src, dtype=np.uint32), n_tgt), np.tile(np.arange(n_tgt, dtype=np.uint32), n_src)


def _frames(rng, f, dim, kind):
    if kind == "int":
        return rng.integers(0, 3, size=(f, dim)).astype(np.float64)        # {0, 1, 2}: exact sums, real ties
    return rng.standard_normal((f, dim)).astype(np.float32)                # (f32 values: both dtypes hold them exactly)


SRC_FRAMES = [1, 2, 63, 64, 65, 127, 128, 129, 200]   # chunk edges, the hand-off, profile stores of a partial chunk
TGT_FRAMES = [1, 2, 3, 63, 64, 65, 130]               # one column, the ring and its refill
_SHAPE_DATA = {}


def _shape_data(kind):
    """Features and the profile cache of test 1, made once per kind and shared by every K and dtype."""
    if kind not in _SHAPE_DATA:
        rng = np.random.default_rng(0xA115 + (kind == "int"))
        _SHAPE_DATA[kind] = ([_frames(rng, f, 3, kind) for f in SRC_FRAMES], [_frames(rng, f, 3, kind) for f in TGT_FRAMES], {})
    return _SHAPE_DATA[kind]


# ---- 1. shapes, K, dtypes, ties ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("kind,squared", [("int", True), ("real", False)])
def test_every_source_length_against_every_target_length(kind, squared, k, dtype):
    src, tgt, profiles = _shape_data(kind)
    s = _Sets(src, tgt, 3, dtype=dtype, squared=squared, profiles=profiles)
    si, ti = _all_pairs(len(src), len(tgt))
    out = _raw(s, si, ti, k=k)
    total, ties = _check(s, si, ti, out, k)
    s.close()
    print("occurrences: %d of %d slots, pairs with equal costs in their list: %d" % (total, si.size * k, ties))
    assert total >= si.size                                  # every pair has frames on both sides: at least the spot
    if k == 64:
        assert total < si.size * k                           # ... and no 200-frame source holds 64 disjoint spans of each
    if kind == "int" and k > 1:
        assert ties >= 10, ties                              # the (cost, end) order is exercised, not just stated


# ---- 2. padding edges of DIMR --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 13, 14, 16, 17, 40, 41, 64])
def test_padding_edges_of_every_dimr(dim):
    rng = np.random.default_rng(0xD1A + dim)
    for kind, squared in (("int", True), ("real", False)):
        s = _Sets([_frames(rng, 70, dim, kind)], [_frames(rng, 9, dim, kind)], dim, squared=squared)
        total, _ = _check(s, [0], [0], _raw(s, [0], [0], k=4), 4)
        assert total >= 2
        s.close()


_LONG = [c for c in wave_lds.CROSSINGS if c[1] > 130]


@pytest.mark.parametrize("dim,fb,above", _LONG)
def test_both_sides_of_every_lds_crossing(dim, fb, above):
    """The launch's dynamic LDS goes by the longest listed target: one call per length, on the side of 64 KiB the case
    names, up to the 116736 bytes of dim 64 x 4096 frames; K = 3."""
    need = wave_lds.spot_lds_bytes(dim, fb)
    assert (need > wave_lds.LIMIT) == above, (dim, fb, need)
    rng = np.random.default_rng(0x1D5 + 4099 * dim + fb)
    s = _Sets([_frames(rng, f, dim, "real") for f in (65, 130)], [_frames(rng, fb, dim, "real")], dim)
    si, ti = _all_pairs(2, 1)
    total, _ = _check(s, si, ti, _raw(s, si, ti, k=3), 3)
    assert total >= 2
    s.close()


# ---- 3. identical plants and max_cost ------------------------------------------------------------------------------------

def test_identical_plants_and_a_threshold_per_pair():
    rng = np.random.default_rng(0x91A)
    tgt = rng.integers(1, 4, size=(6, 3)).astype(np.float64)
    rec = rng.integers(5, 9, size=(120, 3)).astype(np.float64)             # noise that no target frame equals
    for at in (10, 50, 90):
        rec[at:at + 6] = tgt
    s = _Sets([rec], [tgt], 3, squared=True)
    least = s.ref(0, 0, 1)[1][0]
    assert least == 0.0
    zero = np.zeros(1, dtype=np.uint32)
    out = _raw(s, zero, zero, k=6, max_cost=[0.0])
    _check(s, zero, zero, out, 6, max_cost=[0.0])
    _, count, cost, start, end = out
    assert count[0] == 3 and np.array_equal(_bits(cost[0, :3]), _bits([0.0] * 3))          # +0.0, not -0.0
    assert start[0, :3].tolist() == [10, 50, 90] and end[0, :3].tolist() == [15, 55, 95]
    assert np.isinf(cost[0, 3:]).all() and (start[0, 3:] == NO).all() and (end[0, 3:] == NO).all()
    out = _raw(s, zero, zero, k=6, max_cost=[np.nextafter(least, -np.inf)])                # below the least delta
    assert out[0] == nat.SSYM_OK and out[1][0] == 0 and np.isinf(out[2][0]).all() and (out[4][0] == NO).all()
    out = _raw(s, zero, zero, k=2, max_cost=[0.0])
    assert out[1][0] == 2 and out[4][0].tolist() == [15, 55]
    # one call, another threshold per pair: none fits, the plants, the plants and what costs at most 100, everything
    si = ti = np.zeros(5, dtype=np.uint32)
    limits = [-1.0, 0.0, 100.0, np.inf, -np.inf]
    out = _raw(s, si, ti, k=8, max_cost=limits)
    _check(s, si, ti, out, 8, max_cost=limits)
    assert out[1][:2].tolist() == [0, 3] and out[1][4] == 0 and 3 <= out[1][2] <= out[1][3]
    assert (out[2][2][:out[1][2]] <= 100.0).all()
    count, cost, start, end = s.e.dtw_spot_all(s.d, s.q, si, ti, max_spots=8, max_cost=limits)
    assert np.array_equal(count, out[1][:5]) and np.array_equal(_bits(cost), _bits(out[2][:5]))
    assert np.array_equal(start, out[3][:5]) and np.array_equal(end, out[4][:5])
    count, cost, start, end = s.e.dtw_spot_all(s.d, s.q, si, ti, max_spots=6, max_cost=0.0)          # a scalar
    assert count.tolist() == [3] * 5 and cost.shape == (5, 6)
    s.close()


# ---- 4. agreement with the existing calls --------------------------------------------------------------------------------

def test_first_occurrence_is_the_spot_and_costs_are_the_exact_kernels_on_the_cuts():
    rng = np.random.default_rng(0xA64E)
    dim = 13
    for squared in (False, True):
        tgt = [rng.standard_normal((f, dim)) for f in (24, 7, 70)]
        noise = rng.standard_normal((400, dim))
        planted = noise.copy()
        plants = []
        # the target as is, stretched (every other frame twice), and hurried (every fourth frame left out)
        for at, idx in ((40, np.arange(24)), (170, np.repeat(np.arange(24), [2, 1] * 12)), (300, np.arange(24)[np.arange(24) % 4 != 2])):
            warped = tgt[0][idx]
            planted[at:at + warped.shape[0]] = warped
            plants.append((at, at + warped.shape[0] - 1))
        src = [planted, rng.standard_normal((90, dim)), rng.standard_normal((64, dim)), np.zeros((0, dim))]
        s = _Sets(src, tgt, dim, squared=squared)
        si, ti = _all_pairs(4, 3)
        # K = 1 without a threshold: ssym_dtw_spot's three outputs
        one = _raw(s, si, ti, k=1)
        cost1, start1, end1 = s.e.dtw_spot(s.d, s.q, si, ti)
        assert one[0] == nat.SSYM_OK
        assert np.array_equal(_bits(one[2][:-1, 0]), _bits(cost1))
        assert np.array_equal(one[3][:-1, 0], start1) and np.array_equal(one[4][:-1, 0], end1)
        assert np.array_equal(one[1][:-1], (end1 != NO).astype(np.uint32))
        # K = 8: the restatement, then the properties through the GPU alone
        out = _raw(s, si, ti, k=8)
        _check(s, si, ti, out, 8)
        _, count, cost, start, end = out
        spans = [(p, m) for p in range(si.size) for m in range(int(count[p]))]
        cuts = [src[si[p]][start[p, m]:end[p, m] + 1] for p, m in spans]
        c = _Sets(cuts, tgt, dim, squared=squared)
        plain = c.e.pair_matrix(c.d, c.q, exact=True)
        for row, (p, m) in enumerate(spans):
            assert _bits(cost[p, m]) == _bits(plain[row, ti[p]]), (p, m)
        c.close()
        for p in range(si.size):
            got = cost[p, :count[p]]
            assert (np.diff(got) >= 0).all()
            taken = np.zeros(src[si[p]].shape[0] + 1, dtype=int)
            for m in range(int(count[p])):
                taken[start[p, m]:end[p, m] + 1] += 1
            assert taken.max() <= 1
        # the three plants are the first three occurrences of target 0 in source 0, each within its planted stretch
        assert count[0] >= 3
        found = sorted((int(start[0, m]), int(end[0, m])) for m in range(3))
        for (a, b), (lo, hi) in zip(found, plants):
            assert lo <= a <= b <= hi and b - a >= (hi - lo) // 2, (found, plants)
        assert cost[0, 0] == 0.0 and cost[0, 1] == 0.0 and end[0, 0] < end[0, 1]      # as is and stretched: both exact
        s.close()


# ---- 5. profile slots are reused -----------------------------------------------------------------------------------------

def test_5000_pairs_reuse_every_profile_slot():
    rng = np.random.default_rng(0x5107)
    dim = 3
    frames = np.array([130, 3, 130, 3])
    src = [rng.integers(0, 3, size=(f, dim)).astype(np.float64) for f in frames]
    tgt = [rng.integers(0, 3, size=(f, dim)).astype(np.float64) for f in (1, 2, 3, 4, 5)]
    s = _Sets(src, tgt, dim, squared=True)
    n = 5000
    assert n > 2 * 8 * 256                            # 8 workgroups per CU, 256 CUs: every workgroup walks several pairs
    # sources drawn at random: no period for the grid stride to fall in step with.  Workgroup b of a grid of g walks
    # pairs b, b + g, b + 2g, ...; whatever the part's CU count (g = 8 * CUs, up to 304 CUs), hundreds of workgroups
    # walk a 3-frame source right after a 130-frame one, in the slot the longer profile was left in
    si = rng.integers(0, 4, size=n).astype(np.uint32)
    ti = rng.integers(0, 5, size=n).astype(np.uint32)
    fa = frames[si]
    for cus in range(1, 305):
        g = 8 * cus
        assert np.count_nonzero((fa[:-g] == 130) & (fa[g:] == 3)) >= 200, cus
    out = _raw(s, si, ti, k=8)
    total, ties = _check(s, si, ti, out, 8)
    short = out[1][:n][fa == 3]
    assert short.max() <= 3 and total > n and ties >= 1          # a 3-frame source holds at most 3 disjoint spans
    tm = s.e.timings()
    assert tm["n_pairs"] == n and tm["main_ms"] > 0
    s.close()


# ---- 6. pairings ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pairings_index_base_no_match_empty_segments_and_device_outputs(dtype):
    rng = np.random.default_rng(0x9A13)
    dim = 13
    mk = lambda f: rng.integers(-3, 4, size=(f, dim)).astype(np.float64)
    src = [mk(f) for f in (30, 0, 90, 1, 150, 64, 0, 77, 5)]
    tgt = [mk(f) for f in (10, 0, 33, 1, 80, 64, 7)]
    s = _Sets(src, tgt, dim, dtype=dtype, squared=True)
    first = np.array([3, 0, 8, 8, 1, 2, 5], dtype=np.uint32)
    a = _raw(s, first, k=5)                                            # tgt_idx = NULL: pair p uses target p
    b = _raw(s, first, np.arange(7, dtype=np.uint32), k=5)
    _check(s, first, None, a, 5)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    assert a[1][[1, 4]].tolist() == [0, 0] and np.isinf(a[2][[1, 4]]).all() and (a[3][[1, 4]] == NO).all()
    _check(s, first[:3], None, _raw(s, first[:3], k=5), 5)             # fewer pairs than targets
    # repeats, any pairing, SSYM_NO_MATCH, index_base = 1
    si = np.array([5, 5, 9, NO, 1, 5, NO, 9, 2, 7], dtype=np.uint32)
    ti = np.array([6, 6, 0, 2, 5, 6, 0, 0, 4, 1], dtype=np.uint32)
    out = _raw(s, si, ti, base=1, k=5)
    _check(s, si, ti, out, 5, base=1)
    for p in (3, 6, 8, 9):                                             # no match, no match, empty source, empty target
        assert out[1][p] == 0 and np.isinf(out[2][p]).all() and (out[3][p] == NO).all() and (out[4][p] == NO).all()
    assert np.array_equal(out[2][0], out[2][1]) and np.array_equal(out[4][0], out[4][5])
    dev = _raw(s, si, ti, base=1, k=5, device=True)
    assert dev[0] == nat.SSYM_OK
    for x, y in zip(out[1:], dev[1:]):
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
    # the Python layer
    count, cost, start, end = s.e.dtw_spot_all(s.d, s.q, si, ti, index_base=1, max_spots=5)
    assert np.array_equal(count, out[1][:-1]) and np.array_equal(_bits(cost), _bits(out[2][:-1]))
    assert np.array_equal(start, out[3][:-1]) and np.array_equal(end, out[4][:-1])
    dcount, dcost, dstart, dend = s.e.dtw_spot_all_device(s.d, s.q, si, ti, index_base=1, max_spots=5)
    assert dcount.is_cuda and dcost.is_cuda and dstart.is_cuda and dend.is_cuda and tuple(dcost.shape) == (10, 5)
    assert np.array_equal(dcount.cpu().numpy().view(np.uint32), count) and np.array_equal(_bits(dcost.cpu().numpy()), _bits(cost))
    assert np.array_equal(dstart.cpu().numpy().view(np.uint32), start) and np.array_equal(dend.cpu().numpy().view(np.uint32), end)
    tm = s.e.timings()
    assert tm["n_pairs"] == si.size and tm["main_ms"] > 0
    s.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------

def test_every_listed_error_leaves_the_outputs_untouched():
    rng = np.random.default_rng(0xE78)
    dim = 12
    mk = lambda f: rng.integers(-2, 3, size=(f, dim)).astype(np.float64)
    s = _Sets([mk(20), mk(9), mk(30), mk(4)], [mk(5), mk(8), mk(3)], dim, squared=True)
    L, ctx = nat.lib(), s.e.ctx
    idx = np.array([0, 1, 2], dtype=np.uint32)
    assert _raw(s, idx, k=4)[0] == nat.SSYM_OK

    def call(want, **kw):
        kw.setdefault("k", 4)
        out = _raw(s, kw.pop("src_idx", idx), **kw)
        assert out[0] == want and _untouched(out), (out[0], kw)
        assert L.ssym_last_error(ctx)

    inv = nat.SSYM_E_INVALID
    call(inv, k=0)
    call(inv, k=65)
    call(inv, max_cost=[1.0, np.nan, 2.0])
    for name in ("count", "cost", "start", "end"):
        call(inv, null=(name,))
    call(inv, src_idx=np.array([0, 4, 1], dtype=np.uint32))                               # beyond the dictionary
    call(inv, src_idx=np.array([1, 2, 0], dtype=np.uint32), base=1)                       # below index_base
    call(inv, tgt_idx=np.array([0, 3, 1], dtype=np.uint32))                               # beyond the targets
    call(inv, src_idx=np.array([0, 1, 2, 3], dtype=np.uint32))                            # NULL tgt_idx, 4 pairs, 3 targets
    call(inv, src_idx=np.array([0, 4, 1], dtype=np.uint32), null=("cost",))               # two faults in one call

    def call_handles(d, q, n=3):
        count, cost = np.full(4, SENT32, dtype=np.uint32), np.full((4, 4), SENTF)
        start, end = np.full((4, 4), SENT32, dtype=np.uint32), np.full((4, 4), SENT32, dtype=np.uint32)
        rc = L.ssym_dtw_spot_all(ctx, d, q, idx.ctypes.data, None, n, 0, 4, None, count.ctypes.data, cost.ctypes.data,
                                 start.ctypes.data, end.ctypes.data, 0)
        assert _untouched((rc, count, cost, start, end)), rc
        return rc

    assert call_handles(None, s.q.ptr) == inv and call_handles(s.d.ptr, None) == inv
    other = s.e.queries(np.zeros(3 * 13), np.array([0, 1, 2, 3], dtype=np.uint64), 13)    # a set of another dimension
    assert call_handles(s.d.ptr, other.ptr) == inv
    empty = s.e.dictionary(np.zeros(0), np.zeros(1, dtype=np.uint64), dim)
    assert call_handles(empty.ptr, s.q.ptr) == nat.SSYM_E_EMPTY_DICT
    with pytest.raises(nat.EmptyDictionaryError):
        s.e.dtw_spot_all(empty, s.q, [0])
    # n_pairs = 0 succeeds and does nothing, even with nothing to write to and an empty dictionary
    assert call_handles(s.d.ptr, s.q.ptr, n=0) == nat.SSYM_OK and call_handles(empty.ptr, s.q.ptr, n=0) == nat.SSYM_OK
    assert L.ssym_dtw_spot_all(ctx, s.d.ptr, s.q.ptr, None, None, 0, 0, 8, None, None, None, None, None, 0) == nat.SSYM_OK
    count, cost, start, end = s.e.dtw_spot_all(s.d, s.q, [], max_spots=3)
    assert count.size == 0 and cost.shape == start.shape == end.shape == (0, 3)
    s.close()


def test_limits_of_target_length_dim_and_source_length():
    rng = np.random.default_rng(0x4097)
    mk = lambda f: rng.integers(-2, 3, size=(f, 2)).astype(np.float64)
    s = _Sets([mk(50), mk(300)], [mk(4096), mk(4097), mk(3)], 2, squared=True)
    si, ti = np.array([0, 1], np.uint32), np.array([0, 2], np.uint32)               # at the limit
    _check(s, si, ti, _raw(s, si, ti, k=2), 2)
    out = _raw(s, np.array([0], np.uint32), np.array([1], np.uint32), k=2)
    assert out[0] == nat.SSYM_E_UNSUPPORTED and b"4096" in nat.lib().ssym_last_error(s.e.ctx) and _untouched(out)
    s.close()
    wide = _Sets([np.zeros((3, 65))], [np.zeros((3, 65))], 65)
    out = _raw(wide, np.array([0], dtype=np.uint32), k=2)
    assert out[0] == nat.SSYM_E_UNSUPPORTED and _untouched(out)
    wide.close()
    # one source over the 2^24-frame limit beside one of 200 frames: a dim-1 dictionary, 128 MiB, made once
    frames = 2 ** 24 + 1
    e = Engine(metric="dtw", dtype="f64")
    flat = np.zeros(frames + 200)
    long_ = _Sets.__new__(_Sets)
    long_.e, long_.d = e, e.dictionary(flat, np.array([0, frames, frames + 200], dtype=np.uint64), 1)
    long_.q = e.queries(np.zeros(4), np.array([0, 4], dtype=np.uint64), 1)
    out = _raw(long_, np.array([1, 0], dtype=np.uint32), np.array([0, 0], dtype=np.uint32), k=2)
    assert out[0] == nat.SSYM_E_UNSUPPORTED and b"16777216" in nat.lib().ssym_last_error(e.ctx) and _untouched(out)
    out = _raw(long_, np.array([1], dtype=np.uint32), k=2)              # the short source alone is fine
    assert out[0] == nat.SSYM_OK and out[1][0] == 2 and out[2][0].tolist() == [0.0, 0.0]
    e.close()


@pytest.mark.parametrize("kw", [dict(band=0), dict(band=32), dict(metric="refcos")])
def test_banded_and_refcos_contexts_are_refused(kw):
    rng = np.random.default_rng(1)
    s = _Sets([rng.standard_normal((50, 12))], [rng.standard_normal((6, 12))], 12, **kw)
    out = _raw(s, np.array([0], dtype=np.uint32), k=3)
    assert out[0] == nat.SSYM_E_UNSUPPORTED and _untouched(out)
    assert (b"refcos" if "metric" in kw else b"band") in nat.lib().ssym_last_error(s.e.ctx)
    with pytest.raises(nat.SsymError):
        s.e.dtw_spot_all(s.d, s.q, [0])
    s.close()


# ---- 8. SoundDictionary.spot_all -----------------------------------------------------------------------------------------

def test_spot_all_merges_the_plants_of_two_recordings_and_feeds_cut_and_align():
    rng = np.random.default_rng(0x50A11)
    nc = 5
    tgt_f = rng.standard_normal((8, nc))
    other_f = rng.standard_normal((5, nc))

    def recording(frames, plants, name):
        f = 4.0 + rng.standard_normal((frames, nc))                   # noise away from the target's frames
        for at in plants:
            f[at:at + 8] = tgt_f
        return Sound(rng.standard_normal(frames * HOP), 8000.0, f.reshape(-1), name, ncoeffs=nc)

    e = Engine(metric="dtw", dtype="f64")
    d = SoundDictionary(engine=e)
    d.sounds = [recording(90, (10, 60), "twice"), recording(70, (33,), "once")]
    targets = [Sound(rng.standard_normal(8 * HOP), 8000.0, tgt_f.reshape(-1), "t", ncoeffs=nc),
               Sound(rng.standard_normal(5 * HOP), 8000.0, other_f.reshape(-1), "o", ncoeffs=nc)]
    feats = [x.mfcc_arrays() for x in d.sounds]

    lists = d.spot_all(targets, max_spots=4, max_cost=0.0)
    assert [(sp.source_index, sp.start_frame, sp.end_frame, sp.cost) for sp in lists[0]] == \
        [(0, 10, 17, 0.0), (0, 60, 67, 0.0), (1, 33, 40, 0.0)]                    # by (cost, source index, end)
    assert lists[1] == []
    # without a threshold: per target the two recordings' lists merged by (cost, source index, end)
    lists = d.spot_all(targets, max_spots=4)
    for t, spots in enumerate(lists):
        want = []
        for r in range(2):
            count, cost, start, end = spot_all_ref.spot_all(feats[r], targets[t].mfcc_arrays(), 4)
            want += [(float(cost[m]), r, int(end[m]), int(start[m])) for m in range(count)]
        want.sort()
        assert [(sp.cost, sp.source_index, sp.end_frame, sp.start_frame) for sp in spots] == want
    assert [(sp.source_index, sp.start_frame) for sp in lists[0][:3]] == [(0, 10), (0, 60), (1, 33)]
    assert [[(sp.source_index, sp.end_frame) for sp in x] for x in SoundSequence.new(targets).spot_all_in_dictionary(d, max_spots=4)] == \
        [[(sp.source_index, sp.end_frame) for sp in x] for x in lists]
    # with indices: target t in recording indices[t] alone, a threshold per target
    given = d.spot_all(targets, indices=[1, 0], max_spots=3, max_cost=[0.0, np.inf])
    assert [(sp.source_index, sp.start_frame, sp.end_frame) for sp in given[0]] == [(1, 33, 40)]
    count, cost, start, end = spot_all_ref.spot_all(feats[0], targets[1].mfcc_arrays(), 3)
    assert [(sp.source_index, sp.start_frame, sp.end_frame) for sp in given[1]] == [(0, int(start[m]), int(end[m])) for m in range(count)]
    assert np.array_equal(_bits([sp.cost for sp in given[1]]), _bits(cost[:count]))
    # cut(spots) then align: every cut aligns with the target at the spot's cost
    spots = lists[0]
    cut = d.cut(spots)
    al = cut.align([targets[0]] * len(spots), indices=np.arange(len(spots)))
    for sp, x in zip(spots, al):
        assert _bits(x.cost) == _bits(sp.cost) and x.frame_map.size == 8
    e.close()
