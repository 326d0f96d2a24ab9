"""ssym_dtw_spot and ssym_spot_queries on the GPU against the numpy restatement (tests/spot_ref.py): cost bit for bit,
start and end equal, at every shape edge of the kernel (64-row chunks and their hand-off, the 128-frame ring and its
refill, the padding edges of every DIMR, the grid stride), with real ties, through every way of listing pairs, end to end
on the recordings, and every error the header lists.  Outputs are sentinel-filled before every call."""
import os

import numpy as np
import pytest

import spot_ref
import wave_lds
from soundsym_amd import Engine, Sound, SoundDictionary, SoundSequence, Spot
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT32, SENTF = 0xDEADBEEF, -12345.5
NO = nat.NO_MATCH


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class _Sets:
    """An engine with a resident dictionary and query set made from lists of [frames, dim] arrays."""

    def __init__(self, src, tgt, dim, dtype="f64", band=-1, squared=False, metric="dtw"):
        self.src, self.tgt, self.dim, self.squared = src, tgt, dim, squared
        npd = np.float32 if dtype == "f32" else np.float64
        self.e = Engine(metric=metric, dtype=dtype, band=band, squared=squared)
        sf, so = pack_segments(src, dim, npd)
        tf, to = pack_segments(tgt, dim, npd)
        self.d, self.q = self.e.dictionary(sf, so, dim), self.e.queries(tf, to, dim)
        self._ref = {}

    def close(self):
        self.e.close()

    def ref(self, s, t):
        """(cost, start, end, rows tied for the end, tied cells on the way to the start), computed once per pair."""
        if (s, t) not in self._ref:
            self._ref[(s, t)] = spot_ref.spot(np.asarray(self.src[s], np.float64), np.asarray(self.tgt[t], np.float64),
                                              self.squared, want_ties=True)
        return self._ref[(s, t)]


def _raw(sets, src_idx, tgt_idx=None, base=0, device=False):
    """ssym_dtw_spot through ctypes into sentinel-filled outputs (one slot more than the pairs): (rc, cost, start, end)."""
    src = np.ascontiguousarray(src_idx, dtype=np.uint32)
    tgt = None if tgt_idx is None else np.ascontiguousarray(tgt_idx, dtype=np.uint32)
    n = src.size
    cost = np.full(n + 1, SENTF)
    start = np.full(n + 1, SENT32, dtype=np.uint32)
    end = np.full(n + 1, SENT32, dtype=np.uint32)
    tp = None if tgt is None else tgt.ctypes.data
    L = nat.lib()
    if device:
        import torch
        dc, ds, de = (torch.from_numpy(cost).cuda(), torch.from_numpy(start.view(np.int32)).cuda(),
                      torch.from_numpy(end.view(np.int32)).cuda())
        rc = L.ssym_dtw_spot(sets.e.ctx, sets.d.ptr, sets.q.ptr, src.ctypes.data, tp, n, base, dc.data_ptr(),
                             ds.data_ptr(), de.data_ptr(), nat.OUT_DEVICE)
        torch.cuda.synchronize()
        cost, start, end = dc.cpu().numpy(), ds.cpu().numpy().view(np.uint32), de.cpu().numpy().view(np.uint32)
    else:
        rc = L.ssym_dtw_spot(sets.e.ctx, sets.d.ptr, sets.q.ptr, src.ctypes.data, tp, n, base, cost.ctypes.data,
                             start.ctypes.data, end.ctypes.data, 0)
    return rc, cost, start, end


def _check(sets, src_idx, tgt_idx, out, base=0):
    """Every pair of a call equal to the restatement; the slot beyond the pairs untouched.  Returns (pairs with a tie in
    the end column, pairs with a tie on the way to the start)."""
    rc, cost, start, end = out
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(sets.e.ctx)
    n = len(src_idx)
    assert cost[n] == SENTF and start[n] == SENT32 and end[n] == SENT32
    end_ties = start_ties = 0
    for p in range(n):
        t = p if tgt_idx is None else int(tgt_idx[p])
        if int(src_idx[p]) == NO:
            want = (float("inf"), NO, NO, 0, 0)
        else:
            want = sets.ref(int(src_idx[p]) - base, t)
        assert _bits(cost[p]) == _bits(want[0]), (p, cost[p], want[0])
        assert (int(start[p]), int(end[p])) == (want[1], want[2]), (p, int(start[p]), int(end[p]), want)
        end_ties += int(want[3] > 1)
        start_ties += int(want[4] > 0)
    return end_ties, start_ties


def _all_pairs(n_src, n_tgt):
    return np.repeat(np.arange(n_src, dtype=np.uint32), n_tgt), np.tile(np.arange(n_tgt, dtype=np.uint32), n_src)


def _frames(rng, f, dim, kind):
    if kind == "int":
        return rng.integers(0, 3, size=(f, dim)).astype(np.float64)        # {0, 1, 2}: exact sums, real ties
    return rng.standard_normal((f, dim)).astype(np.float32)


SRC_FRAMES = [1, 2, 63, 64, 65, 128, 129, 1000]       # chunk edges, the chunk-to-chunk hand-off, the end across chunks
TGT_FRAMES = [1, 2, 63, 64, 65, 127, 128, 129, 200]   # the ring and its refill


# ---- 1. shapes, cost modes, dtypes, ties --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind,squared", [("int", True), ("real", False), ("real", True)])
def test_every_source_length_against_every_target_length(kind, squared, dtype):
    rng = np.random.default_rng(0x5107 + squared)
    dim = 2 if kind == "int" else 13
    src = [_frames(rng, f, dim, kind) for f in SRC_FRAMES]
    tgt = [_frames(rng, f, dim, kind) for f in TGT_FRAMES]
    s = _Sets(src, tgt, dim, dtype=dtype, squared=squared)
    si, ti = _all_pairs(len(src), len(tgt))
    out = _raw(s, si, ti)
    end_ties, start_ties = _check(s, si, ti, out)
    # a source shorter than the target still has a spot: the path dwells on source frames
    short = (np.array(SRC_FRAMES)[si] < np.array(TGT_FRAMES)[ti])
    assert short.sum() >= 20 and np.isfinite(out[1][:-1][short]).all()
    s.close()
    print("pairs with a tie in the end column: %d, on the way to the start: %d (of %d)" % (end_ties, start_ties, si.size))
    if kind == "int":
        assert end_ties >= 1 and start_ties >= 1, (end_ties, start_ties)   # the tie rules are exercised, not just stated


@pytest.mark.parametrize("dim", [1, 12, 13, 14, 15, 16, 17, 40, 41, 64])
def test_padding_edges_of_every_dimr(dim):
    rng = np.random.default_rng(0xD1 + dim)
    end_ties = start_ties = 0
    for kind, squared in (("int", True), ("real", False)):
        src = [_frames(rng, f, dim, kind) for f in (70, 130, 9)]
        tgt = [_frames(rng, f, dim, kind) for f in (5, 66, 130)]
        s = _Sets(src, tgt, dim, dtype="f64", squared=squared)
        si, ti = _all_pairs(3, 3)
        a, b = _check(s, si, ti, _raw(s, si, ti))
        end_ties, start_ties = end_ties + a, start_ties + b
        s.close()
    if dim <= 2:
        assert end_ties >= 1 and start_ties >= 1, (end_ties, start_ties)


_LONG = [c for c in wave_lds.CROSSINGS if c[1] > 130]       # (the dim 64 / 41 crossing at 65 frames: test_padding_edges_of_every_dimr)


@pytest.mark.parametrize("dim,fb,above", _LONG)
def test_both_sides_of_every_lds_crossing(dim, fb, above):
    """The launch's dynamic LDS goes by the longest listed target: one call per length, on the side of 64 KiB the case
    names (above it the launch sets MaxDynamicSharedMemorySize first), up to the 116736 bytes of dim 64 x 4096 frames."""
    need = wave_lds.spot_lds_bytes(dim, fb)
    assert (need > wave_lds.LIMIT) == above, (dim, fb, need)
    rng = np.random.default_rng(0x1D5 + 4099 * dim + fb)
    s = _Sets([_frames(rng, f, dim, "real") for f in (65, 130)], [_frames(rng, fb, dim, "real")], dim)
    si, ti = _all_pairs(2, 1)
    out = _raw(s, si, ti)
    _check(s, si, ti, out)
    assert np.isfinite(out[1][:2]).all()
    _check_queries(s, _raw_queries(s))
    s.close()


def test_plants_at_the_edges_and_late_in_a_long_source():
    rng = np.random.default_rng(0x91A7)
    dim = 13
    a = rng.standard_normal((150, dim))
    long_ = rng.standard_normal((20000, dim))
    mid = rng.standard_normal((200, dim))
    src = [a, long_, mid]
    tgt = [a[:30].copy(), a[120:].copy(), long_[19950:19990].copy(), mid[57:97].copy()]
    for squared in (False, True):
        s = _Sets(src, tgt, dim, squared=squared)
        si, ti = np.array([0, 0, 1, 2], np.uint32), np.arange(4, dtype=np.uint32)
        out = _raw(s, si, ti)
        _check(s, si, ti, out)
        assert out[1][:4].tolist() == [0.0] * 4
        assert out[2][:4].tolist() == [0, 120, 19950, 57] and out[3][:4].tolist() == [29, 149, 19989, 96]
        s.close()


def test_cost_is_the_exact_kernels_cost_of_the_span_and_the_least_over_all_spans():
    """Properties 2 and 3 through the GPU alone: ssym_pair_matrix(exact = 1) on the cut spans."""
    rng = np.random.default_rng(0x9209)
    dim = 13
    for squared in (False, True):
        src = [rng.standard_normal((f, dim)) for f in (90, 200, 64, 12)]
        tgt = [rng.standard_normal((f, dim)) for f in (7, 40, 70)]
        s = _Sets(src, tgt, dim, squared=squared)
        si, ti = _all_pairs(4, 3)
        rc, cost, start, end = _raw(s, si, ti)
        assert rc == nat.SSYM_OK
        cuts = [src[si[p]][start[p]:end[p] + 1] for p in range(si.size)]
        c = _Sets(cuts, tgt, dim, squared=squared)
        plain = c.e.pair_matrix(c.d, c.q, exact=True)
        for p in range(si.size):
            assert _bits(cost[p]) == _bits(plain[p, ti[p]]), p
        c.close()
        # every span of the 12-frame source: the spot's cost is the least, its end the first that reaches it
        spans = [(a, b) for b in range(12) for a in range(b + 1)]
        c = _Sets([src[3][a:b + 1] for a, b in spans], tgt, dim, squared=squared)
        plain = c.e.pair_matrix(c.d, c.q, exact=True)
        for t in range(3):
            p = 3 * 3 + t
            assert _bits(cost[p]) == _bits(plain[:, t].min())
            assert spans[int(np.argmin(plain[:, t]))][1] == end[p]          # spans are listed by ascending end
            assert _bits(plain[spans.index((int(start[p]), int(end[p]))), t]) == _bits(cost[p])
        c.close()
        s.close()


# ---- 2. pair lists and batches -------------------------------------------------------------------------------------------

def test_5000_tiny_pairs_in_one_call():
    rng = np.random.default_rng(0x5000)
    dim = 3
    src = [rng.integers(0, 3, size=(int(rng.integers(1, 13)), dim)).astype(np.float64) for _ in range(40)]
    tgt = [rng.integers(0, 3, size=(int(rng.integers(1, 9)), dim)).astype(np.float64) for _ in range(30)]
    s = _Sets(src, tgt, dim, squared=True)
    si = rng.integers(0, 40, size=5000).astype(np.uint32)
    ti = rng.integers(0, 30, size=5000).astype(np.uint32)
    end_ties, start_ties = _check(s, si, ti, _raw(s, si, ti))
    assert end_ties >= 1 and start_ties >= 1
    s.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pairings_index_base_no_match_empty_segments_and_device_outputs(dtype):
    rng = np.random.default_rng(0x9A13)
    dim = 13
    mk = lambda f: rng.integers(-3, 4, size=(f, dim)).astype(np.float64)
    src = [mk(f) for f in (30, 0, 90, 1, 150, 64, 0, 77, 5)]
    tgt = [mk(f) for f in (10, 0, 33, 1, 80, 64, 7)]
    s = _Sets(src, tgt, dim, dtype=dtype, squared=True)
    first = np.array([3, 0, 8, 8, 1, 2, 5], dtype=np.uint32)
    a = _raw(s, first)                                               # tgt_idx = NULL: pair p uses target p
    b = _raw(s, first, np.arange(7, dtype=np.uint32))
    _check(s, first, None, a)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    assert np.isinf(a[1][[1, 4]]).all() and (a[2][[1, 4]] == NO).all() and (a[3][[1, 4]] == NO).all()   # empty target, empty source
    _check(s, first[:3], None, _raw(s, first[:3]))                   # fewer pairs than targets
    # repeats, any pairing, SSYM_NO_MATCH, index_base = 1
    si = np.array([5, 5, 9, NO, 1, 5, NO, 9, 2, 7], dtype=np.uint32)
    ti = np.array([6, 6, 0, 2, 5, 6, 0, 0, 4, 1], dtype=np.uint32)
    out = _raw(s, si, ti, base=1)
    _check(s, si, ti, out, base=1)
    for p in (3, 6, 8, 9):                                           # no match, no match, empty source, empty target
        assert np.isinf(out[1][p]) and out[2][p] == NO and out[3][p] == NO
    dev = _raw(s, si, ti, base=1, device=True)
    for x, y in zip(out[1:], dev[1:]):
        assert np.array_equal(x, y)
    # the Python layer
    cost, start, end = s.e.dtw_spot(s.d, s.q, si, ti, index_base=1)
    assert np.array_equal(_bits(cost), _bits(out[1][:-1])) and np.array_equal(start, out[2][:-1]) and np.array_equal(end, out[3][:-1])
    dcost, dstart, dend = s.e.dtw_spot_device(s.d, s.q, si, ti, index_base=1)
    assert dcost.is_cuda and dstart.is_cuda and dend.is_cuda
    assert np.array_equal(_bits(dcost.cpu().numpy()), _bits(cost))
    assert np.array_equal(dstart.cpu().numpy().view(np.uint32), start) and np.array_equal(dend.cpu().numpy().view(np.uint32), end)
    tm = s.e.timings()
    assert tm["n_pairs"] == si.size and tm["main_ms"] > 0
    s.close()


# ---- 3. ssym_spot_queries ------------------------------------------------------------------------------------------------

def _raw_queries(sets, base=0, device=False):
    m = sets.q.n
    idx, start, end = (np.full(m + 1, SENT32, dtype=np.uint32) for _ in range(3))
    cost = np.full(m + 1, SENTF)
    L = nat.lib()
    if device:
        import torch
        di, ds, de = (torch.from_numpy(x.view(np.int32)).cuda() for x in (idx, start, end))
        dc = torch.from_numpy(cost).cuda()
        rc = L.ssym_spot_queries(sets.e.ctx, sets.d.ptr, sets.q.ptr, base, di.data_ptr(), dc.data_ptr(), ds.data_ptr(),
                                 de.data_ptr(), nat.OUT_DEVICE)
        torch.cuda.synchronize()
        idx, start, end = (x.cpu().numpy().view(np.uint32) for x in (di, ds, de))
        cost = dc.cpu().numpy()
    else:
        rc = L.ssym_spot_queries(sets.e.ctx, sets.d.ptr, sets.q.ptr, base, idx.ctypes.data, cost.ctypes.data,
                                 start.ctypes.data, end.ctypes.data, 0)
    return rc, idx, cost, start, end


def _check_queries(sets, out, base=0):
    rc, idx, cost, start, end = out
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(sets.e.ctx)
    m = len(sets.tgt)
    assert idx[m] == SENT32 and cost[m] == SENTF and start[m] == SENT32 and end[m] == SENT32
    for t in range(m):
        want = spot_ref.spot_best([np.asarray(a, np.float64) for a in sets.src], np.asarray(sets.tgt[t], np.float64),
                                  sets.squared)
        want_idx = NO if want[0] == NO else want[0] + base
        assert (int(idx[t]), int(start[t]), int(end[t])) == (want_idx, want[2], want[3]), (t, want)
        assert _bits(cost[t]) == _bits(want[1]), t


@pytest.mark.parametrize("dtype,squared", [("f64", False), ("f32", True)])
def test_spot_queries_five_sources_seven_targets(dtype, squared):
    rng = np.random.default_rng(0x5077)
    dim = 13
    src = [rng.standard_normal((f, dim)).astype(np.float32) for f in (300, 64, 0, 129, 1000)]
    tgt = [rng.standard_normal((f, dim)).astype(np.float32) for f in (20, 1, 65, 0, 130, 7)]
    tgt.append(src[4][900:940].copy())                               # planted in the last source
    s = _Sets(src, tgt, dim, dtype=dtype, squared=squared)
    out = _raw_queries(s)
    _check_queries(s, out)
    assert (int(out[1][6]), out[2][6], int(out[3][6]), int(out[4][6])) == (4, 0.0, 900, 939)
    assert out[1][3] == NO and np.isinf(out[2][3]) and out[3][3] == NO and out[4][3] == NO      # the empty target
    based = _raw_queries(s, base=100)
    _check_queries(s, based, base=100)
    assert based[1][3] == NO                                         # a missing entry carries no base
    dev = _raw_queries(s, base=100, device=True)
    for x, y in zip(based[1:], dev[1:]):
        assert np.array_equal(x, y)
    idx, cost, start, end = s.e.spot_queries(s.d, s.q, index_base=100)
    assert np.array_equal(idx, based[1][:-1]) and np.array_equal(_bits(cost), _bits(based[2][:-1]))
    assert np.array_equal(start, based[3][:-1]) and np.array_equal(end, based[4][:-1])
    tm = s.e.timings()
    assert tm["n_pairs"] == 5 * 7 and tm["main_ms"] > 0 and tm["reduce_ms"] > 0
    s.close()


def test_spot_queries_identical_recordings_and_no_targets():
    rng = np.random.default_rng(0x1DE)
    dim = 12
    rec = rng.integers(0, 3, size=(140, dim)).astype(np.float64)
    src = [rng.integers(0, 3, size=(50, dim)).astype(np.float64), rec, rec.copy(), rec.copy()]
    tgt = [rec[20:50].copy(), rec[100:140].copy(), rng.integers(0, 3, size=(9, dim)).astype(np.float64)]
    s = _Sets(src, tgt, dim, squared=True)
    out = _raw_queries(s)
    _check_queries(s, out)
    assert out[1][:2].tolist() == [1, 1] and out[2][:2].tolist() == [0.0, 0.0]       # the lower index wins
    # no targets: succeeds and writes nothing
    none = s.e.queries(np.zeros(0), np.zeros(1, dtype=np.uint64), dim)
    word, cost = np.full(3, SENT32, dtype=np.uint32), np.full(1, SENTF)
    rc = nat.lib().ssym_spot_queries(s.e.ctx, s.d.ptr, none.ptr, 0, word.ctypes.data, cost.ctypes.data, word[1:].ctypes.data,
                                     word[2:].ctypes.data, 0)
    assert rc == nat.SSYM_OK and (word == SENT32).all() and cost[0] == SENTF
    assert nat.lib().ssym_spot_queries(s.e.ctx, s.d.ptr, none.ptr, 0, None, None, None, None, 0) == nat.SSYM_OK
    s.close()


# ---- 4. errors -----------------------------------------------------------------------------------------------------------

def test_every_listed_error_leaves_the_outputs_untouched():
    rng = np.random.default_rng(0xE78)
    dim = 12
    mk = lambda f: rng.integers(-2, 3, size=(f, dim)).astype(np.float64)
    s = _Sets([mk(20), mk(9), mk(30), mk(4)], [mk(5), mk(8), mk(3)], dim, squared=True)
    L, ctx = nat.lib(), s.e.ctx
    idx = np.array([0, 1, 2], dtype=np.uint32)
    assert _raw(s, idx)[0] == nat.SSYM_OK

    def call(d=s.d.ptr, q=s.q.ptr, src_idx=idx, tgt_idx=None, n=3, base=0, null=()):
        cost, start, end = np.full(4, SENTF), np.full(4, SENT32, dtype=np.uint32), np.full(4, SENT32, dtype=np.uint32)
        ptr = lambda name, arr: None if name in null or arr is None else arr.ctypes.data
        rc = L.ssym_dtw_spot(ctx, d, q, ptr("src", src_idx), ptr("tgt", tgt_idx), n, base, ptr("cost", cost),
                             ptr("start", start), ptr("end", end), 0)
        assert (cost == SENTF).all() and (start == SENT32).all() and (end == SENT32).all(), rc
        return rc

    def call_q(d=s.d.ptr, q=s.q.ptr, null=()):
        cost = np.full(4, SENTF)
        words = {k: np.full(4, SENT32, dtype=np.uint32) for k in ("idx", "start", "end")}
        ptr = lambda name, arr: None if name in null else arr.ctypes.data
        rc = L.ssym_spot_queries(ctx, d, q, 0, ptr("idx", words["idx"]), ptr("cost", cost), ptr("start", words["start"]),
                                 ptr("end", words["end"]), 0)
        assert (cost == SENTF).all() and all((w == SENT32).all() for w in words.values()), rc
        return rc

    inv = nat.SSYM_E_INVALID
    assert call(d=None) == inv and call(q=None) == inv and call_q(d=None) == inv and call_q(q=None) == inv
    for name in ("src", "cost", "start", "end"):
        assert call(null=(name,)) == inv, name
        assert L.ssym_last_error(ctx)
    for name in ("idx", "cost", "start", "end"):
        assert call_q(null=(name,)) == inv, name
        assert L.ssym_last_error(ctx)
    assert call(src_idx=np.array([0, 4, 1], dtype=np.uint32)) == inv                      # beyond the dictionary
    assert call(src_idx=np.array([1, 2, 0], dtype=np.uint32), base=1) == inv              # below index_base
    assert call(tgt_idx=np.array([0, 3, 1], dtype=np.uint32)) == inv                      # beyond the targets
    assert call(src_idx=np.array([0, 1, 2, 3], dtype=np.uint32), n=4) == inv              # NULL tgt_idx, 4 pairs, 3 targets
    assert call(src_idx=np.array([0, 4, 1], dtype=np.uint32), null=("cost",)) == inv      # two faults in one call
    other = s.e.queries(np.zeros(3 * 13), np.array([0, 1, 2, 3], dtype=np.uint64), 13)    # a set of another dimension
    assert call(q=other.ptr) == inv and call_q(q=other.ptr) == inv
    empty = s.e.dictionary(np.zeros(0), np.zeros(1, dtype=np.uint64), dim)
    assert call(d=empty.ptr) == nat.SSYM_E_EMPTY_DICT and call_q(d=empty.ptr) == nat.SSYM_E_EMPTY_DICT
    with pytest.raises(nat.EmptyDictionaryError):
        s.e.dtw_spot(empty, s.q, [0])
    # n_pairs = 0 succeeds and does nothing, even with nothing to write to and an empty dictionary
    assert call(n=0) == nat.SSYM_OK and call(d=empty.ptr, n=0) == nat.SSYM_OK
    assert L.ssym_dtw_spot(ctx, s.d.ptr, s.q.ptr, None, None, 0, 0, None, None, None, 0) == nat.SSYM_OK
    cost, start, end = s.e.dtw_spot(s.d, s.q, [])
    assert cost.size == start.size == end.size == 0
    s.close()


def test_limits_of_target_length_and_dim():
    rng = np.random.default_rng(0x4097)
    mk = lambda f: rng.integers(-2, 3, size=(f, 2)).astype(np.float64)
    s = _Sets([mk(50), mk(5000)], [mk(4096), mk(4097), mk(3)], 2, squared=True)
    # at the limit (and a source beyond 4096 frames: the source has no limit of the kernel's)
    si, ti = np.array([0, 1, 1], np.uint32), np.array([0, 0, 2], np.uint32)
    _check(s, si, ti, _raw(s, si, ti))
    out = _raw(s, np.array([0], np.uint32), np.array([1], np.uint32))
    assert out[0] == nat.SSYM_E_UNSUPPORTED and b"4096" in nat.lib().ssym_last_error(s.e.ctx)
    assert (out[1] == SENTF).all() and (out[2] == SENT32).all() and (out[3] == SENT32).all()
    q = _raw_queries(s)
    assert q[0] == nat.SSYM_E_UNSUPPORTED and (q[1] == SENT32).all() and (q[2] == SENTF).all()
    s.close()
    wide = _Sets([np.zeros((3, 65))], [np.zeros((3, 65))], 65)
    out = _raw(wide, np.array([0], dtype=np.uint32))
    assert out[0] == nat.SSYM_E_UNSUPPORTED and (out[1] == SENTF).all() and (out[2] == SENT32).all()
    assert _raw_queries(wide)[0] == nat.SSYM_E_UNSUPPORTED
    wide.close()


@pytest.mark.parametrize("kw", [dict(band=0), dict(band=32), dict(metric="refcos")])
def test_banded_and_refcos_contexts_are_refused(kw):
    rng = np.random.default_rng(1)
    s = _Sets([rng.standard_normal((50, 12))], [rng.standard_normal((6, 12))], 12, **kw)
    out = _raw(s, np.array([0], dtype=np.uint32))
    assert out[0] == nat.SSYM_E_UNSUPPORTED and (out[1] == SENTF).all() and (out[2] == SENT32).all() and (out[3] == SENT32).all()
    assert (b"refcos" if "metric" in kw else b"band") in nat.lib().ssym_last_error(s.e.ctx)
    q = _raw_queries(s)
    assert q[0] == nat.SSYM_E_UNSUPPORTED and (q[1] == SENT32).all() and (q[2] == SENTF).all()
    with pytest.raises(nat.SsymError):
        s.e.dtw_spot(s.d, s.q, [0])
    with pytest.raises(nat.SsymError):
        s.e.spot_queries(s.d, s.q)
    s.close()


# ---- 5. end to end on the recordings ---------------------------------------------------------------------------------------

def test_spot_cut_and_warp_on_the_reference_recordings():
    from soundsym_amd import io as sio
    from soundsym_amd.api import HOP, NCOEFFS, frame_features
    gold = os.path.join(ROOT, "tests", "golden", "audio")
    e = Engine(metric="dtw", dtype="f64")
    t_smp, t_rate = sio.read_wav(os.path.join(gold, "sample.wav"))
    d_smp, d_rate = sio.read_wav(os.path.join(gold, "Section_7_1.wav"))
    whole = Sound(t_smp, t_rate, frame_features(t_smp, t_rate, engine=e))
    seg = 16 * HOP
    cut_up = SoundDictionary.from_segments(whole, [seg] * (t_smp.size // seg), engine=e)
    targets = cut_up.sounds[::24]                                     # 12 segments of 16 frames across the recording
    assert len(targets) == 12 and all(t.num_frames() == 16 for t in targets)
    # the dictionary: the other recording whole, and a stretch of it that holds no better spot than the whole
    rec = Sound(d_smp, d_rate, frame_features(d_smp, d_rate, engine=e), "Section_7_1")
    part = Sound(d_smp[:300 * HOP], d_rate, rec.mfcc_arrays()[:300].reshape(-1).copy(), "head")
    dictionary = SoundDictionary(engine=e)
    dictionary.sounds = [part, rec]
    assert rec.num_frames() == 1981

    spots = dictionary.spot(targets)
    assert len(spots) == 12 and all(isinstance(x, Spot) and x for x in spots)
    feats = [x.mfcc_arrays() for x in dictionary.sounds]
    for t, sp in enumerate(spots):
        want = spot_ref.spot_best(feats, targets[t].mfcc_arrays())
        assert (sp.source_index, sp.start_frame, sp.end_frame) == (want[0], want[2], want[3]), (t, sp, want)
        assert _bits(sp.cost) == _bits(want[1])
    assert [x.source_index for x in SoundSequence.new(targets).spot_in_dictionary(dictionary)] == [x.source_index for x in spots]
    given = dictionary.spot(targets[:4], indices=[1, 0, 1, 1])
    for t, sp in enumerate(given):
        want = spot_ref.spot(feats[[1, 0, 1, 1][t]], targets[t].mfcc_arrays())
        assert (sp.source_index, _bits(sp.cost), sp.start_frame, sp.end_frame) == ([1, 0, 1, 1][t], _bits(want[0]), want[1], want[2])

    # cut(spots) feeds warp with indices = arange; a dictionary built by hand from the same spans gives the same samples
    cut = dictionary.cut(spots)
    order = np.arange(len(spots))
    got = cut.warp(targets, indices=order)
    by_hand = SoundDictionary(engine=e)
    for sp in spots:
        src = dictionary.sounds[sp.source_index]
        a, b = sp.start_frame * HOP, min((sp.end_frame + 1) * HOP, src.samples().size)
        by_hand.sounds.append(Sound(src.samples()[a:b], src.sample_rate(),
                                    src.mfccs()[sp.start_frame * NCOEFFS:(sp.end_frame + 1) * NCOEFFS]))
    want = by_hand.warp(targets, indices=order)
    assert got.size == sum(t.samples().size for t in targets) and np.array_equal(_bits(got), _bits(want))
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    # the cut aligns with its target at the spot's cost: the span's plain DTW (property 2 through the API)
    al = cut.align(targets, indices=order)
    for sp, x in zip(spots, al):
        assert _bits(x.cost) == _bits(sp.cost) and x.frame_map.size == 16
    e.close()
