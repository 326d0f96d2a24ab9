"""ssym_chain at every shape it accepts, against tests/tail_ref.py's fold fed with the oracle's values.

chain_argmin_kernel is one workgroup of 1024 threads: a thread folds s, s + 1024, ...; a wave reduces with shuffles;
thread 0 folds the 16 wave results.  The cases here make every one of those three levels decide: dictionaries larger
than one pass, ties across lanes, waves and passes, and the exit where nothing beats the fold's start.

refcos: indices and values bit for bit.  dtw: indices identical, costs to 1e-12 relative; index identity under a
tolerance is only a fair demand when the runner-up is not within rounding of the winner, so every dtw case first
checks ON THE ORACLE'S VALUES that at each step the two best keys are bit-equal (planted copies, which the GPU scores
bit-equal too) or more than 1e-9 relative apart."""
import ctypes
import math

import numpy as np
import pytest

import tail_ref
from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

SENT32, SENTF = 0xA5A5A5A5, -7.25


def _ragged(rng, n, dim, lo, hi, dtype=np.float64):
    return [rng.normal(size=(int(rng.integers(lo, hi + 1)), dim)).astype(dtype) for _ in range(n)]


class _Ref:
    """The chain by tail_ref on columns of oracle values (cached per query entry)."""

    def __init__(self, oracle, segs, dim, metric, band=-1, squared=False):
        self.o, self.dim, self.metric, self.band, self.squared = oracle, dim, metric, band, squared
        self.segs = [np.asarray(s, dtype=np.float64) for s in segs]
        self.sf, self.so = pack_segments(self.segs, dim)
        self.cols = {}

    def col(self, feats):
        f = np.ascontiguousarray(feats, dtype=np.float64).reshape(-1)
        off = np.array([0, f.size // self.dim], dtype=np.uint64)
        if self.metric == "refcos":
            return self.o.refcos_matrix(self.sf, self.so, f, off, self.dim)[:, 0]
        return self.o.dtw_match_all(self.sf, self.so, f, off, self.dim, band=self.band, squared=self.squared,
                                    want_matrix=True)[2][:, 0]

    def entry(self, i):
        if i not in self.cols:
            self.cols[i] = self.col(self.segs[i])
        return self.cols[i]

    def typical(self, rng, k):
        """k distances from where the values really lie (an entry's own column, a little off the values themselves),
        so that the chain wanders over the dictionary and does not sit on one extreme entry."""
        col = self.entry(int(rng.integers(0, len(self.segs))))
        col = col[np.isfinite(col)]
        if col.size == 0:
            return np.zeros(k)
        return rng.choice(col, size=k) * rng.uniform(0.97, 1.03, size=k)

    def chain(self, start, dist):
        refcos = self.metric == "refcos"
        start_col = self.col(start)
        idx, val = tail_ref.chain(self.entry, start_col, dist, 2.0 if refcos else math.inf, "key" if refcos else "value")
        if not refcos:                      # the precondition of comparing indices under a cost tolerance
            col = start_col
            for step, d in enumerate(dist):
                k1, k2 = tail_ref.best_two_keys(col, d)
                assert k1 == k2 or k2 == math.inf or k2 - k1 > 1e-9 * k2, (step, k1, k2)
                col = self.entry(int(idx[step]))
        return idx, val


def _check(e, d, ref, start, dist):
    want_idx, want_val = ref.chain(start, dist)         # (with the dtw precondition, before the GPU is consulted)
    idx, val = e.chain(d, start, dist)
    assert np.array_equal(idx.astype(np.int64), want_idx), (idx, want_idx)
    if ref.metric == "refcos":
        assert np.array_equal(val.view(np.uint64), want_val.view(np.uint64))
    else:
        fin = np.isfinite(want_val)
        assert np.array_equal(np.isfinite(val), fin) and np.array_equal(val[~fin], want_val[~fin])
        assert np.allclose(val[fin], want_val[fin], rtol=1e-12, atol=0)
    return idx, val


def _dict(e, segs, dim):
    f, o = pack_segments(segs, dim, e.np_dtype)
    return e.dictionary(f, o, dim)


# ---------------------------------------------------------------------------------------------------------
# dictionary sizes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000])
def test_refcos_sizes(oracle, n):
    rng = np.random.default_rng(0xC5A0 + n)
    segs = _ragged(rng, n, 12, 1, 8)
    start = rng.normal(size=(4, 12))
    ref = _Ref(oracle, segs, 12, "refcos")
    dist = np.concatenate([[ref.col(start)[n - 1], 1.0], ref.typical(rng, 38)])     # step 0 lands on the LAST entry
    e = Engine(metric="refcos", dtype="f64")
    idx, _ = _check(e, _dict(e, segs, 12), ref, start, dist)
    assert idx[0] == n - 1
    if n >= 1025:
        assert np.unique(idx).size >= 20                                # the chain moves
    e.close()


@pytest.mark.parametrize("n", [1, 2, 65, 1025, 1500])
def test_dtw_sizes(oracle, n):
    rng = np.random.default_rng(0xC5B0 + n)
    segs = _ragged(rng, n, 13, 1, 20, np.float32)
    start = rng.normal(size=(7, 13)).astype(np.float32)
    ref = _Ref(oracle, segs, 13, "dtw")
    dist = np.concatenate([[ref.col(start)[n - 1], 0.0], ref.typical(rng, 7)])      # step 0 lands on the LAST entry
    e = Engine(metric="dtw", dtype="f32")
    idx, _ = _check(e, _dict(e, segs, 13), ref, start, dist)
    assert idx[0] == n - 1
    if n >= 1025:
        assert np.unique(idx).size >= 5
    e.close()


# ---------------------------------------------------------------------------------------------------------
# ties placed by position: copies of one entry at s, s + 1, s + 64, s + 1024 (, s + 4096); the lowest copy must win;
# then the lowest copy is taken away, so that the winner sits in a later lane, a later wave, a later pass in turn
# ---------------------------------------------------------------------------------------------------------
def _tie_rounds(oracle, metric, n, s, far, seed):
    rng = np.random.default_rng(seed)
    dim = 12 if metric == "refcos" else 13
    segs = _ragged(rng, n, dim, 2, 6)
    entry = rng.normal(size=(3, dim))
    if metric == "refcos":
        entry /= math.sqrt(float((entry * entry).sum()))      # cosine_sim divides by SQUARED norms: 1.0 needs norm 1
    places = [s, s + 1, s + 64, s + 1024] + ([s + 4096] if far else [])
    assert places[-1] < n
    for p in places:
        segs[p] = entry.copy()
    target = 1.0 if metric == "refcos" else 0.0
    dist = [target] * 3
    e = Engine(metric=metric, dtype="f64")
    for lowest in range(len(places)):
        ref = _Ref(oracle, segs, dim, metric)
        keys = np.abs(ref.col(entry) - target)
        live = places[lowest:]
        others = np.delete(keys, live)
        assert np.all(keys[live] == keys[live[0]]) and not (others <= keys[live[0]]).any()   # the copies ARE the unique best key
        d = _dict(e, segs, dim)
        idx, _ = _check(e, d, ref, entry, dist)
        assert idx.tolist() == [live[0]] * 3
        d.close()
        segs[places[lowest]] = rng.normal(size=(4, dim)) * 3.0                                # the lowest copy goes
    e.close()


@pytest.mark.parametrize("s", [0, 63, 500])
def test_refcos_ties_by_position(oracle, s):
    _tie_rounds(oracle, "refcos", 2100, s, False, 0xC5C0 + s)


def test_refcos_ties_by_position_far(oracle):
    _tie_rounds(oracle, "refcos", 5000, 63, True, 0xC5C9)


@pytest.mark.parametrize("s", [0, 63, 400])
def test_dtw_ties_by_position(oracle, s):
    _tie_rounds(oracle, "dtw", 1500, s, False, 0xC5D0 + s)


# ---------------------------------------------------------------------------------------------------------
# nothing beats the fold's start
# ---------------------------------------------------------------------------------------------------------
def test_nothing_found_refcos_distance_out_of_reach(oracle):
    rng = np.random.default_rng(0xC5E0)
    segs = _ragged(rng, 1300, 12, 1, 8)
    e = Engine(metric="refcos", dtype="f64")
    d, ref = _dict(e, segs, 12), _Ref(oracle, segs, 12, "refcos")
    start = rng.normal(size=(3, 12))
    idx, val = _check(e, d, ref, start, [5.0] * 6)                 # every key is >= 2.0
    assert idx.tolist() == [0] * 6 and val.tolist() == [2.0] * 6
    dist = [0.2, 5.0, 0.3, 5.0, 5.0, 0.1, 0.0]                     # ... and the chain goes on from entry 0
    idx, val = _check(e, d, ref, start, dist)
    assert [idx[i] for i in (1, 3, 4)] == [0, 0, 0] and [val[i] for i in (1, 3, 4)] == [2.0] * 3
    e.close()


def test_nothing_found_refcos_no_entry_has_a_key(oracle):
    rng = np.random.default_rng(0xC5E1)
    segs = []
    for i in range(1100):
        s = np.zeros((int(rng.integers(1, 5)), 12))
        if i % 3 == 1:
            s[0, int(rng.integers(0, 12))] = np.nan
        elif i % 3 == 2:
            s = np.zeros((0, 12))
        segs.append(s)
    e = Engine(metric="refcos", dtype="f64")
    idx, val = _check(e, _dict(e, segs, 12), _Ref(oracle, segs, 12, "refcos"), rng.normal(size=(2, 12)),
                      [1.0, 0.0, 0.5, 1.0, 1.5])
    assert idx.tolist() == [0] * 5 and val.tolist() == [2.0] * 5
    e.close()


def test_nothing_found_dtw_band_out_of_reach(oracle):
    rng = np.random.default_rng(0xC5E2)
    segs = [rng.normal(size=(int(rng.integers(18, 23)), 13)) for _ in range(1100)]
    start = rng.normal(size=(3, 13))                                # |Fa - Fb| >= 15 > 5 for every entry
    e = Engine(metric="dtw", dtype="f64", band=5)
    ref = _Ref(oracle, segs, 13, "dtw", band=5)
    assert np.isinf(ref.col(start)).all()
    idx, val = _check(e, _dict(e, segs, 13), ref, start, [0.0, 30.0, 45.0, 0.0, 60.0])
    assert idx[0] == 0 and val[0] == math.inf and np.isfinite(val[1:]).all()
    e.close()


@pytest.mark.parametrize("band", [-1, 5])
def test_nothing_found_dtw_empty_segments(oracle, band):
    segs = [np.zeros((0, 13)) for _ in range(1030)]
    e = Engine(metric="dtw", dtype="f64", band=band)
    idx, val = _check(e, _dict(e, segs, 13), _Ref(oracle, segs, 13, "dtw", band=band),
                      np.random.default_rng(1).normal(size=(4, 13)), [0.0, 1.0, 2.0, 0.0])
    assert idx.tolist() == [0] * 4 and val.tolist() == [math.inf] * 4
    e.close()


# ---------------------------------------------------------------------------------------------------------
# mixed dictionaries
# ---------------------------------------------------------------------------------------------------------
def test_refcos_nan_and_zero_norm_entries_among_ordinary_ones(oracle):
    rng = np.random.default_rng(0xC5F0)
    segs = _ragged(rng, 1200, 12, 1, 8)
    for i in range(0, 1200, 7):
        segs[i] = np.zeros((2, 12))
    for i in range(3, 1200, 11):
        segs[i][0, 0] = np.nan
    for i in range(5, 1200, 13):
        segs[i][-1, 3] = np.inf
    segs[1100] = np.zeros((0, 12))
    e = Engine(metric="refcos", dtype="f64")
    ref = _Ref(oracle, segs, 12, "refcos")
    dist = np.concatenate([[1.0], ref.typical(rng, 45)])
    idx, _ = _check(e, _dict(e, segs, 12), ref, rng.normal(size=(5, 12)), dist)
    assert np.unique(idx).size >= 20
    e.close()


@pytest.mark.parametrize("metric", ["refcos", "dtw"])
def test_an_empty_entry_becomes_the_query(oracle, metric):
    """An entry without frames has no key in either metric (NaN similarity, +inf cost), so the only way it becomes the
    current query is as entry 0 after a step that found nothing; every later step then finds nothing either."""
    rng = np.random.default_rng(0xC5F1)
    dim = 12 if metric == "refcos" else 13
    segs = [np.zeros((0, dim))] + _ragged(rng, 70, dim, 1, 9)
    out_of_reach = 5.0 if metric == "refcos" else math.inf          # (|cost - inf| is inf or NaN: never < inf)
    start = 2.0 if metric == "refcos" else math.inf
    dist = [0.7, 0.4, out_of_reach, 0.3, 0.9]
    e = Engine(metric=metric, dtype="f64")
    idx, val = _check(e, _dict(e, segs, dim), _Ref(oracle, segs, dim, metric), rng.normal(size=(4, dim)), dist)
    assert idx[0] != 0 and idx[1] != 0
    assert idx[2:].tolist() == [0, 0, 0] and val[2:].tolist() == [start] * 3
    e.close()


@pytest.mark.parametrize("metric", ["refcos", "dtw"])
def test_a_start_without_frames(oracle, metric):
    rng = np.random.default_rng(0xC5F2)
    dim = 12 if metric == "refcos" else 13
    segs = _ragged(rng, 90, dim, 1, 9)
    e = Engine(metric=metric, dtype="f64")
    d, ref = _dict(e, segs, dim), _Ref(oracle, segs, dim, metric)
    dist = [0.5, 0.8, 0.2, 1.0] if metric == "refcos" else [0.0, 9.0, 20.0, 3.0]
    idx, val = _check(e, d, ref, np.zeros((0, dim)), dist)
    assert idx[0] == 0 and val[0] == (2.0 if metric == "refcos" else math.inf)
    # the same through the C ABI with a NULL start pointer, which start_frames = 0 allows
    dd = np.asarray(dist, dtype=np.float64)
    oi, oc = np.zeros(4, dtype=np.uint32), np.zeros(4)
    rc = nat.lib().ssym_chain(e.ctx, d.ptr, None, 0, dd.ctypes.data, 4, oi.ctypes.data, oc.ctypes.data)
    assert rc == nat.SSYM_OK and np.array_equal(oi, idx) and np.array_equal(oc.view(np.uint64), val.view(np.uint64))
    e.close()


# ---------------------------------------------------------------------------------------------------------
# contexts
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("band,squared", [(0, False), (5, False), (-1, True), (5, True)])
def test_dtw_contexts(oracle, band, squared, dtype):
    rng = np.random.default_rng(0xC600 + 10 * band + squared)
    npd = np.float32 if dtype == "f32" else np.float64
    lo, hi = (3, 5) if band == 0 else (1, 12)          # band 0: only entries of the query's length are in reach
    segs = _ragged(rng, 1100, 13, lo, hi, npd)
    start = rng.normal(size=(4, 13)).astype(npd)
    ref = _Ref(oracle, segs, 13, "dtw", band=band, squared=squared)
    dist = np.concatenate([[0.0], ref.typical(rng, 8)])
    e = Engine(metric="dtw", dtype=dtype, band=band, squared=squared)
    idx, _ = _check(e, _dict(e, segs, 13), ref, start, dist)
    assert np.unique(idx).size >= 3                    # the chain moves
    e.close()


def test_refcos_f32_input(oracle):
    rng = np.random.default_rng(0xC610)
    segs = _ragged(rng, 1100, 12, 1, 8, np.float32)
    segs[40] = np.zeros((2, 12), dtype=np.float32)
    e = Engine(metric="refcos", dtype="f32")
    ref = _Ref(oracle, segs, 12, "refcos")
    dist = np.concatenate([[1.0], ref.typical(rng, 40)])
    idx, _ = _check(e, _dict(e, segs, 12), ref, rng.normal(size=(3, 12)).astype(np.float32), dist)
    assert np.unique(idx).size >= 20
    e.close()


# ---------------------------------------------------------------------------------------------------------
# the cached self-similarity matrix
# ---------------------------------------------------------------------------------------------------------
def test_cache_follows_appends(oracle):
    rng = np.random.default_rng(0xC620)
    segs = _ragged(rng, 700, 12, 1, 8)
    start = rng.normal(size=(4, 12))
    ref = _Ref(oracle, segs, 12, "refcos")
    dist = np.concatenate([[1.0], ref.typical(rng, 30)])
    e = Engine(metric="refcos", dtype="f64")
    d = _dict(e, segs, 12)
    first = _check(e, d, ref, start, dist)
    e.dictionary_append(d, np.zeros(0), np.zeros(1, dtype=np.uint64))        # no segment: nothing changes
    again = e.chain(d, start, dist)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1].view(np.uint64), first[1].view(np.uint64))
    for k in (400, 1):                                                       # two appends, then one chain
        more = _ragged(rng, k, 12, 1, 8)
        f, o = pack_segments(more, 12)
        e.dictionary_append(d, f, o)
        segs = segs + more
    idx, _ = _check(e, d, _Ref(oracle, segs, 12, "refcos"), start, dist)
    assert idx.max() >= 700                                                  # the appended entries take part
    e.close()


@pytest.mark.parametrize("n_a,n_b", [(300, 1300), (1100, 1100)])
def test_two_dictionaries_alternately_on_one_engine(oracle, n_a, n_b):
    rng = np.random.default_rng(0xC630 + n_a)
    sa, sb = _ragged(rng, n_a, 12, 1, 8), _ragged(rng, n_b, 12, 1, 8)
    e = Engine(metric="refcos", dtype="f64")
    da, db = _dict(e, sa, 12), _dict(e, sb, 12)
    ra, rb = _Ref(oracle, sa, 12, "refcos"), _Ref(oracle, sb, 12, "refcos")
    start = rng.normal(size=(4, 12))
    for r in range(3):
        dist = np.concatenate([[1.0], (ra if r % 2 else rb).typical(rng, 20)])
        _check(e, da, ra, start, dist)
        _check(e, db, rb, start, dist)
    e.close()


def test_one_step_does_not_build_the_matrix(oracle):
    """200 000 entries: their self-similarity matrix would be 320 GB, more than the device has, so a one-step chain
    that built it could not succeed.  A later, longer chain on a dictionary that had a one-step chain first must
    still be right."""
    rng = np.random.default_rng(0xC640)
    n = 200_000
    flat = rng.normal(size=n * 12)
    off = np.arange(n + 1, dtype=np.uint64)
    start = rng.normal(size=(1, 12))
    e = Engine(metric="refcos", dtype="f64")
    big = e.dictionary(flat, off, 12)
    idx, val = e.chain(big, start, [0.01])
    col = oracle.refcos_matrix(flat, off, start.reshape(-1), np.array([0, 1], dtype=np.uint64), 12)[:, 0]
    want, found = tail_ref.first_min(col, 0.01, 2.0)
    assert found and idx.tolist() == [want] and val[0] == abs(col[want] - 0.01)
    big.close()
    segs = _ragged(rng, 1100, 12, 1, 8)
    d, ref = _dict(e, segs, 12), _Ref(oracle, segs, 12, "refcos")
    _check(e, d, ref, start, [0.3])
    _check(e, d, ref, start, np.concatenate([[0.3], ref.typical(rng, 30)]))
    e.close()


# ---------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------
def test_every_listed_error_leaves_the_outputs_untouched():
    rng = np.random.default_rng(0xC650)
    e = Engine(metric="refcos", dtype="f64")
    d = _dict(e, _ragged(rng, 20, 12, 1, 5), 12)
    empty = e.dictionary(np.zeros(0), np.zeros(1, dtype=np.uint64), 12)
    L, ctx = nat.lib(), e.ctx
    start = np.ascontiguousarray(rng.normal(size=(2, 12)))
    dist = np.array([1.0, 0.5, 0.2])

    def call(dh=d.ptr, null=(), steps=3, frames=2):
        oi, oc = np.full(3, SENT32, dtype=np.uint32), np.full(3, SENTF)
        ptr = lambda name, arr: None if name in null else arr.ctypes.data
        rc = L.ssym_chain(ctx, dh, ptr("start", start), frames, ptr("dist", dist), steps, ptr("idx", oi), ptr("cost", oc))
        return rc, oi, oc

    def untouched(oi, oc):
        return (oi == SENT32).all() and (oc == SENTF).all()

    for kw, want in [(dict(dh=None), nat.SSYM_E_INVALID), (dict(null=("dist",)), nat.SSYM_E_INVALID),
                     (dict(null=("idx",)), nat.SSYM_E_INVALID), (dict(null=("start",)), nat.SSYM_E_INVALID),
                     (dict(dh=empty.ptr), nat.SSYM_E_EMPTY_DICT)]:
        rc, oi, oc = call(**kw)
        assert rc == want and untouched(oi, oc), kw
        assert L.ssym_last_error(ctx)
    # no steps: nothing to do, whatever else is missing
    rc, oi, oc = call(steps=0, null=("dist", "idx", "cost", "start"))
    assert rc == nat.SSYM_OK and untouched(oi, oc)
    # out_cost may be NULL
    rc, oi, oc = call(null=("cost",))
    want, _ = e.chain(d, start, dist)
    assert rc == nat.SSYM_OK and np.array_equal(oi, want) and (oc == SENTF).all()
    e.close()
