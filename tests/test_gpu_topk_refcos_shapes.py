"""ssym_match_topk and per-target distances on every route of the refcos search, against tests/topk_ref.py.

The similarities come from the CPU oracle (oracle.refcos_matrix), the rows from the numpy restatement; indices and keys
are compared bit for bit, entry 0 of a row against ssym_match_queries with the same arguments, and every case asserts
the route it took from Engine.timings(): refcos_filter 2 = integer filter, 1 = f64 filter, 0 = the tile kernel on every
pair (with fold_final_topk_kernel for k > 1); used_filter 1 = a filter's candidates answered.  k = 1 through
ssym_match_topk is ssym_match_queries: a target nothing enters for has index 0 + base and 2.0 (topk_ref.rows).
"""
import ctypes

import numpy as np
import pytest

import topk_ref as ref
from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
Q8, F64, TILE = 2, 1, 0


def _sets(seed, n, m, fmin, fmax, dim, scale=0.05):
    """cosine_sim is dot / (|a|^2 |b|^2): at scale 0.05 short segments have similarities far outside the fold's start
    (rows with missing entries), at scale 0.3 every pair enters."""
    rng = np.random.default_rng(seed)
    src = [rng.normal(size=(int(rng.integers(fmin, fmax + 1)), dim)) * scale for _ in range(n)]
    tgt = [rng.normal(size=(int(rng.integers(fmin, fmax + 1)), dim)) * scale for _ in range(m)]
    return src, tgt, rng


def _edge_distances(rng, m):
    """Distances in range, with the edge values at fixed targets."""
    d = rng.uniform(-0.2, 1.4, size=m)
    for i, v in enumerate([NAN, INF, -INF, 1e301]):
        d[(7 * i + 2) % m] = v
    return d


class _Case:
    """One pair of sets on one engine: the oracle's similarities once, any number of (k, distance, base) searches."""

    def __init__(self, oracle, e, src, tgt, dim):
        self.e, self.m = e, len(tgt)
        sf, so = pack_segments(src, dim, e.np_dtype)
        tf, to = pack_segments(tgt, dim, e.np_dtype)
        self.d, self.q = e.dictionary(sf, so, dim), e.queries(tf, to, dim)
        self.sims = oracle.refcos_matrix(sf.astype(np.float64), so, tf.astype(np.float64), to, dim)

    def check(self, k, dist, route, base=0, used=None, one_route=None, every_pair=False):
        """route: of ssym_match_topk(k); one_route: of ssym_match_queries on the same sets where it differs (the top-k
        list is k times as long, so a set of ties that overflows the plain search's list need not overflow it);
        every_pair: the filter listed every pair as a candidate."""
        e = self.e
        idx, key = e.match_topk(self.d, self.q, k, dist, index_base=base)
        tm = e.timings()
        print("refcos k=%d base=%#x dist=%s:" % (k, base, dist is not None), tm)
        assert tm["refcos_filter"] == route, tm
        assert tm["used_filter"] == (used if used is not None else int(route != TILE)), tm
        if route != TILE:
            assert 0 < tm["n_refined"] <= tm["n_pairs"], tm         # (fewer sources than k: every pair is a candidate)
            assert (tm["n_refined"] == tm["n_pairs"]) == every_pair or k == 1 or self.sims.shape[0] <= k, tm
        want_idx, want_key = ref.rows(self.sims, k, dist, index_base=base, **ref.REFCOS)
        ref.check_rows(idx, key, want_idx, want_key)
        one, val = e.match(self.d, self.q, dist, index_base=base)
        assert e.timings()["refcos_filter"] == (route if one_route is None else one_route), e.timings()
        ref.check_first_entry(idx, key, one, val)
        first_idx, first_val = ref.first(self.sims, dist, index_base=base, **ref.REFCOS)
        assert np.array_equal(one.astype(np.int64), first_idx) and np.array_equal(val, first_val)
        return idx, key


@pytest.fixture(scope="module")
def engine():
    e = Engine(metric="refcos", dtype="f64")
    yield e
    e.close()


@pytest.fixture(scope="module")
def sweep(oracle, engine):
    """420 x 200 ragged segments (84 000 pairs: the filters' side of the 65 536-pair limit) with everything a row can
    hold: a three-way tie, 100 bit-identical sources, a zero-norm and an empty source, an empty and an all-zero target,
    and two one-frame sources whose similarities to target 10 are exactly 0.5 and 0.25."""
    dim = 12
    src, tgt, rng = _sets(0x5EED7C01, 420, 200, 2, 30, dim)
    tgt[0] = src[7].copy()
    src[11] = src[7].copy()
    src[300] = src[7].copy()
    for i in range(100, 200):
        src[i] = src[100].copy()
    tgt[1] = src[100].copy()
    src[5] = np.zeros_like(src[5])
    src[9] = np.zeros((0, dim))
    tgt[3] = np.zeros((0, dim))
    tgt[4] = np.zeros((4, dim))
    unit = np.zeros((1, dim))
    unit[0, 0] = 1.0
    tgt[10] = unit.copy()                       # sim(x e0, e0) = x / x^2 = 1 / x
    src[250], src[40] = 2.0 * unit, 4.0 * unit
    c = _Case(oracle, engine, src, tgt, dim)
    assert c.sims[250, 10] == 0.5 and c.sims[40, 10] == 0.25
    dist = _edge_distances(rng, len(tgt))       # (targets 2, 9, 16, 23: NaN, +inf, -inf, 1e301)
    dist[10] = 0.375                            # 0.5 - d = d - 0.25 = 0.125 exactly: index 40 before index 250
    dist[0] = c.sims[7, 0]                      # key 0 for the three copies
    dist[1] = c.sims[100, 1]                    # key 0 for the hundred copies
    return c, dist


@pytest.mark.parametrize("knob,route", [("1", Q8), ("0", F64)])
@pytest.mark.parametrize("k", [1, 2, 7, 8, 9, 33, 63, 64])
def test_k_sweep_on_the_integer_filter_and_on_the_f64_filter(sweep, monkeypatch, k, knob, route):
    c, dist = sweep
    monkeypatch.setenv("SSYM_REFCOS_Q8", knob)
    idx, key = c.check(k, None, route)
    none = nat.NO_MATCH if k > 1 else 0                                            # (k = 1: index 0 and the fold's start)
    assert (idx[3] == none).all() and (idx[4] == none).all()                       # empty / all-zero target
    idx, key = c.check(k, dist, route)
    assert idx[0, :min(k, 3)].tolist() == [7, 11, 300][:k]                         # the three-way tie, lowest index first
    assert np.array_equal(idx[1], np.arange(100, 100 + k))                         # 100 duplicates: the lowest k, in order
    for t in (2, 9, 16, 23):                                                       # NaN, +inf, -inf, 1e301: nothing enters
        assert (idx[t] == none).all() and (np.isnan(key[t]).all() if k > 1 else key[t, 0] == 2.0)
    row = idx[10].tolist()
    if 250 in row:                                                                 # equal keys from either side: index order
        r = row.index(250)
        assert r > 0 and row[r - 1] == 40 and key[10, r - 1] == key[10, r] == 0.125
    assert k < 64 or 250 in row


def test_nan_distance_with_k_1_is_index_0_and_the_folds_start(sweep, monkeypatch):
    c, dist = sweep
    for knob, route in (("1", Q8), ("0", F64)):
        monkeypatch.setenv("SSYM_REFCOS_Q8", knob)
        one, val = c.e.match(c.d, c.q, dist, index_base=5)
        assert c.e.timings()["refcos_filter"] == route
        assert one[2] == 5 and val[2] == 2.0 and one[16] == 5 and val[16] == 2.0


@pytest.mark.parametrize("k", [1, 8])
def test_values_the_integer_records_cannot_hold_take_the_f64_filter(oracle, engine, k):
    dim = 12
    src, tgt, rng = _sets(0x5EED7C02, 300, 260, 2, 20, dim)
    src[17][1, 3] = INF
    src[33][0, 0] = NAN
    src[60] = src[60] * 1e150 / 0.05
    src[61] = src[61] * 1e-150 / 0.05
    tgt[8] = tgt[8] * 1e-150 / 0.05
    tgt[12] = src[61].copy()
    src[90] = src[61].copy()                                    # a tie among the tiny ones
    c = _Case(oracle, engine, src, tgt, dim)
    c.check(k, None, F64)
    c.check(k, _edge_distances(rng, len(tgt)), F64)


@pytest.mark.parametrize("n,m", [(63, 1041), (64, 1024), (65, 1009), (127, 517), (128, 512), (129, 509), (257, 256),
                                 (600, 127), (600, 128), (600, 129)])
def test_sources_and_targets_either_side_of_a_tile(oracle, engine, n, m):
    src, tgt, rng = _sets(0x5EED7C10 + n + m, n, m, 1, 12, 12, 0.3)
    src[n - 1] = src[0].copy()                                  # a tie across the whole range of rows
    tgt[m - 1] = src[0].copy()
    c = _Case(oracle, engine, src, tgt, 12)
    assert n * m >= 65536
    c.check(7, None, Q8)
    c.check(7, _edge_distances(rng, m), Q8)


def test_fewer_sources_than_k(oracle, engine):
    src, tgt, rng = _sets(0x5EED7C20, 5, 13108, 1, 6, 12, 0.3)
    c = _Case(oracle, engine, src, tgt, 12)
    idx, _ = c.check(8, None, Q8)
    assert (idx[:, 5:] == nat.NO_MATCH).all()
    src, tgt, rng = _sets(0x5EED7C21, 1, 65536, 1, 4, 12, 0.3)
    c = _Case(oracle, engine, src, tgt, 12)
    idx, _ = c.check(3, None, Q8)
    assert (idx[:, 1:] == nat.NO_MATCH).all() and np.isin(idx[:, 0], [0, nat.NO_MATCH]).all() and (idx[:, 0] == 0).mean() > 0.9


@pytest.mark.parametrize("base", [0, 1000, 0xFFFFFF00])
def test_fewer_sources_with_a_norm_than_k_and_index_base(oracle, engine, base):
    """Five of 200 sources have a nonzero norm: rows of k = 8 hold five entries, shifted by the base, and three
    SSYM_NO_MATCH, not shifted -- through a filter and through the tile kernel."""
    src, tgt, rng = _sets(0x5EED7C22, 200, 330, 2, 10, 12, 0.3)
    keep = (3, 50, 51, 128, 199)
    src = [s if i in keep else np.zeros_like(s) for i, s in enumerate(src)]
    c = _Case(oracle, engine, src, tgt, 12)
    idx, _ = c.check(8, None, Q8, base)
    assert (idx[:, 5:] == nat.NO_MATCH).all() and (idx[:, :5] != nat.NO_MATCH).all()
    assert set(np.unique(idx[:, :5]).tolist()) == {(i + base) & 0xFFFFFFFF for i in keep}
    c.check(8, _edge_distances(rng, 330), Q8, base)
    small = _Case(oracle, engine, src, tgt[:100], 12)             # 20 000 pairs: the tile kernel
    idx, _ = small.check(8, None, TILE, base)
    assert (idx[:, 5:] == nat.NO_MATCH).all() and (idx[:, :5] != nat.NO_MATCH).all()
    small.check(8, _edge_distances(rng, 100), TILE, base)


def _identical(seed, n, m, jitter):
    dim, f = 12, 6
    rng = np.random.default_rng(seed)
    one = rng.standard_normal((f, dim)) * 0.1
    src = [one * (1.0 + jitter * rng.standard_normal((f, dim))) if jitter else one.copy() for _ in range(n)]
    tgt = [rng.standard_normal((f, dim)) * 0.1 for _ in range(m)]
    return src, tgt, rng


def test_every_source_identical_at_2200_x_600(oracle, engine):
    """Every pair ties.  The plain search's list (2^20 entries) overflows on both filters and the tile kernel answers;
    the top-k list is min(N M, k 2^20) entries, which for k >= 2 is all 1 320 000 pairs here: the integer filter lists
    every pair, the exact keys and the rounds' (key, index) order give the first k indices."""
    src, tgt, rng = _identical(3, 2200, 600, 0.0)
    c = _Case(oracle, engine, src, tgt, 12)
    idx, _ = c.check(64, None, Q8, one_route=TILE, every_pair=True)
    assert np.array_equal(idx, np.tile(np.arange(64, dtype=np.uint32), (600, 1)))
    c.check(64, _edge_distances(rng, 600), Q8, one_route=TILE)
    c.check(1, None, TILE)


def test_sources_1e_9_apart_at_2200_x_600(oracle, engine):
    """23 bits of fixed point cannot tell the sources apart: the plain search's integer list overflows and the f64
    filter answers; the top-k list holds every pair and the integer filter answers."""
    src, tgt, rng = _identical(31, 2200, 600, 1e-9)
    tgt[5] = src[1234].copy()
    c = _Case(oracle, engine, src, tgt, 12)
    c.check(8, None, Q8, one_route=F64, every_pair=True)
    c.check(8, _edge_distances(rng, 600), Q8, one_route=F64)
    c.check(1, None, F64)


@pytest.mark.parametrize("jitter,route", [(0.0, TILE), (1e-9, F64)])
def test_topk_list_overflow_takes_the_next_filter_and_then_the_tile_kernel(oracle, engine, jitter, route):
    """k = 2 on 2200 x 1000 tied pairs: more than the 2 x 2^20 entries of the top-k list (about 50 MB, the ordinary
    overflow).  Identical sources overflow the f64 filter's list as well and the tile kernel answers with
    fold_final_topk_kernel; sources 1e-9 apart stop at the f64 filter."""
    src, tgt, rng = _identical(37, 2200, 1000, jitter)
    tgt[5] = src[1234].copy()
    c = _Case(oracle, engine, src, tgt, 12)
    assert 2200 * 1000 > 2 * (1 << 20)
    idx, _ = c.check(2, None, route)
    if jitter == 0.0:
        assert np.array_equal(idx, np.tile(np.arange(2, dtype=np.uint32), (1000, 1)))
    c.check(2, _edge_distances(rng, 1000), route)


@pytest.mark.parametrize("n", [129, 257])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_below_65536_pairs_the_tile_kernel_folds_the_rows(oracle, engine, n, k):
    """N is not a multiple of the fold's 128-source chunks: the last chunk is short."""
    m = 150
    src, tgt, rng = _sets(0x5EED7C30 + n, n, m, 1, 12, 12, 0.3)
    src[n - 1] = src[2].copy()
    src[128] = src[2].copy()                                    # a tie across chunks
    tgt[0] = src[2].copy()
    tgt[6] = np.zeros((0, 12))
    c = _Case(oracle, engine, src, tgt, 12)
    assert n * m < 65536
    c.check(k, None, TILE)
    dist = _edge_distances(rng, m)
    dist[0] = c.sims[2, 0]                                      # key 0 for the copies
    idx, _ = c.check(k, dist, TILE)
    copies = sorted({2, 128, n - 1})[:k]
    assert idx[0, :len(copies)].tolist() == copies


def test_f32_context(oracle):
    e = Engine(metric="refcos", dtype="f32")
    src, tgt, rng = _sets(0x5EED7C40, 300, 260, 2, 20, 12, 0.3)
    src[200] = src[4].copy()
    tgt[0] = src[4].copy()
    c = _Case(oracle, e, src, tgt, 12)
    c.check(8, None, Q8)
    c.check(8, _edge_distances(rng, 260), Q8)
    e.close()


def test_device_outputs_equal_host_outputs(sweep, monkeypatch):
    """SSYM_OUT_DEVICE: the rows land in torch tensors and are the host rows, on both filters and on the tile kernel."""
    import torch
    c, dist = sweep
    e = c.e
    dbuf = np.ascontiguousarray(dist)

    def on_device(d, q, m, k, base):
        oi = torch.full((m, k), 12345, dtype=torch.int32, device="cuda")
        oc = torch.full((m, k), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()             # (the fills ran on torch's stream, the library writes on its own)
        nat.check(nat.lib().ssym_match_topk(e.ctx, d.ptr, q.ptr, ctypes.c_void_p(dbuf.ctypes.data), k, base,
                                            ctypes.c_void_p(oi.data_ptr()), ctypes.c_void_p(oc.data_ptr()),
                                            nat.OUT_DEVICE), e.ctx)
        tm = e.timings()
        e.synchronize()
        return oi.cpu().numpy().view(np.uint32), oc.cpu().numpy(), tm

    for knob, route in (("1", Q8), ("0", F64)):
        monkeypatch.setenv("SSYM_REFCOS_Q8", knob)
        for k in (1, 9):
            idx, key = e.match_topk(c.d, c.q, k, dist, index_base=1000)
            di, dc, tm = on_device(c.d, c.q, c.m, k, 1000)
            assert tm["refcos_filter"] == route and tm["used_filter"] == 1, tm
            assert np.array_equal(di, idx) and np.array_equal(dc, key, equal_nan=True)
            want_idx, want_key = ref.rows(c.sims, k, dist, index_base=1000, **ref.REFCOS)
            ref.check_rows(di, dc, want_idx, want_key)


def test_no_targets(engine):
    d = engine.dictionary(np.ones(24), [0, 1, 2], 12)
    q = engine.queries(np.zeros(0), [0], 12)
    idx, key = engine.match_topk(d, q, 4)
    assert idx.shape == (0, 4) and key.shape == (0, 4) and engine.timings()["n_pairs"] == 0
