"""ssym_match_topk and per-target distances on every route of the dtw search, against tests/topk_ref.py.

The costs come from the CPU oracle (oracle.dtw_match_all(..., want_matrix=True)), the rows from the numpy restatement:
indices equal, costs within the exact kernel's 1e-12 relative, entry 0 of a row equal to
ssym_match_queries with the same arguments, the all-pairs route (force_exact) equal to the filter route bit for bit.
Every case asserts the route it took from Engine.timings().

Near-ties: the GPU and the oracle may differ in a cost's last place, so every search first asserts on the oracle's
matrix alone (topk_ref.assert_separated) that within a target's first k + 1 keys any two unequal keys are more than
1e-9 relative apart; intended ties are bit-identical duplicates or exact integer costs.  No row is excused.
"""
import ctypes

import numpy as np
import pytest

import topk_ref as ref
from soundsym_amd import Engine, synth
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12
NAN, INF = float("nan"), float("inf")


def _ragged(seed, n, lo, hi, dim):
    st = np.random.default_rng(seed)
    sig = synth.sigma(dim)
    return [(st.normal(size=(int(st.integers(lo, hi + 1)), dim)) * sig).astype(np.float32) for _ in range(n)]


def _edge_distances(rng, mat):
    """Distances among the costs, with NaN, +inf, -inf and a value above every cost at fixed targets."""
    m = mat.shape[1]
    fin = mat[np.isfinite(mat)]
    top = float(fin.max()) if fin.size else 1.0
    d = rng.uniform(0.0, float(np.median(fin)) if fin.size else 1.0, size=m)
    for i, v in enumerate([NAN, INF, -INF, 2.0 * top + 1.0]):
        if m > 4:
            d[(5 * i + 1) % m] = v
    return d


def filter_route(launches=None, more_than=None, some=False):
    """used_filter = 1 and no pruning.  Default: fewer pairs re-scored than there are (candidates, not the matrix);
    more_than: at least that many re-scored (list 1's first capacity: the selection was redone with the reported size);
    some: any number (fewer sources than k: every finite pair is a candidate)."""
    def check(tm):
        assert tm["used_filter"] == 1 and tm["pruned"] == 0, tm
        if launches is not None:
            assert tm["main_launches"] == launches, tm
        if more_than is not None:
            assert tm["n_refined"] > more_than, tm
        elif not some:
            assert 0 < tm["n_refined"] < tm["n_pairs"], tm
    return check


def exact_route(tm):
    assert tm["used_filter"] == 0 and tm["n_refined"] == tm["n_pairs"], tm


class _Case:
    def __init__(self, oracle, e, src, tgt, dim, band=-1, squared=False):
        self.e, self.n, self.m = e, len(src), len(tgt)
        sf, so = pack_segments(src, dim, e.np_dtype)
        tf, to = pack_segments(tgt, dim, e.np_dtype)
        self.d, self.q = e.dictionary(sf, so, dim), e.queries(tf, to, dim)
        _, _, self.mat = oracle.dtw_match_all(sf.astype(np.float64), so, tf.astype(np.float64), to, dim, band=band,
                                              squared=squared, nthreads=oracle.max_threads(), want_matrix=True)

    def check(self, k, dist, route, base=0, exact_too=True):
        e = self.e
        ref.assert_separated(self.mat, k, dist)                     # the inputs' precondition, on the oracle alone
        want_idx, want_cost = ref.rows(self.mat, k, dist, index_base=base, **ref.DTW)
        idx, cost = e.match_topk(self.d, self.q, k, dist, index_base=base)
        tm = e.timings()
        print("dtw n=%d m=%d k=%d dist=%s:" % (self.n, self.m, k, dist is not None), tm)
        route(tm)
        ref.check_rows(idx, cost, want_idx, want_cost, rtol=EXACT_RTOL)
        one, c1 = e.match(self.d, self.q, dist, index_base=base)
        route(e.timings())
        ref.check_first_entry(idx, cost, one, c1)
        first_idx, first_cost = ref.first(self.mat, dist, index_base=base, **ref.DTW)
        assert np.array_equal(one.astype(np.int64), first_idx)
        fin = np.isfinite(first_cost)
        assert np.array_equal(np.isfinite(c1), fin) and np.all(np.abs(c1[fin] - first_cost[fin]) <= EXACT_RTOL * first_cost[fin])
        assert (c1[~fin] == INF).all()
        if exact_too:                                               # all pairs through fold_*_topk: the same bits
            idx2, cost2 = e.match_topk(self.d, self.q, k, dist, index_base=base, force_exact=True)
            exact_route(e.timings())
            assert np.array_equal(idx2, idx) and np.array_equal(cost2, cost, equal_nan=True)
        return idx, cost


@pytest.fixture(scope="module")
def dtw():
    e = Engine(metric="dtw", dtype="f32")
    yield e
    e.close()


@pytest.fixture(scope="module")
def grids(oracle, dtw):
    """A planted grid (every target has a near source) and an unplanted one, each with a bit-identical duplicate."""
    g = synth.make_grid(256, 64, 24, 13, 0x5EED0D01)
    ps, pt = [x for x in g.sources], [x for x in g.targets]
    ps[50] = ps[3].copy()
    pt[0] = ps[3].copy()
    us = [x for x in synth.make_grid(200, 1, 24, 13, 0x5EED0D02).sources]
    ut = [x for x in synth.make_grid(72, 1, 24, 13, 0x5EED0D03).sources]
    us[150] = us[9].copy()
    us[151] = us[9].copy()
    ut[2] = us[9].copy()
    return {"planted": _Case(oracle, dtw, ps, pt, 13), "unplanted": _Case(oracle, dtw, us, ut, 13)}


@pytest.mark.parametrize("which", ["planted", "unplanted"])
@pytest.mark.parametrize("k", [1, 2, 16, 17, 32, 64])
def test_k_sweep_through_the_filter(grids, which, k):
    c = grids[which]
    rng = np.random.default_rng(0xD700 + k)
    idx, cost = c.check(k, None, filter_route())
    if which == "planted":
        assert idx[0, :min(k, 2)].tolist() == [3, 50][:k] and cost[0, 0] == 0.0
    else:
        assert idx[2, :min(k, 3)].tolist() == [9, 150, 151][:k]
    c.check(k, _edge_distances(rng, c.mat), filter_route())


@pytest.fixture(scope="module")
def ragged(oracle, dtw):
    """600 x 300 segments of 5...40 frames (all three single-pass length classes of the filter's sp kernel), with two
    one-frame sources whose costs to the one-frame target 7 are exactly 3 and 1."""
    src, tgt = _ragged(0x5EED0D10, 600, 5, 40, 13), _ragged(0x5EED0D11, 300, 5, 40, 13)
    src[400] = src[12].copy()
    tgt[0] = src[12].copy()
    unit = np.zeros((1, 13), dtype=np.float32)
    unit[0, 0] = 1.0
    src[10], src[20], tgt[7] = 3.0 * unit, 1.0 * unit, 0.0 * unit
    c = _Case(oracle, dtw, src, tgt, 13)
    assert c.mat[10, 7] == 3.0 and c.mat[20, 7] == 1.0
    return c


def test_ragged_sets_across_the_length_classes(ragged):
    c = ragged
    rng = np.random.default_rng(0xD710)
    idx, _ = c.check(5, None, filter_route(launches=3))          # one filter launch per length class
    assert idx[0, :2].tolist() == [12, 400]
    dist = _edge_distances(rng, c.mat)
    dist[7] = 2.0                                   # |3 - 2| = |1 - 2| = 1 exactly: the lower index (cost 3) first
    idx, cost = c.check(5, dist, filter_route(launches=3))
    assert idx[7, :2].tolist() == [10, 20] and cost[7, :2].tolist() == [3.0, 1.0]
    for t in (1, 6, 11):                            # NaN, +inf, -inf: nothing enters
        assert (idx[t] == nat.NO_MATCH).all() and np.isnan(cost[t]).all()
    one, c1 = c.e.match(c.d, c.q, dist, index_base=9)
    assert one[1] == 9 and c1[1] == INF             # k = 1 under a NaN distance: index 0 + base, +inf
    top = np.nanmax(np.where(np.isfinite(c.mat[:, 16]), c.mat[:, 16], np.nan))
    assert cost[16, 0] == pytest.approx(top, rel=EXACT_RTOL)      # a distance above every cost: the largest cost first


@pytest.mark.parametrize("k", [1, 3])
def test_multi_pair_tasks_forced_on_a_power_of_two_dictionary(oracle, dtw, monkeypatch, k):
    """1024 sources of at most 16 frames, dim 13: with SSYM_SP_MULTIPAIR=2 the filter's last task reads the lengths of
    pairs beyond the set's end (masked; the length array keeps room for them)."""
    src, tgt = _ragged(0x5EED0D20, 1024, 1, 16, 13), _ragged(0x5EED0D21, 70, 1, 40, 13)
    src[1023] = src[5].copy()
    tgt[0] = src[5].copy()
    c = _Case(oracle, dtw, src, tgt, 13)
    plain = c.check(k, None, filter_route())
    monkeypatch.setenv("SSYM_SP_MULTIPAIR", "2")
    forced = c.check(k, None, filter_route(), exact_too=False)
    assert np.array_equal(plain[0], forced[0]) and np.array_equal(plain[1], forced[1], equal_nan=True)
    assert forced[0][0, :min(k, 2)].tolist() == [5, 1023][:k]
    rng = np.random.default_rng(0xD720)
    c.check(k, _edge_distances(rng, c.mat), filter_route(), exact_too=False)


@pytest.mark.parametrize("dim,r,m", [(13, 0, 255), (13, 3, 257), (13, 32, 256), (40, 0, 257), (40, 3, 256), (40, 32, 255)])
def test_banded(oracle, dim, r, m):
    g = synth.make_grid(128, m, 40, dim, 0x5EED0D30 + dim + r)
    src, tgt = [x for x in g.sources], [x for x in g.targets]
    src[77] = src[6].copy()
    tgt[m - 1] = src[6].copy()
    e = Engine(metric="dtw", dtype="f32", band=r)
    c = _Case(oracle, e, src, tgt, dim, band=r)
    idx, _ = c.check(4, None, filter_route())
    assert idx[m - 1, :2].tolist() == [6, 77]
    c.check(4, _edge_distances(np.random.default_rng(r), c.mat), filter_route())
    e.close()


def test_a_band_that_cuts_every_path_of_some_pairs(oracle):
    """r = 3 on ragged lengths: a pair whose lengths differ by more than 3 has no path, cost +inf, and never enters."""
    src, tgt = _ragged(0x5EED0D40, 150, 8, 24, 13), _ragged(0x5EED0D41, 90, 8, 24, 13)
    src[100] = src[4].copy()
    tgt[0] = src[4].copy()
    tgt[1] = _ragged(1, 1, 40, 40, 13)[0]           # no source within 3 frames of 40: an empty row
    e = Engine(metric="dtw", dtype="f32", band=3)
    c = _Case(oracle, e, src, tgt, 13, band=3)
    assert np.isinf(c.mat).mean() > 0.3 and np.isinf(c.mat[:, 1]).all()
    idx, cost = c.check(4, None, filter_route())
    assert (idx[1] == nat.NO_MATCH).all() and idx[0, :2].tolist() == [4, 100]
    short = (np.isfinite(c.mat).sum(axis=0) < 4)
    assert short.sum() >= 1 and (idx[short, 3] == nat.NO_MATCH).all()
    c.check(4, _edge_distances(np.random.default_rng(3), c.mat), filter_route())
    e.close()


@pytest.mark.parametrize("dtype,squared", [("f32", True), ("f64", False), ("f64", True)])
def test_squared_cost_and_f64_context(oracle, dtype, squared):
    g = synth.make_grid(160, 70, 24, 13, 0x5EED0D50 + squared)
    src, tgt = [x for x in g.sources], [x for x in g.targets]
    src[90] = src[8].copy()
    tgt[3] = src[8].copy()
    e = Engine(metric="dtw", dtype=dtype, squared=squared)
    c = _Case(oracle, e, src, tgt, 13, squared=squared)
    idx, _ = c.check(4, None, filter_route())
    assert idx[3, :2].tolist() == [8, 90]
    c.check(4, _edge_distances(np.random.default_rng(5), c.mat), filter_route())
    e.close()


@pytest.mark.parametrize("dim", [45, 64])
@pytest.mark.parametrize("k", [1, 3])
def test_wide_frames_with_per_target_distances(oracle, dtw, dim, k):
    """Frames wider than the filter's 42 values: the filter's costs are lower bounds only (launch_dtw_bounds_partial);
    with per-target distances and k > 1 the cascade still answers, and re-scores fewer pairs than there are."""
    g = synth.make_grid(96, 80, 40, dim, 0x5EED0D60 + dim)
    src, tgt = [x for x in g.sources], [x for x in g.targets]
    src[17] = src[5].copy()
    tgt[3] = src[5].copy()
    tgt[4] = np.zeros((0, dim), dtype=np.float32)
    c = _Case(oracle, dtw, src, tgt, dim)
    idx, _ = c.check(k, None, filter_route())
    assert idx[3, :min(k, 2)].tolist() == [5, 17][:k]
    assert (idx[4] == nat.NO_MATCH).all() if k > 1 else idx[4, 0] == 0     # the empty target
    c.check(k, _edge_distances(np.random.default_rng(dim), c.mat), filter_route())


@pytest.mark.parametrize("frames", [200, 300])
def test_sources_of_several_row_block_passes(oracle, dtw, frames):
    g = synth.make_grid(64, 24, frames, 13, 0x5EED0D70 + frames)
    src, tgt = [x for x in g.sources], [x for x in g.targets]
    src[40] = src[2].copy()
    tgt[5] = src[2].copy()
    c = _Case(oracle, dtw, src, tgt, 13)
    idx, _ = c.check(3, None, filter_route())
    assert idx[5, :2].tolist() == [2, 40]
    c.check(3, _edge_distances(np.random.default_rng(frames), c.mat), filter_route())


def test_list_1_overflow_is_redone_and_gives_the_same_rows(oracle, dtw):
    """Every source identical: list 1 wants all 600 x 200 pairs, more than (256 + 16 (k - 1)) per target; the selection
    is redone with the reported size and the rows are the first k indices in order."""
    n, m, f, k = 600, 200, 8, 4
    one = synth.make_grid(1, 1, f, 13, 0x5EED0395).sources[0]
    src = [one.copy() for _ in range(n)]
    tgt = [x for x in synth.make_grid(m, 1, f, 13, 0x5EED0396).sources]
    c = _Case(oracle, dtw, src, tgt, 13)
    cap0 = max((256 + 16 * (k - 1)) * m, 65536)                   # list 1's first capacity (match.hip, dtw_filter_back)
    idx, _ = c.check(k, None, filter_route(more_than=cap0))
    assert np.array_equal(idx, np.tile(np.arange(k, dtype=np.uint32), (m, 1)))
    # (with distances the three targets whose distance is NaN or infinite list nothing: 197 x 600 pairs, still an overflow)
    c.check(k, _edge_distances(np.random.default_rng(8), c.mat), filter_route(more_than=cap0))


def test_non_finite_features_decline_the_filter(oracle, dtw):
    src, tgt = _ragged(0x5EED0D80, 80, 5, 20, 13), _ragged(0x5EED0D81, 70, 5, 20, 13)
    for i in range(80):
        if i not in (2, 30, 31, 79):
            src[i][i % src[i].shape[0], i % 13] = NAN if i % 2 else INF
    src[31] = src[30].copy()
    tgt[0] = src[30].copy()
    c = _Case(oracle, dtw, src, tgt, 13)
    assert (np.isfinite(c.mat).sum(axis=0) == 4).all()
    idx, cost = c.check(6, None, exact_route, exact_too=False)
    assert (idx[:, 4:] == nat.NO_MATCH).all() and (idx[:, :4] != nat.NO_MATCH).all() and idx[0, :2].tolist() == [30, 31]
    c.check(6, _edge_distances(np.random.default_rng(9), c.mat), exact_route, exact_too=False)
    tgt[5][0, 0] = NAN                               # a NaN target: its row is empty
    c = _Case(oracle, dtw, src[:4] + [src[30]], tgt, 13)
    idx, cost = c.check(2, None, exact_route, exact_too=False)
    assert (idx[5] == nat.NO_MATCH).all()


@pytest.mark.parametrize("n,m", [(63, 70), (64, 63), (65, 64), (129, 65), (1, 66), (5, 40)])
def test_sizes_either_side_of_the_selection_chunks(oracle, dtw, n, m):
    """kSelChunk = 64 sources, kSelTgt = 64 targets; one source; fewer sources than k."""
    src, tgt = _ragged(0x5EED0D90 + n, n, 5, 30, 13), _ragged(0x5EED0DA0 + m, m, 5, 30, 13)
    src[n - 1] = src[0].copy()
    tgt[m - 1] = src[0].copy()
    c = _Case(oracle, dtw, src, tgt, 13)
    k = 8
    route = filter_route(some=True) if n <= k else filter_route()
    idx, _ = c.check(k, None, route)
    assert (idx[:, min(n, k):] == nat.NO_MATCH).all() and (idx[:, :min(n, k)] != nat.NO_MATCH).all()
    assert idx[m - 1, 0] == 0 and (n == 1 or idx[m - 1, 1] == n - 1)
    c.check(k, _edge_distances(np.random.default_rng(n), c.mat), route)


@pytest.mark.parametrize("base", [1000, 0xFFFFFF00])
def test_index_base_and_device_outputs(oracle, dtw, base):
    """Five finite sources, k = 8: SSYM_NO_MATCH stays unshifted, the rest carry the base -- on the filter route, on the
    all-pairs route, and with SSYM_OUT_DEVICE."""
    import torch
    src, tgt = _ragged(0x5EED0DB0, 200, 5, 20, 13), _ragged(0x5EED0DB1, 90, 5, 20, 13)
    keep = (3, 50, 51, 128, 199)
    src = [s if i in keep else np.zeros((0, 13), dtype=np.float32) for i, s in enumerate(src)]
    c = _Case(oracle, dtw, src, tgt, 13)
    k = 8
    rng = np.random.default_rng(base & 0xFFFF)
    for dist in (None, _edge_distances(rng, c.mat)):
        idx, cost = c.check(k, dist, filter_route(), base)
        if dist is None:
            assert (idx[:, 5:] == nat.NO_MATCH).all()
            assert set(np.unique(idx[:, :5]).tolist()) == {(i + base) & 0xFFFFFFFF for i in keep}
        for flags, route in ((nat.OUT_DEVICE, filter_route()), (nat.OUT_DEVICE | nat.DTW_FORCE_EXACT, exact_route)):
            oi = torch.full((c.m, k), 12345, dtype=torch.int32, device="cuda")
            oc = torch.full((c.m, k), -7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()             # (the fills ran on torch's stream, the library writes on its own)
            dbuf = None if dist is None else np.ascontiguousarray(dist)
            nat.check(nat.lib().ssym_match_topk(dtw.ctx, c.d.ptr, c.q.ptr,
                                                ctypes.c_void_p(dbuf.ctypes.data) if dbuf is not None else None, k, base,
                                                ctypes.c_void_p(oi.data_ptr()), ctypes.c_void_p(oc.data_ptr()), flags),
                      dtw.ctx)
            route(dtw.timings())
            dtw.synchronize()
            assert np.array_equal(oi.cpu().numpy().view(np.uint32), idx)
            assert np.array_equal(oc.cpu().numpy(), cost, equal_nan=True)
