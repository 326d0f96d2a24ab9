"""tests/topk_ref.py held against the C oracle's sort-based top-k and first-minimum searches, and against rows worked
out by hand.  No GPU."""
import numpy as np
import pytest

import topk_ref as ref

NAN, INF = float("nan"), float("inf")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# value column (one target), distance, k, fold start, report -> the row, worked by hand from the rules in topk_ref.py
HAND = [
    # plain order by |v - 1|
    ([0.9, 0.5, 1.0, 0.7], None, 1.0, 3, 2.0, "key", [2, 0, 3], [0.0, 1.0 - 0.9, 1.0 - 0.7]),
    # a tie: the lower index first, at every rank
    ([0.5, 0.25, 0.5, 0.5], None, 1.0, 3, 2.0, "key", [0, 2, 3], [0.5, 0.5, 0.5]),
    # NaN values never enter; k above what enters: -1 / NaN after it
    ([NAN, 0.5, NAN], None, 1.0, 3, 2.0, "key", [1, -1, -1], [0.5, NAN, NAN]),
    # a key of exactly the fold start does not enter (strict <): v = -1 has key 2.0
    ([-1.0, 0.0], None, 1.0, 2, 2.0, "key", [1, -1], [1.0, NAN]),
    # a distance between two values at equal distance from both (exact binary fractions): the index decides
    ([0.75, 0.25, 0.5], 0.5, 1.0, 3, 2.0, "key", [2, 0, 1], [0.0, 0.25, 0.25]),
    # NaN distance: every key NaN, the row is empty
    ([0.1, 0.2], NAN, 1.0, 2, 2.0, "key", [-1, -1], [NAN, NAN]),
    # +inf distance: every key +inf, none below 2.0
    ([0.1, 0.2], INF, 1.0, 1, 2.0, "key", [-1], [NAN]),
    # a distance of 1e301: keys 1e301, none below 2.0
    ([0.1, 0.2], 1e301, 1.0, 2, 2.0, "key", [-1, -1], [NAN, NAN]),
    # dtw: the cost is reported, not the key; +inf costs never enter
    ([3.0, INF, 1.0, 2.0], None, 0.0, 4, INF, "value", [2, 3, 0, -1], [1.0, 2.0, 3.0, NAN]),
    # dtw with a distance between two exact costs: keys 1, 1, 3 -> index order, costs reported
    ([5.0, 1.0, 3.0], 4.0, 0.0, 3, INF, "value", [0, 2, 1], [5.0, 3.0, 1.0]),
    # dtw, -inf distance: every key +inf, nothing enters
    ([1.0, 2.0], -INF, 0.0, 2, INF, "value", [-1, -1], [NAN, NAN]),
    # dtw, a distance above every cost: the largest cost first
    ([1.0, 2.0, 4.0], 10.0, 0.0, 2, INF, "value", [2, 1], [4.0, 2.0]),
    # k = 1 is the head of the same order
    ([0.5, 0.25, 0.5], 0.5, 1.0, 1, 2.0, "key", [0], [0.0]),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_worked_rows(case):
    col, dist, default, k, start, report, want_idx, want_val = HAND[case]
    mat = np.array(col, dtype=np.float64)[:, None]
    d = None if dist is None else np.array([dist])
    idx, val = ref.topk(mat, k, d, default, start, 0, report)
    assert idx[0].tolist() == want_idx
    assert _same(val[0], np.array(want_val))
    # with a base: real entries shifted, missing ones not
    idx2, val2 = ref.topk(mat, k, d, default, start, 1000, report)
    assert idx2[0].tolist() == [i + 1000 if i >= 0 else -1 for i in want_idx] and _same(val2, val)
    # the k = 1 form: the row's head, or index 0 + base and the fold's start
    i1, v1 = ref.first(mat, d, default, start, 7, report)
    if want_idx[0] >= 0:
        assert i1[0] == want_idx[0] + 7 and v1[0] == want_val[0]
    else:
        assert i1[0] == 7 and v1[0] == start


def test_index_base_wraps_like_uint32_and_leaves_missing_entries():
    mat = np.array([[0.5], [NAN], [0.75]])
    idx, _ = ref.topk(mat, 3, index_base=0xFFFFFF00)
    assert idx[0].tolist() == [0xFFFFFF02, 0xFFFFFF00, -1]


def _edge_matrix(rng, n, m, lo, hi):
    mat = rng.uniform(lo, hi, size=(n, m))
    mat[rng.random((n, m)) < 0.08] = np.nan
    mat[rng.random((n, m)) < 0.05] = np.inf
    mat[rng.random((n, m)) < 0.03] = -np.inf
    for _ in range(max(1, n // 3)):                               # exact ties inside columns
        a, b = rng.integers(0, n, 2)
        mat[b] = mat[a]
    mat[:, 0] = np.nan                                            # a column nothing enters
    return mat


def _edge_distances(rng, m, lo, hi):
    d = rng.uniform(lo, hi, size=m)
    edge = [np.nan, np.inf, -np.inf, 1e301, -1e301, 0.0]
    for i, v in enumerate(edge):
        if i + 1 < m:
            d[i + 1] = v
    return d


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("mode", ["refcos", "dtw"])
def test_against_the_oracle_topk(oracle, seed, mode):
    rng = np.random.default_rng(0x70BE + seed)
    n, m = int(rng.integers(1, 40)), int(rng.integers(7, 30))
    kw = ref.REFCOS if mode == "refcos" else ref.DTW
    mat = _edge_matrix(rng, n, m, -1.0, 1.0) if mode == "refcos" else _edge_matrix(rng, n, m, 0.0, 50.0)
    dist = _edge_distances(rng, m, 0.0, 1.2 if mode == "refcos" else 40.0)
    for k in (1, 2, n, n + 3, 64):
        for d in (None, dist):
            want_idx, want_key = oracle.topk(mat, k, distance=d, default_distance=kw["default_distance"],
                                             fold_start=kw["fold_start"])
            idx, key = ref.topk(mat, k, d, kw["default_distance"], kw["fold_start"], 0, "key")
            assert np.array_equal(idx, want_idx)
            assert _same(key, want_key)
            # report="value" gathers the entry behind the same index
            idx2, val = ref.topk(mat, k, d, kw["default_distance"], kw["fold_start"], 0, "value")
            assert np.array_equal(idx2, idx)
            have = idx >= 0
            assert _same(val[have], mat[idx[have], np.nonzero(have)[0]]) and np.isnan(val[~have]).all()


def _segments(rng, n, fmax, dim, scale):
    return [rng.normal(size=(int(rng.integers(1, fmax)), dim)) * scale for _ in range(n)]


@pytest.mark.parametrize("seed", range(3))
def test_first_against_the_oracle_searches(oracle, seed):
    """`first` on the oracle's matrices against the oracle's own sequential searches (which never build a matrix)."""
    from soundsym_amd.engine import pack_segments
    rng = np.random.default_rng(0xF1A5 + seed)
    dim = 6
    src, tgt = _segments(rng, 23, 9, dim, 0.3), _segments(rng, 11, 9, dim, 0.3)
    src[5] = src[2].copy()
    src[0] = np.zeros_like(src[0])                    # norm 0: similarity NaN, never wins
    tgt[4] = np.zeros((0, dim))                       # empty target: nothing wins
    tgt[6] = src[2].copy()
    sf, so = pack_segments(src, dim)
    tf, to = pack_segments(tgt, dim)
    dist = _edge_distances(rng, len(tgt), 0.0, 1.2)
    sims = oracle.refcos_matrix(sf, so, tf, to, dim)
    for d in (None, dist):
        want_idx, want_val = oracle.refcos_match_all(sf, so, tf, to, dim, distance=d)
        idx, val = ref.first(sims, d, **ref.REFCOS)
        assert np.array_equal(idx, want_idx) and _same(val, want_val)
        tidx, tval = ref.topk(sims, 4, d, **ref.REFCOS)
        has = tidx[:, 0] >= 0
        assert np.array_equal(tidx[has, 0], idx[has]) and _same(tval[has, 0], val[has])
        assert (idx[~has] == 0).all() and (val[~has] == 2.0).all()
    idx, cost, mat = oracle.dtw_match_all(sf, so, tf, to, dim, want_matrix=True)
    got_idx, got_cost = ref.first(mat, None, **ref.DTW)
    assert np.array_equal(got_idx, idx) and _same(got_cost, cost)
    assert got_cost[4] == INF and got_idx[4] == 0


def test_assert_separated_sees_a_near_tie_and_accepts_an_exact_one():
    mat = np.array([[1.0], [1.0], [2.0], [3.0]])
    ref.assert_separated(mat, 2)                                  # an exact tie is fine
    mat[1, 0] = 1.0 + 1e-12
    with pytest.raises(AssertionError):
        ref.assert_separated(mat, 2)
    mat[1, 0] = 1.5
    mat[3, 0] = 2.0 + 1e-11                                       # ... also between the k-th and the k + 1-th key
    with pytest.raises(AssertionError):
        ref.assert_separated(mat, 3)
    ref.assert_separated(mat, 2)
    # a distance next to the costs: the gap counts relative to the costs, not to the tiny keys
    near = np.array([[100.0], [100.0 + 1e-8], [50.0]])
    with pytest.raises(AssertionError):
        ref.assert_separated(near, 1, np.array([100.0 - 1e-8]))
