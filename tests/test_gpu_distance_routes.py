"""Per-target distances (k = 1) on the entry points around ssym_match_queries, both metrics: ssym_match_batch and
ssym_match_one on either side of the few-targets shortcut, ssym_match_begin / ssym_match_finish on the routes where the
filter applies and where it does not, and a dictionary grown by ssym_dict_append.

The distance vectors hold NaN, +inf, -inf and a value beyond every key.  Every answer is compared with
ssym_match_queries for the same arguments bit for bit and with tests/topk_ref.py on the CPU oracle's matrix (refcos bit
for bit; dtw: indices equal, costs within 1e-12 relative, after the tie-separation precondition of
test_gpu_topk_dtw_shapes.py).  Every case asserts its route from Engine.timings(): the one-launch kernels of
ssym_match_batch leave pack_ms = 0, n_refined = 0 and main_launches = 1; the all-pairs dtw route has n_refined = n_pairs;
the filters set used_filter / refcos_filter.
"""
import numpy as np
import pytest

import topk_ref as ref
from soundsym_amd import Engine, synth
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12
NAN, INF = float("nan"), float("inf")


def _segs(seed, n, lo, hi, dim, dtype, scale=None):
    rng = np.random.default_rng(seed)
    sc = synth.sigma(dim) if scale is None else scale
    return [(rng.normal(size=(int(rng.integers(lo, hi + 1)), dim)) * sc).astype(dtype) for _ in range(n)]


def _dists(seed, m, lo, hi, far):
    d = np.random.default_rng(seed).uniform(lo, hi, size=m)
    for i, v in enumerate([NAN, INF, -INF, far]):
        if i < m - 1:
            d[i + 1] = v
    return d


def _matrix(oracle, metric, sf, so, tf, to, dim, band=-1):
    sf, tf = np.asarray(sf, dtype=np.float64), np.asarray(tf, dtype=np.float64)
    if metric == "refcos":
        return oracle.refcos_matrix(sf, so, tf, to, dim)
    return oracle.dtw_match_all(sf, so, tf, to, dim, band=band, nthreads=oracle.max_threads(), want_matrix=True)[2]


def _check_against_ref(metric, mat, dist, idx, val, base=0):
    kw = ref.REFCOS if metric == "refcos" else ref.DTW
    want_idx, want_val = ref.first(mat, dist, index_base=base, **kw)
    assert np.array_equal(np.asarray(idx).astype(np.int64), want_idx)
    if metric == "refcos":
        assert np.array_equal(val, want_val)
    else:
        ref.assert_separated(mat, 1, dist)
        fin = np.isfinite(want_val)
        assert np.array_equal(np.isfinite(val), fin) and (np.asarray(val)[~fin] == INF).all()
        assert np.all(np.abs(np.asarray(val)[fin] - want_val[fin]) <= EXACT_RTOL * np.abs(want_val[fin]))


def one_launch(tm):
    assert tm["pack_ms"] == 0 and tm["main_launches"] == 1 and tm["n_refined"] == 0 and tm["used_filter"] == 0, tm


def packed_then(route):
    def check(tm):
        assert tm["pack_ms"] > 0, tm                            # the targets were packed: not the one-launch kernels
        route(tm)
    return check


def dtw_filter(tm):
    assert tm["used_filter"] == 1, tm


def dtw_all_pairs(tm):
    assert tm["used_filter"] == 0 and tm["n_refined"] == tm["n_pairs"], tm


def refcos_tile(tm):
    assert tm["used_filter"] == 0 and tm["refcos_filter"] == 0, tm


def refcos_q8(tm):
    assert tm["used_filter"] == 1 and tm["refcos_filter"] == 2, tm


def _batch_case(oracle, e, metric, src, tgt, dim, route, far):
    """ssym_match_batch (and ssym_match_one for a single target) against ssym_match_queries and the restatement."""
    sf, so = pack_segments(src, dim, e.np_dtype)
    tf, to = pack_segments(tgt, dim, e.np_dtype)
    d = e.dictionary(sf, so, dim)
    mat = _matrix(oracle, metric, sf, so, tf, to, dim)
    fin = mat[np.isfinite(mat)]
    dist = _dists(len(src) + len(tgt), len(tgt), 0.0, float(np.median(fin)) if metric == "dtw" else 1.2, far)
    if len(tgt) == 1:
        dist = np.array([dist[0]])
    for dd in (dist, None):
        bi, bv = e.match_batch(d, tf, to, dd)
        tm = e.timings()
        print(metric, "batch n=%d m=%d:" % (len(src), len(tgt)), tm)
        route(tm)
        ri, rv = e.match(d, e.queries(tf, to, dim), dd)
        assert np.array_equal(bi, ri) and np.array_equal(bv, rv)
        _check_against_ref(metric, mat, dd, bi, bv)
    if len(tgt) == 1:
        for v in (float(dist[0]), NAN, INF, -INF, far):
            oi, ov = e.match_one(d, tf, v)
            route(e.timings())
            ri, rv = e.match(d, e.queries(tf, to, dim), np.array([v]))
            assert oi == int(ri[0]) and (ov == rv[0])
            _check_against_ref(metric, mat, np.array([v]), np.array([oi]), np.array([ov]))
    d.close()


@pytest.mark.parametrize("n,m,sf_max,tf_max,route", [
    (100, 4, 20, 20, one_launch),                               # four targets: dtw_match_few_kernel
    (100, 5, 20, 20, packed_then(dtw_filter)),                  # five: packed, the filter route
    (2048, 4, 6, 6, one_launch),                                # N M = 8192
    (2049, 4, 6, 6, packed_then(dtw_filter)),                   # N M = 8196 (8193 is no multiple of a target count > 1)
    (8192, 1, 6, 6, one_launch),                                # N M = 8192, ssym_match_one
    (8193, 1, 6, 6, packed_then(dtw_filter)),                   # N M = 8193
    (60, 1, 64, 64, one_launch),                                # 64-frame entries: the kernel's longest
    (60, 1, 65, 63, packed_then(dtw_all_pairs)),                # 65 + 63 = 128 frames: the exact kernel on every pair
    (60, 1, 65, 64, packed_then(dtw_filter)),                   # 65 + 64 = 129: the filter route
])
def test_dtw_batch_either_side_of_the_few_targets_shortcut(oracle, n, m, sf_max, tf_max, route):
    e = Engine(metric="dtw", dtype="f32")
    src = _segs(0xD15700 + n, n, 3, sf_max, 13, np.float32)
    tgt = _segs(0xD15800 + m + tf_max, m, 3, tf_max, 13, np.float32)
    src[0] = _segs(1, 1, sf_max, sf_max, 13, np.float32)[0]    # the longest lengths are there
    tgt[0] = _segs(2, 1, tf_max, tf_max, 13, np.float32)[0]
    src[n - 1] = src[1].copy()                                  # a tie: the lower index
    _batch_case(oracle, e, "dtw", src, tgt, 13, route, 1e6)
    e.close()


@pytest.mark.parametrize("n,m,frames,route", [
    (1100, 64, 8, one_launch),                                  # kFewMaxQueries = 64 queries: refcos_match_one_kernel
    (1100, 65, 8, packed_then(refcos_q8)),                      # 65: packed; 71 500 pairs take the integer filter
    (300, 1, 341, one_launch),                                  # 341 x 12 = 4092 <= kOneMaxVals = 4096 query values
    (300, 1, 342, packed_then(refcos_tile)),                    # 4104 values: packed, the tile kernel
])
def test_refcos_batch_either_side_of_the_few_targets_shortcut(oracle, n, m, frames, route):
    e = Engine(metric="refcos", dtype="f64")
    src = _segs(0xD15900 + n, n, 1, 12, 12, np.float64, 0.3)
    tgt = _segs(0xD15A00 + m + frames, m, 1, frames, 12, np.float64, 0.3)
    tgt[0] = _segs(3, 1, frames, frames, 12, np.float64, 0.3)[0]
    src[n - 1] = src[1].copy()
    if m > 1:
        tgt[m - 1] = src[1].copy()
    _batch_case(oracle, e, "refcos", src, tgt, 12, route, 1e301)
    e.close()


# -- ssym_match_begin / ssym_match_finish -----------------------------------------------------------------------------
def _begin_finish(e, d, q, dist, base=0):
    import torch
    b = torch.full((q.n,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.match_begin(d, q, b, distance=None if dist is None else dist.copy(), index_base=base)
    oi = torch.full((q.n,), 12345, dtype=torch.int32, device="cuda")
    oc = torch.full((q.n,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()             # (the fills ran on torch's stream, the library writes on its own)
    e.match_finish(b, oi, oc)
    tm = e.timings()
    e.synchronize()
    return oi.cpu().numpy().view(np.uint32), oc.cpu().numpy(), b.cpu().numpy(), tm


def _filter_sets():
    g = synth.make_grid(96, 40, 24, 13, 0x5EED0E01)
    return [x for x in g.sources], [x for x in g.targets], 13


def _wide_sets():
    g = synth.make_grid(96, 40, 24, 50, 0x5EED0E02)
    return [x for x in g.sources], [x for x in g.targets], 50


def _nonfinite_sets():
    src, tgt, dim = _filter_sets()
    src[7] = src[7].copy()
    src[7][3, 2] = NAN
    src[8] = src[8].copy()
    src[8][0, 0] = INF
    return src, tgt, dim


def _refcos_sets():
    return _segs(0xD15B00, 300, 2, 20, 12, np.float64, 0.3), _segs(0xD15B01, 260, 2, 20, 12, np.float64, 0.3), 12


@pytest.mark.parametrize("name,metric,sets,filtered,route", [
    ("filter", "dtw", _filter_sets, True, dtw_filter),
    ("wide frames", "dtw", _wide_sets, False, dtw_filter),      # (the plain search of finish takes the cascade)
    ("non-finite", "dtw", _nonfinite_sets, False, dtw_all_pairs),
    ("refcos", "refcos", _refcos_sets, False, refcos_q8),
])
def test_finish_answers_for_the_distances_given_to_begin(oracle, name, metric, sets, filtered, route):
    src, tgt, dim = sets()
    e = Engine(metric=metric, dtype="f32" if metric == "dtw" else "f64")
    sf, so = pack_segments(src, dim, e.np_dtype)
    tf, to = pack_segments(tgt, dim, e.np_dtype)
    d, q = e.dictionary(sf, so, dim), e.queries(tf, to, dim)
    mat = _matrix(oracle, metric, sf, so, tf, to, dim)
    fin = mat[np.isfinite(mat)]
    hi = float(np.median(fin)) if metric == "dtw" else 1.2
    far = 1e6 if metric == "dtw" else 1e301
    dist_a, dist_b = _dists(11, len(tgt), 0.0, hi, far), _dists(12, len(tgt), 0.0, hi, far)[::-1].copy()
    for dist in (dist_a, dist_b, None):
        want_i, want_c = e.match(d, q, dist, index_base=3)
        route(e.timings())
        gi, gc, bounds, tm = _begin_finish(e, d, q, dist, 3)
        print(name, "begin/finish:", tm)
        route(tm)
        if dist is None and name == "wide frames":
            pass                                                  # (without distances the filter's bounds go out)
        elif filtered:
            assert np.isfinite(bounds).any() and (bounds >= 0).all()
        else:
            assert (bounds == INF).all()                          # "the filter does not apply": begin writes +inf
        assert np.array_equal(gi, want_i) and np.array_equal(gc, want_c)
        _check_against_ref(metric, mat, dist, gi, gc, 3)
    # a second begin with other distances: finish gives the second answer
    import torch
    b = torch.zeros(len(tgt), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.match_begin(d, q, b, distance=dist_a)
    gi, gc, _, _ = _begin_finish(e, d, q, dist_b)
    want_i, want_c = e.match(d, q, dist_b)
    assert np.array_equal(gi, want_i) and np.array_equal(gc, want_c)
    assert not np.array_equal(gi, e.match(d, q, dist_a)[0])       # (the two answers do differ)
    # begin without distances after begin with distances: the old ones are gone
    e.match_begin(d, q, b, distance=dist_a)
    gi, gc, _, _ = _begin_finish(e, d, q, None)
    want_i, want_c = e.match(d, q, None)
    assert np.array_equal(gi, want_i) and np.array_equal(gc, want_c)
    _check_against_ref(metric, mat, None, gi, gc)
    e.close()


# -- ssym_dict_append -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dtw", "refcos"])
def test_distances_on_a_dictionary_grown_by_append(oracle, metric):
    """Match with distances, append 1 and then 300 segments, match again: each time what a dictionary created whole
    gives.  refcos: 300 x 260 pairs take the integer filter, so the records exist before the first append."""
    if metric == "dtw":
        e, dim, npdt = Engine(metric="dtw", dtype="f32"), 13, np.float32
        src, tgt = _segs(0xD15C00, 601, 5, 30, dim, npdt), _segs(0xD15C01, 260, 5, 30, dim, npdt)
        route, hi, far = dtw_filter, None, 1e6
    else:
        e, dim, npdt = Engine(metric="refcos", dtype="f64"), 12, np.float64
        src, tgt = _segs(0xD15C02, 601, 2, 20, dim, npdt, 0.3), _segs(0xD15C03, 260, 2, 20, dim, npdt, 0.3)
        route, hi, far = refcos_q8, 1.2, 1e301
    src[300] = src[4].copy()                                      # the appended segments tie with an old one: it stays first
    src[450] = src[4].copy()
    tgt[0] = src[4].copy()
    tf, to = pack_segments(tgt, dim, npdt)
    q = e.queries(tf, to, dim)
    sf0, so0 = pack_segments(src[:300], dim, npdt)
    grown = e.dictionary(sf0, so0, dim)
    have = 300
    for add in (0, 1, 300):
        if add:
            af, ao = pack_segments(src[have:have + add], dim, npdt)
            e.dictionary_append(grown, af, ao)
            have += add
        sf, so = pack_segments(src[:have], dim, npdt)
        mat = _matrix(oracle, metric, sf, so, tf, to, dim)
        dist = _dists(have, len(tgt), 0.0, hi if hi else float(np.median(mat)), far)
        dist[0] = mat[4, 0]                                       # key 0 for source 4 and its copies
        whole = e.dictionary(sf, so, dim)
        for dd in (dist, None):
            gi, gv = e.match(grown, q, dd)
            route(e.timings())
            wi, wv = e.match(whole, q, dd)
            assert np.array_equal(gi, wi) and np.array_equal(gv, wv)
            _check_against_ref(metric, mat, dd, gi, gv)
        assert gi.shape == (260,) and e.match(grown, q, dist)[0][0] == 4
        whole.close()
    e.close()
