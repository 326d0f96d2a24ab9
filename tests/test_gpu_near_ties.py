"""The dtw search on near-ties the f32 filter cannot order (cases and rungs: tests/near_tie_cases.py; their conditions
on the oracle alone: tests/test_near_tie_cases.py).

Every test holds the ANSWER to the f64 oracle: the index equal to the oracle's first minimum for every target, the cost
within the exact kernel's 1e-12 relative, the filter route taken (Engine.timings), and the all-pairs route
(force_exact) equal bit for bit.  On these inputs a margin that is too small, a certificate that is too generous, a
two-sided interval where the filter bounds from below only, a threshold that abandons the nearer twin or a merge that
orders near-equal costs by shard returns a wrong index.

Each test also reads the filter's own matrix (pair_matrix, exact=False) and counts, over the blind targets, how often
the filter ties the two contenders or ranks the farther one first; the count is printed and must be at least 1, or the
case has no power on the route.  That is an assertion about the INPUTS which only a GPU can check.
"""
import time

import numpy as np
import pytest

import near_tie_cases as ntc
import topk_ref as ref
from soundsym_amd import Engine
from soundsym_amd.engine import pack_segments
from test_gpu_comm import _run_ranks, _split

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12


class _Sets:
    """A case resident on an engine of its own configuration."""

    def __init__(self, c):
        self.c = c
        self.e = Engine(metric="dtw", dtype=c.dtype, band=c.band, squared=c.squared)
        sf, so = pack_segments(c.src, c.dim, c.np_dtype)
        tf, to = pack_segments(c.tgt, c.dim, c.np_dtype)
        self.d, self.q = self.e.dictionary(sf, so, c.dim), self.e.queries(tf, to, c.dim)
        self.want_idx, self.want_cost = ref.first(c.mat, c.distance, **ref.DTW)

    def close(self):
        self.e.close()


@pytest.fixture
def sets(request, oracle):
    made = []

    def make(name):
        made.append(_Sets(ntc.build(name)))
        return made[-1]
    yield make
    for s in made:
        s.close()


def _explain(c, fm, idx, want_idx):
    """What a wrong index needs to be traced: per wrong target, the contenders' filter costs, bounds and exact costs."""
    lines = []
    for t in np.flatnonzero(np.asarray(idx).astype(np.int64) != want_idx)[:8]:
        lines.append("target %d (%s, gap %.3g): got %d, want %d, distance %r" % (
            t, c.rung[t], c.gap[t], idx[t], want_idx[t], None if c.distance is None else c.distance[t]))
        for s in sorted(set(c.contenders[t]) | {int(idx[t]) % len(c.src)}):
            lines.append("    source %4d: filter %.9g  bound %.4g  exact %.17g" % (s, fm[s, t], c.bound[s, t], c.mat[s, t]))
    return "\n".join(lines)


def check_answer(c, idx, cost, want_idx, want_cost, fm=None):
    wrong = int((np.asarray(idx).astype(np.int64) != want_idx).sum())
    assert wrong == 0, "%s: %d wrong indices\n%s" % (c.name, wrong, _explain(c, fm if fm is not None else c.mat * np.nan,
                                                                                 idx, want_idx))
    assert np.all(np.abs(cost - want_cost) <= EXACT_RTOL * np.abs(want_cost)), c.name


def filter_confusions(c, fm):
    """Over the blind targets (beyond the filter's reach: every target): how often the filter's own keys tie the two
    contenders or rank the farther one first."""
    key_f = ref.keys(fm, c.distance, 0.0)
    key = ref.keys(c.mat, c.distance, 0.0)
    n = 0
    for t, cont in enumerate(c.contenders):
        if c.rung[t] not in ("blind", "reach"):
            continue
        order = sorted(cont, key=lambda s: (key[s, t], s))
        near, far = order[0], order[1]
        n += bool(key_f[near, t] >= key_f[far, t])
    return n


def assert_power(c, n):
    assert n >= 1, ("%s: the filter ordered the contenders of every blind target rightly, so this case cannot tell a "
                    "wrong selection from a right one on this route.  This says nothing about a kernel: the INPUTS lack "
                    "power -- change the case's seed in tests/near_tie_cases.py" % c.name)


def search(s, what="match", **kw):
    """The checks every test makes on one call; returns (idx, cost, timings)."""
    c, e = s.c, s.e
    t0 = time.perf_counter()
    fm = e.pair_matrix(s.d, s.q, exact=False)
    idx, cost = e.match(s.d, s.q, distance=c.distance, **kw)
    tm = e.timings()
    check_answer(c, idx, cost, s.want_idx, s.want_cost, fm)
    assert tm["used_filter"] == 1, tm
    idx2, cost2 = e.match(s.d, s.q, distance=c.distance, force_exact=True)
    assert e.timings()["used_filter"] == 0
    assert np.array_equal(idx, idx2) and np.array_equal(cost, cost2)
    n = filter_confusions(c, fm)
    print("\n%-12s %s: filter ties or inversions on blind targets %d of %d, n_refined %d of %d pairs, %.2f s" % (
        c.name, what, n, sum(r in ("blind", "reach") for r in c.rung), tm["n_refined"], tm["n_pairs"],
        time.perf_counter() - t0))
    assert_power(c, n)
    return idx, cost, tm


# (1)-(9): every route of the first-minimum search
@pytest.mark.parametrize("name", ntc.FIRST_MINIMUM)
def test_first_minimum_on_near_ties(sets, name):
    s = sets(name)
    idx, cost, tm = search(s)
    assert tm["pruned"] == 0
    if s.c.distance is None:                                  # the oracle's own fold agrees with the restated one
        assert np.array_equal(s.want_idx, np.argmin(s.c.mat, axis=0))


# (10): top-k on the quadruples
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_topk_on_quadruples(sets, oracle, k):
    s = sets("quads")
    c, e = s.c, s.e
    t0 = time.perf_counter()
    want_idx, want_cost = ref.rows(c.mat, k, None, **ref.DTW)
    o_idx, _ = oracle.topk(c.mat, k, default_distance=0.0, fold_start=float("inf"))
    assert np.array_equal(o_idx, want_idx)
    idx, cost = e.match_topk(s.d, s.q, k)
    tm = e.timings()
    assert tm["used_filter"] == 1, tm
    got = ref.rows_as_int64(idx)
    for t in np.flatnonzero((got != want_idx).any(axis=1))[:4]:
        fm = e.pair_matrix(s.d, s.q, exact=False)
        print("quads k=%d target %d (%s): got %s, want %s" % (k, t, c.rung[t], got[t], want_idx[t]))
        for src in c.contenders[t]:
            print("    source %4d: filter %.9g  bound %.4g  exact %.17g" % (src, fm[src, t], c.bound[src, t], c.mat[src, t]))
    ref.check_rows(idx, cost, want_idx, want_cost, rtol=EXACT_RTOL)
    one, c1 = e.match(s.d, s.q)
    ref.check_first_entry(idx, cost, one, c1)
    check_answer(c, one, c1, s.want_idx, s.want_cost)
    idx2, cost2 = e.match_topk(s.d, s.q, k, force_exact=True)
    assert e.timings()["used_filter"] == 0
    assert np.array_equal(idx, idx2) and np.array_equal(cost, cost2, equal_nan=True)
    n = filter_confusions(c, e.pair_matrix(s.d, s.q, exact=False))
    print("\nquads k=%d: filter ties or inversions on blind targets %d of %d, n_refined %d of %d pairs, %.2f s" % (
        k, n, c.rung.count("blind"), tm["n_refined"], tm["n_pairs"], time.perf_counter() - t0))
    assert_power(c, n)


# (11): early abandoning
@pytest.mark.parametrize("name", ["sp", "mid", "band3", "band8"])
def test_pruned_search_on_near_ties(sets, name):
    s = sets(name)
    e = s.e
    i0, c0 = e.match(s.d, s.q)
    t0 = e.timings()
    i1, c1, t1 = search(s, what="prune", prune=True)
    assert t0["pruned"] == 0 and t1["pruned"] == 1 and t1["used_filter"] == 1          # (as tests/test_gpu_prune.py)
    assert np.array_equal(i0, i1) and np.array_equal(c0, c1)


# (12): sharded, in process
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,prune", [("sp", False), ("sp", True), ("tied", False)])
def test_sharded_ranks_return_the_oracles_indices(oracle, world, name, prune):
    c = ntc.build(name)
    t0 = time.perf_counter()
    want_idx, want_cost = ref.first(c.mat, c.distance, **ref.DTW)
    shards, bases = _split(c.src, world, c.dim, c.np_dtype)
    tf, to = pack_segments(c.tgt, c.dim, c.np_dtype)
    res = _run_ranks(world, "dtw", c.dtype, shards, c.dim, tf, to, bases, band=c.band, distance=c.distance, prune=prune)
    if not c.tied:                                            # contenders of a target in different shards: all of them
        cut = np.searchsorted(np.array(bases), np.array([list(x) for x in c.contenders]), side="right")     # where the
        across = int((cut[:, 0] != cut[:, 1]).sum())                                        # shards are the blocks
        assert across == len(c.tgt) if world == c.blocks else across >= len(c.tgt) // 4, across
    for r in range(world):
        idx, cost, tm = res[r]
        check_answer(c, idx, cost, want_idx, want_cost)       # every rank: the oracle's answer, not only the unsharded call's
        assert tm["used_filter"] == 1 and tm["attempts"] == 1 and tm["pruned"] == (1 if prune else 0), (r, tm)
    print("\n%-12s world %d prune %d: n_refined per rank %s, %.2f s" % (
        name, world, prune, [res[r][2]["n_refined"] for r in range(world)], time.perf_counter() - t0))
    e = Engine(metric="dtw", dtype=c.dtype, band=c.band)      # the power of the inputs: one shard's filter matrix is the set's
    sf, so = pack_segments(c.src, c.dim, c.np_dtype)
    fm = e.pair_matrix(e.dictionary(sf, so, c.dim), e.queries(tf, to, c.dim), exact=False)
    e.close()
    assert_power(c, filter_confusions(c, fm))


# (13): the selection without its pretests
@pytest.mark.parametrize("name", ["sp", "tied"])
def test_without_the_selections_pretests(sets, monkeypatch, name):
    s = sets(name)
    i0, c0, t0 = search(s)
    monkeypatch.setenv("SSYM_SELECT_PRETEST", "0")
    i1, c1, t1 = search(s, what="no pretest")
    assert np.array_equal(i0, i1) and np.array_equal(c0, c1)
