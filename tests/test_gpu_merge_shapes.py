"""ssym_merge_shards / ssym_merge_shards_at at every shape they accept, against tests/tail_ref.py's merge: exact.

merge_shards_kernel seeds its fold with shard 0's entry, one thread per target: the cases here place NaN, +inf and
dense ties in every shard position, use per-target distances with ties from both sides of the distance, and target
counts on both sides of the 256-thread workgroup."""
import ctypes

import numpy as np
import pytest

import tail_ref
from soundsym_amd import Engine
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHARDS = [1, 2, 3, 8, 64]
TARGETS = [0, 1, 255, 256, 257, 100_001]


@pytest.fixture(scope="module")
def dtw():
    e = Engine(metric="dtw", dtype="f32")
    yield e
    e.close()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _indices(rng, g, m):
    """Global indices of shards ordered by index, with some repeated across shards (a tie on key AND index picks
    either: same answer)."""
    return (np.arange(g, dtype=np.int64)[:, None] * 1_000_000 + rng.integers(0, 1_000_000, size=(g, m))).astype(np.uint32)


def _run(e, costs, idx, distance=None, plain=False):
    g, m = costs.shape
    if m:
        c, i = torch.from_numpy(costs).cuda(), torch.from_numpy(idx.view(np.int32)).cuda()
    else:                                           # (an empty tensor has no address; NULL is an error even for no targets)
        c, i = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    oi = torch.full((m + 3,), -77, dtype=torch.int32, device="cuda")
    oc = torch.full((m + 3,), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if plain:
        assert distance is None
        nat.check(nat.lib().ssym_merge_shards(e.ctx, g, m, c.data_ptr(), i.data_ptr(), oi.data_ptr(), oc.data_ptr()), e.ctx)
    elif m:
        e.merge_shards(c, i, oi, oc, distance)
    else:
        dp = None if distance is None else np.zeros(1).ctypes.data
        nat.check(nat.lib().ssym_merge_shards_at(e.ctx, g, 0, c.data_ptr(), i.data_ptr(), dp, oi.data_ptr(),
                                                 oc.data_ptr()), e.ctx)
    oi, oc = oi.cpu().numpy(), oc.cpu().numpy()
    assert (oi[m:] == -77).all() and (oc[m:] == -7.25).all()              # nothing past the last target
    return oi[:m].view(np.uint32), oc[:m]


def _check(e, costs, idx, distance=None):
    want_idx, want_cost = tail_ref.merge(costs, idx, distance)
    got_idx, got_cost = _run(e, costs, idx, distance)
    assert np.array_equal(got_idx, want_idx)
    assert np.array_equal(_bits(got_cost), _bits(want_cost))
    return got_idx, got_cost


@pytest.mark.parametrize("m", TARGETS)
@pytest.mark.parametrize("g", SHARDS)
def test_dense_ties_inf_and_nan(dtw, g, m):
    rng = np.random.default_rng(0x3E60 + 1000 * g + m % 997)
    costs = rng.integers(0, 5, size=(g, m)).astype(np.float64)           # integer costs: many exact ties
    costs[rng.random((g, m)) < 0.15] = np.inf
    costs[rng.random((g, m)) < 0.10] = np.nan
    idx = _indices(rng, g, m)
    if m >= 255:
        costs[:, 3] = np.inf                                              # a column of +inf: the lowest index wins
        idx[:, 3] = idx[::-1, 3].copy()                                   # ... which the LAST shard holds here
        costs[:, 5] = np.nan                                              # NaN in every shard: shard 0's entry stays
        costs[:, 7], costs[0, 7] = 2.0, np.nan                            # NaN in shard 0 only
        costs[:, 9], costs[g - 1, 9] = 2.0, np.nan                        # NaN in the last shard only
        costs[:, m - 1], costs[0, m - 1] = np.inf, np.nan                 # the last target: NaN, then +inf
    got_idx, got_cost = _check(dtw, costs, idx)
    if m >= 255:
        assert got_idx[3] == idx[:, 3].min() and got_cost[3] == np.inf
        assert got_idx[5] == idx[0, 5] and np.isnan(got_cost[5])
        if g > 1:
            assert got_cost[7] == 2.0 and got_idx[7] == idx[1:, 7].min()
            assert got_cost[9] == 2.0 and got_idx[9] == idx[:g - 1, 9].min()
            assert got_cost[m - 1] == np.inf and got_idx[m - 1] == idx[1:, m - 1].min()
    # the entry point without distances is the same call
    plain_idx, plain_cost = _run(dtw, costs, idx, plain=True)
    assert np.array_equal(plain_idx, got_idx) and np.array_equal(_bits(plain_cost), _bits(got_cost))


@pytest.mark.parametrize("m", TARGETS)
@pytest.mark.parametrize("g", SHARDS)
def test_with_distances(dtw, g, m):
    rng = np.random.default_rng(0x3E61 + 1000 * g + m % 997)
    costs = rng.integers(0, 9, size=(g, m)).astype(np.float64)
    costs[rng.random((g, m)) < 0.1] = np.inf
    costs[rng.random((g, m)) < 0.1] = np.nan
    idx = _indices(rng, g, m)
    dist = rng.integers(0, 9, size=m).astype(np.float64)                  # |c - d| ties from both sides of d
    dist[rng.random(m) < 0.2] += 0.5
    if m >= 255 and g >= 2:
        costs[:, 11], costs[g - 1, 11], dist[11] = 1.0, 40.0, 39.0        # the far entry is the best key
        costs[:, 13], costs[0, 13], costs[g - 1, 13], dist[13] = 0.0, 3.0, 7.0, 5.0   # keys 2 and 2 from both sides
        idx[0, 13], idx[g - 1, 13] = 900, 17                              # ... and the one above d has the lower index
        costs[:, 15], costs[0, 15], dist[15] = 6.0, np.nan, 6.0           # NaN in shard 0 against keys of 0
        dist[17] = np.inf                                                 # |c - inf|: +inf for finite c, NaN for +inf
    got_idx, got_cost = _check(dtw, costs, idx, dist)
    if m >= 255 and g >= 2:
        assert got_cost[11] == 40.0 and got_idx[11] == idx[g - 1, 11]
        assert got_idx[13] == 17 and got_cost[13] == 7.0
        assert got_cost[15] == 6.0
    # zero distances are the plain merge
    zero_idx, zero_cost = _run(dtw, costs, idx, np.zeros(m))
    want_idx, want_cost = tail_ref.merge(costs, idx)
    assert np.array_equal(zero_idx, want_idx) and np.array_equal(_bits(zero_cost), _bits(want_cost))


def test_errors_leave_the_outputs_untouched(dtw):
    L, ctx = nat.lib(), dtw.ctx
    c = torch.zeros((2, 10), dtype=torch.float64, device="cuda")
    i = torch.zeros((2, 10), dtype=torch.int32, device="cuda")
    oi = torch.full((10,), -77, dtype=torch.int32, device="cuda")
    oc = torch.full((10,), -7.25, dtype=torch.float64, device="cuda")
    dist = np.zeros(10)
    torch.cuda.synchronize()
    for shards, cp, ip, op in [(0, c.data_ptr(), i.data_ptr(), oi.data_ptr()), (2, None, i.data_ptr(), oi.data_ptr()),
                               (2, c.data_ptr(), None, oi.data_ptr()), (2, c.data_ptr(), i.data_ptr(), None)]:
        assert L.ssym_merge_shards_at(ctx, shards, 10, cp, ip, dist.ctypes.data, op, oc.data_ptr()) == nat.SSYM_E_INVALID
        assert L.ssym_merge_shards(ctx, shards, 10, cp, ip, op, oc.data_ptr()) == nat.SSYM_E_INVALID
        assert L.ssym_last_error(ctx)
        assert bool((oi == -77).all()) and bool((oc == -7.25).all())
    # out_cost may be NULL
    assert L.ssym_merge_shards(ctx, 2, 10, c.data_ptr(), i.data_ptr(), oi.data_ptr(), None) == nat.SSYM_OK
    assert bool((oi == 0).all()) and bool((oc == -7.25).all())
