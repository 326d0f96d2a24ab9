"""tests/tail_ref.py against the C oracle and against answers worked out by hand: two restatements of the same
reference lines, written separately, that agree.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import tail_ref
from oracle.oracle import pack_segments

M31 = 2147483647

# (sample, the 32-bit value Sound::write_file stores for it), each worked out by hand:
#   1 - 2^-53 times (2^31 - 1) is 2^31 - 1 - 2^-22 + 2^-53, which rounds to 2^31 - 1 - 2^-22 and truncates to 2^31 - 2;
#   1 + 2^-52 gives 2^31 - 1 + 2^-21 after rounding: above i32::MAX only in its fraction, it truncates to i32::MAX;
#   fl(1 / (2^31 - 1)) times 2^31 - 1 rounds to exactly 1.0; 0.9 / and 1.9 / (2^31 - 1) give 0.9 and 1.9
PCM_EDGES = [
    (0.0, 0), (-0.0, 0),
    (1.0, M31), (-1.0, -M31),
    (float(np.nextafter(1.0, 0.0)), M31 - 1), (float(np.nextafter(-1.0, 0.0)), -(M31 - 1)),
    (float(np.nextafter(1.0, np.inf)), M31), (float(np.nextafter(-1.0, -np.inf)), -M31),
    (0.5, 1073741823), (-0.5, -1073741823),
    (1.0 / M31, 1), (-1.0 / M31, -1),
    (0.9 / M31, 0), (-0.9 / M31, 0),
    (1.9 / M31, 1), (-1.9 / M31, -1),
    (math.inf, M31), (-math.inf, -M31 - 1), (math.nan, 0),
    (5e-324, 0), (-5e-324, 0),
    (1e300, M31), (-1e300, -M31 - 1),
    (1.5, M31), (-1.5, -M31 - 1),
]


def _ragged(rng, n, dim, lo, hi):
    return [rng.normal(size=(int(rng.integers(lo, hi + 1)), dim)) for _ in range(n)]


@pytest.mark.parametrize("x,want", PCM_EDGES, ids=[repr(x) for x, _ in PCM_EDGES])
def test_pcm32_known_answers(oracle, x, want):
    assert tail_ref.pcm32(x) == want
    assert int(oracle.pcm32([x])[0]) == want


def test_pcm32_against_the_oracle_and_exact_arithmetic(oracle):
    rng = np.random.default_rng(0x7A11)
    xs = np.concatenate([rng.uniform(-1.2, 1.2, size=4000), rng.uniform(-3, 3, size=500) / M31,
                         np.arange(-40, 41) / M31, 1.0 - rng.uniform(0, 1e-9, size=200), -1.0 + rng.uniform(0, 1e-9, size=200)])
    got = tail_ref.pcm32_array(xs)
    assert np.array_equal(got, oracle.pcm32(xs))
    # a third way: the product as an exact rational, rounded once to f64 (float(Fraction) rounds correctly), truncated
    for x, g in zip(xs[::7], got[::7]):
        p = float(Fraction(M31) * Fraction(float(x)))
        assert int(g) == max(-M31 - 1, min(M31, math.trunc(p)))


def test_first_min_by_hand():
    fm = tail_ref.first_min
    assert fm([0.5, 0.25, 0.25, 0.75], 0.0, 2.0) == (1, True)               # the first of equal keys
    assert fm([0.5, 0.25, 0.25, 0.75], 1.0, 2.0) == (3, True)
    assert fm([math.nan, 0.5, math.nan], 0.0, 2.0) == (1, True)             # NaN never wins
    assert fm([math.nan, math.nan], 1.0, 2.0) == (0, False)                 # nothing below the start: index 0
    assert fm([3.5, -1.0], 1.0, 2.0) == (0, False)                          # keys 2.5 and 2.0: not < 2.0
    assert fm([math.inf, math.inf], 0.0, math.inf) == (0, False)
    assert fm([math.inf, 7.0], 0.0, math.inf) == (1, True)
    assert fm([], 1.0, 2.0) == (0, False)


@pytest.mark.parametrize("n,seed", [(1, 1), (2, 2), (65, 3), (300, 4)])
def test_refcos_chain_against_the_oracle(oracle, n, seed):
    rng = np.random.default_rng(0x7A12 + seed)
    segs = _ragged(rng, n, 12, 1, 8)
    if n > 20:
        segs[17] = segs[5].copy()
        segs[9] = np.zeros((2, 12))                  # zero norm: NaN similarity
        segs[11] = np.zeros((0, 12))                 # no frames
    sf, so = pack_segments(segs, 12)
    start = segs[5 % n].reshape(-1)
    dist = np.concatenate([[1.0, 5.0], rng.uniform(0.0, 1.6, size=30)])
    one = np.array([0, 1], dtype=np.uint64)

    def col(feats):
        f = np.asarray(feats, dtype=np.float64).reshape(-1)
        return oracle.refcos_matrix(sf, so, f, one * np.uint64(f.size // 12), 12)[:, 0]

    got_idx, got_val = tail_ref.chain(lambda i: col(segs[i]), col(start), dist, 2.0, "key")
    want_idx, want_val = oracle.chain(sf, so, 12, start, dist)
    assert np.array_equal(got_idx, want_idx)
    assert np.array_equal(got_val.view(np.uint64), want_val.view(np.uint64))
    assert got_idx[1] == 0 and got_val[1] == 2.0     # distance 5.0: every key is >= 2.0


@pytest.mark.parametrize("n,seed", [(1, 1), (2, 2), (40, 3)])
def test_dtw_chain_against_the_oracle(oracle, n, seed):
    rng = np.random.default_rng(0x7A13 + seed)
    segs = _ragged(rng, n, 13, 1, 12)
    if n > 20:
        segs[7] = np.zeros((0, 13))
    sf, so = pack_segments(segs, 13)
    start = segs[3 % n].reshape(-1)
    dist = np.concatenate([[0.0], rng.uniform(0.0, 40.0, size=9)])

    def col(feats):
        f = np.asarray(feats, dtype=np.float64).reshape(-1)
        return oracle.dtw_match_all(sf, so, f, np.array([0, f.size // 13], dtype=np.uint64), 13, want_matrix=True)[2][:, 0]

    got_idx, got_val = tail_ref.chain(lambda i: col(segs[i]), col(start), dist, math.inf, "value")
    want_idx, want_val = oracle.chain(sf, so, 13, start, dist, metric="dtw")
    assert np.array_equal(got_idx, want_idx)
    assert np.array_equal(got_val.view(np.uint64), want_val.view(np.uint64))
    assert got_idx[0] == 3 % n and got_val[0] == 0.0


def test_reconstruct_against_the_oracle(oracle):
    rng = np.random.default_rng(0x7A14)
    lens = [0, 1, 3, 255, 256, 257, 1023, 4096, 4097, 9000]
    sounds = [rng.normal(size=n) for n in lens]
    sounds[3][:4] = [-0.0, np.nan, np.inf, 5e-324]
    smp = np.concatenate(sounds)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    idx = rng.integers(0, len(lens), size=60)
    idx[:4] = [0, 3, 3, 9]
    tlen = rng.choice(lens + [2, 5000], size=60)
    tlen[1], tlen[2] = 255, 300
    ooff = np.concatenate([[0], np.cumsum(tlen)]).astype(np.uint64)
    got = tail_ref.reconstruct(smp, off, idx, ooff)
    want = oracle.reconstruct(smp, off, idx, ooff)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    for t in range(60):                               # and piece by piece against the oracle's length_fit
        piece = oracle.length_fit(sounds[idx[t]], int(tlen[t]))
        assert np.array_equal(got[int(ooff[t]):int(ooff[t + 1])].view(np.uint64), piece.view(np.uint64))
    assert tail_ref.reconstruct(smp, off, [], np.zeros(1, dtype=np.uint64)).size == 0


def test_merge_by_hand():
    nan, inf = math.nan, math.inf
    costs = np.array([[3.0, nan, nan, inf, 1.0, 4.0, nan],
                      [2.0, 5.0, nan, inf, 1.0, 8.0, 2.0],
                      [2.0, 4.0, nan, inf, nan, 7.0, nan]])
    idx = np.array([[10, 11, 12, 13, 14, 15, 16],
                    [20, 21, 22, 23, 4, 25, 26],
                    [7, 31, 32, 3, 34, 35, 36]], dtype=np.uint32)
    oi, oc = tail_ref.merge(costs, idx)
    assert oi.tolist() == [7, 31, 12, 3, 4, 15, 26]            # ties: the lowest index, whichever shard; NaN never wins
    assert oc.tolist()[:2] == [2.0, 4.0] and math.isnan(oc[2]) and oc.tolist()[3:] == [inf, 1.0, 4.0, 2.0]
    oi, oc = tail_ref.merge(costs, idx, np.array([0.0, 0.0, 0.0, 0.0, 0.0, 6.0, inf]))
    assert oi[5] == 35 and oc[5] == 7.0                        # keys 2, 2, 1 around the distance 6
    assert oi[6] == 26 and oc[6] == 2.0                        # |2 - inf| = +inf is a key, the NaNs beside it are none
    oi, oc = tail_ref.merge(costs[:, 3:4], idx[:, 3:4], np.array([inf]))
    assert oi.tolist() == [13] and oc.tolist() == [inf]        # |inf - inf|: a column of NaN keys keeps shard 0's entry


@pytest.mark.parametrize("g_n,m,seed", [(1, 7, 0), (2, 300, 1), (3, 257, 2), (8, 1000, 3), (64, 100, 4)])
def test_merge_against_the_oracle_fold(oracle, g_n, m, seed):
    """Shards ordered by index make the merge the reference's fold over the shards' entries: the oracle's top-1 of
    the [shard][target] cost matrix names the shard."""
    rng = np.random.default_rng(0x7A15 + seed)
    costs = rng.integers(0, 6, size=(g_n, m)).astype(np.float64)
    costs[rng.random((g_n, m)) < 0.1] = np.inf
    costs[rng.random((g_n, m)) < 0.05] = np.nan
    costs[0, :] = np.where(np.isfinite(costs).any(axis=0), costs[0, :], 9.0)     # (top-k reports no entry for a column without a key)
    idx = (np.arange(g_n)[:, None] * 1000 + rng.integers(0, 1000, size=(g_n, m))).astype(np.uint32)
    for dist in (None, rng.integers(0, 6, size=m).astype(np.float64)):
        oi, oc = tail_ref.merge(costs, idx, dist)
        shard, _ = oracle.topk(costs, 1, distance=dist, default_distance=0.0, fold_start=math.inf)
        shard = shard[:, 0]
        assert (shard >= 0).all()
        assert np.array_equal(oi, idx[shard, np.arange(m)])
        assert np.array_equal(oc.view(np.uint64), costs[shard, np.arange(m)].view(np.uint64))
