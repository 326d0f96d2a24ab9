"""tests/count_cases.py holds what the GPU tests of "more tasks than the grid has workgroups" rely on: the two targets a
workgroup visits in a row run through every ordered pair of kinds, the outcomes are mixed, the long targets pass the ring,
the ties fall across the wave's lanes, and the big call stays inside the cover's scratch.  No GPU."""
import numpy as np
import pytest

import count_cases as cc
import cover_ref
import live_cover_ref
import paced_match_ref

ALL_PAIRS = {(i, j) for i in range(8) for j in range(8)}


def _pairs(kinds, stride, m):
    """The kinds of the first two targets of workgroups 0 ... 63 of a grid of `stride` workgroups over m targets."""
    out = set()
    for b in range(64):
        seen = cc.visits(b, stride, m)
        assert seen[:2] == [b, b + stride]
        out.add((kinds[seen[0]], kinds[seen[1]]))
    return out


@pytest.fixture(scope="module")
def paced():
    return cc.paced_case()


@pytest.fixture(scope="module")
def cover():
    return cc.cover_case(256)


def test_paced_targets_enumerate_the_pairs_of_kinds(paced):
    assert paced.m == 65600 == len(paced.ids) and len(paced.kinds) == 128
    assert _pairs(paced.kinds, cc.PACED_STRIDE, paced.m) == ALL_PAIRS
    for t, k in paced.kinds.items():
        assert paced.tgt[t].shape == (cc.PACED_KIND_FRAMES[k], 2)
    assert len(paced.uniq) == cc.POOL + 128 and paced.frames[:cc.POOL].max() <= 6
    assert [a.shape[0] for a in paced.src] == [1, 2, 3, 5, 9, 30, 63, 64, 70]


def test_paced_outcomes_are_mixed(paced):
    (want,) = cc.gather((paced.want_u,), paced.ids)
    assert want.shape == (9, 65600)
    idx, cost = cc.gather(paced_match_ref.fold(paced.want_u), paced.ids)
    second = np.arange(cc.PACED_STRIDE, cc.PACED_STRIDE + 64)
    assert np.isfinite(cost[second]).any() and np.isposinf(cost[second]).any()
    assert np.isfinite(cost[:64]).any() and np.isposinf(cost[:64]).any()
    assert (idx[second] != idx[:64]).sum() >= 16                       # another winner than the target before it
    # finite after +inf and +inf after finite, in one workgroup
    assert (np.isposinf(cost[:64]) & np.isfinite(cost[second])).any() and (np.isfinite(cost[:64]) & np.isposinf(cost[second])).any()
    # every source wins somewhere among the drawn targets, and the pool's targets have winners too
    assert set(idx[list(paced.kinds)].tolist()) >= {0, 1, 2, 5, 6, 7, 8} and np.isfinite(cost[64:cc.PACED_STRIDE]).any()
    # with distances the fold picks other sources than without
    didx, _ = cc.gather(paced_match_ref.fold(paced.want_u, paced.distance_u, 7), paced.ids)
    assert (didx[second] - 7 != idx[second]).any()


def test_the_clamp_case_puts_equal_sources_on_either_side_of_1023():
    src, tgt = cc.clamp_case()
    assert len(src) == 1030 and {a.shape[0] for a in src} == {1, 2, 3}
    block = -(-1030 // 1023)                                           # what the clamp makes of one source per block
    assert block == 2 and 1021 // block < 1023 // block < 1025 // block
    want = paced_match_ref.matrix(src, tgt)
    assert want[1021, 0] == 0.0 and want[1025, 0] == 0.0 and (want[:, 0] == 0.0).sum() == 2
    idx, cost = paced_match_ref.fold(want)
    assert idx[0] == 1021 and np.isfinite(cost).all()


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_cover_targets_enumerate_the_pairs_for_both_strides(cus):
    g = cc.chain_stride(cus)
    kinds = cc.drawn_kinds([g, cc.FORWARD_STRIDE])
    assert len(kinds) == 192 and max(kinds) == cc.COVER_M - 1 == 65598
    assert _pairs(kinds, g, cc.COVER_M) == ALL_PAIRS                   # cover_chain_kernel: min(M, 8 cus) workgroups
    assert _pairs(kinds, cc.FORWARD_STRIDE, cc.COVER_M) == ALL_PAIRS   # cover_forward_kernel: grid z


def test_the_cover_case_fits_the_scratch_and_passes_the_ring(cover):
    assert cover.m == 65599 and [a.shape[0] for a in cover.src] == [1, 3, 2, 0, 3]
    W = live_cover_ref.width(cover.src)
    assert W == 6
    # the drawn targets' frames do not depend on the CU count, the pool's do not exceed 6 each
    assert cc.cover_scratch_bytes(cover.total_frames(), W) < cc.COVER_SCRATCH // 8
    assert cc.cover_scratch_bytes(cover.frames[cc.POOL:].sum() + 6 * cover.m, W) < cc.COVER_SCRATCH
    for t, k in cover.kinds.items():
        assert cover.tgt[t].shape == (cc.COVER_KIND_FRAMES[k], 2)
        assert np.isnan(cover.tgt[t]).any() == (k == cc.COVER_NAN_KIND)
    count, total, src, start, end, cost = cc.gather_cover(cover.want_u, cover.frames, cover.ids)
    off = np.concatenate([[0], np.cumsum(cover.frames[cover.ids])])
    assert src.size == off[-1] == cover.total_frames()
    long = [t for t, k in cover.kinds.items() if cc.COVER_KIND_FRAMES[k] == 600]
    assert len(long) == 24
    for t in long:
        ends = end[off[t]:off[t] + count[t]]
        assert count[t] > 100 and ends[-1] == 599 and (ends > cc.COVER_RING).sum() > 10
    # the gathered arrays are the restatement's own for a stretch that holds drawn and pooled targets
    some = list(range(60, 70))
    direct = cover_ref.arrays(cover.src, [cover.tgt[t] for t in some], cc.COVER_PENALTY)
    lo, hi = off[some[0]], off[some[-1] + 1]
    for got, want in zip((count[some], total[some], src[lo:hi], start[lo:hi], end[lo:hi], cost[lo:hi]), direct):
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("stride", ["chain", "forward"])
def test_cover_outcomes_are_mixed(cover, stride):
    stride = cc.chain_stride(256) if stride == "chain" else cc.FORWARD_STRIDE
    count, total = cover.want_u[0][cover.ids], cover.want_u[1][cover.ids]
    first, second = np.arange(64), np.arange(stride, stride + 64)
    kinds = np.array([cover.kinds[t] for t in first])
    assert (count[first][kinds == cc.COVER_NAN_KIND] == 0).all() and np.isposinf(total[first][kinds == cc.COVER_NAN_KIND]).all()
    # after a target without a cover, the next target of the same workgroup has one -- and the other way round
    assert ((count[first] == 0) & (count[second] > 0)).sum() >= 12 and ((count[first] > 0) & (count[second] == 0)).sum() >= 12
    # after a target that passed the ring (ring[0] then holds best(511), not best(-1)) comes one with a cover
    assert ((cover.frames[cover.ids[first]] == 600) & (count[second] > 0)).sum() >= 6
    assert np.isfinite(total[second]).any() and (count[64:stride] > 0).any()


def test_the_long_targets():
    segs, tgt = cc.long_case()
    assert [x.shape[0] for x in tgt] == [511, 512, 513, 1300] and max(a.shape[0] for a in segs) == 8


@pytest.mark.parametrize("fmax", [40, 128])
def test_ties_fall_across_the_waves_lanes(fmax):
    segs, x, penalty = cc.tie_case(fmax)
    assert live_cover_ref.width(segs) == 2 * fmax > 64 and penalty > 0
    M, S = cover_ref.tables(segs, x)
    tied = cc.tied_lengths(M, S, penalty)
    pieces, total = cover_ref.chain(M, S, penalty)
    # tied_lengths restates the chain: the first tied length is the one the chain took
    assert np.isfinite(total) and all(tied[e][0] == e - a + 1 for _, a, e, _ in pieces)
    across, upper = cc.cross_lane_ties(tied)
    assert len(across) > 20 and len(upper) > 5
    # ... and the cover itself goes through such ends: a wrong pick there changes the pieces, not only a back-pointer
    ends = {e for _, _, e, _ in pieces}
    assert ends & set(upper), (sorted(ends), upper[:10])


def test_the_lane_schedule():
    s = cc.Schedule()
    assert s.pushes == 25 and len(s.never) == 12 and not s.never & {256, 299}
    fed = np.array([[c.shape[0] > 0 for c in op[1]] for op in s.ops if op[0] == "push"])
    assert fed.shape == (25, 300) and 0.35 < fed.mean() < 0.55
    assert fed[:, 256].sum() >= 18 and fed[:, 299].sum() >= 18 and not fed[:, sorted(s.never)].any()
    sizes = {c.shape[0] for op in s.ops if op[0] == "push" for c in op[1]}
    assert {1, 15, 16, 17, 35} <= sizes and max(sizes) == 2 * 16 + 3
    flushed = [op[1] for op in s.ops if op[0] == "flush"]
    reset = [op[1] for op in s.ops if op[0] == "reset"]
    assert len(flushed) >= 20 and 8 <= len(reset) < len(flushed) and len(s.ended) >= 8
    assert any(l >= 256 for l in flushed) and any(l < 256 for l in flushed)
    # a lane that was reset is fed again afterwards
    again = 0
    for i, op in enumerate(s.ops):
        if op[0] == "reset" and op[1] not in s.never:
            again += any(o[0] == "push" and o[1][op[1]].shape[0] for o in s.ops[i:])
    assert again >= 6
