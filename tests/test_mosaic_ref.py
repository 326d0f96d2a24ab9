"""tests/mosaic_ref.py held to the definition of the mosaic ("Mosaic") without a GPU: consequences (1)
to (8) of the contract on the restatement, the total against an enumeration of every mosaic, against paced spotting and
against paced alignment on the cuts."""
import numpy as np
import pytest

import mosaic_ref as ref
import paced_path_ref
import paced_ref
from dtw_path_ref import local_costs

INF, NAN = float("inf"), float("nan")
GAP, NONE = ref.GAP, ref.NONE


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def one(segs, x, penalty, gap=INF, squared=False):
    """The six arrays of one target and its pieces."""
    got = ref.arrays(segs, [x], penalty, gap, squared)
    off = np.array([0, np.asarray(x).shape[0]])
    return got, ref.pieces_of(got, off, 0)


def check_contract(segs, x, penalty, gap=INF, squared=False):
    """(1) tiling and (2) the re-summation, for one target; returns (arrays, pieces)."""
    got, pieces = one(segs, x, penalty, gap, squared)
    count, total, start, src, frame, cost = got
    T = np.asarray(x).shape[0]
    if count[0] == 0:
        assert total[0] == INF and (start == NONE).all() and (src == NONE).all() and (frame == NONE).all() and (cost == INF).all()
        return got, pieces
    assert ref.tiles(start, src, frame, [np.asarray(a).shape[0] for a in segs], T)
    assert bits(ref.resum(start, src, cost, penalty)) == bits(total[0])
    for s, first, last, a, b in pieces:
        if s != GAP:
            L = b - a + 1
            assert (L - 1) // 2 + 1 <= last - first + 1 <= 2 * L - 1
    return got, pieces


def small_cases(n, seed):
    """n random small cases: up to 3 segments of 0 ... 3 frames, T <= 4, integer and real features, penalties 0 / 0.3 / 2,
    gap prices +inf / 0.7 / 1."""
    rng = np.random.default_rng(seed)
    for k in range(n):
        dim = int(rng.integers(1, 3))
        lens = [int(rng.integers(0, 4)) for _ in range(int(rng.integers(1, 4)))]
        T = int(rng.integers(0, 5))
        if k % 2:
            segs = [rng.integers(0, 3, (f, dim)).astype(np.float64) for f in lens]
            x = rng.integers(0, 3, (T, dim)).astype(np.float64)
        else:
            segs = [ref._real(rng, (f, dim)) for f in lens]
            x = ref._real(rng, (T, dim))
        yield segs, x, (0.0, 0.3, 2.0)[int(rng.integers(0, 3))], (INF, 0.7, 1.0)[int(rng.integers(0, 3))], bool(k % 3 == 0)


def test_enumeration_of_every_mosaic():
    """(3) on 400 small cases, bit for bit, with (1) and (2) on each."""
    some = 0
    for segs, x, penalty, gap, squared in small_cases(400, 0x305A):
        got, _ = check_contract(segs, x, penalty, gap, squared)
        want = ref.brute_force(segs, x, penalty, gap, squared)
        assert bits(got[1][0]) == bits(want), (segs, x, penalty, gap, squared)
        some += int(got[0][0] > 0)
    assert some > 200


def test_columns_at_once_are_the_cell_loop():
    """The restatement's columns against a cell-by-cell loop written from the definition with Python floats."""
    rng = np.random.default_rng(7)
    segs = [ref._real(rng, (5, 3)), np.zeros((0, 3)), ref._real(rng, (1, 3)), ref._real(rng, (4, 3))]
    x = ref._real(rng, (6, 3))
    x[3] = NAN
    A, seg, pos = ref.layout(segs)
    c = local_costs(A, x)
    G, T = c.shape
    for penalty, gap in ((0.0, INF), (0.3, 0.7)):
        best, arg, rep, code, _ = ref.forward(segs, x, penalty, gap)
        E, N, before = [INF] * G, [INF] * G, 0.0
        for j in range(T):
            S, newE, newN, v, a = penalty + before, [0.0] * G, [0.0] * G, INF, NONE
            for g in range(G):
                P, kind = (E[g - 1] if pos[g] >= 1 else INF), ref.DIAGONAL
                if pos[g] >= 2 and E[g - 2] < P:
                    P, kind = E[g - 2], ref.SKIP
                if not P <= S:
                    P, kind = S, ref.OPEN
                h = float(c[g, j]) + N[g] if j else INF
                newN[g] = float(c[g, j]) + P
                newE[g] = h if h < newN[g] else newN[g]
                assert bool(rep[g, j]) == (h < newN[g]) and code[g, j] == kind
                if newE[g] < v:
                    v, a = newE[g], g
            vg = gap + before
            if vg < v:
                v, a = vg, GAP
            assert bits(v) == bits(best[j]) and a == arg[j]
            E, N, before = newE, newN, v


def test_against_spotting():
    """(4): at penalty 0 without gaps the total is at most the best spot's cost; on small-integer features with the squared
    option and a penalty of 1024 the mosaic is the best spot, total == penalty + cost."""
    rng = np.random.default_rng(0x5907)
    for k in range(200):
        dim, T = int(rng.integers(1, 4)), int(rng.integers(1, 7))
        lens = [int(rng.integers(2 * T - 1, 2 * T + 6)) for _ in range(int(rng.integers(1, 4)))]
        segs, x = [ref._real(rng, (f, dim)) for f in lens], ref._real(rng, (T, dim))
        got, _ = one(segs, x, 0.0)
        assert got[1][0] <= paced_ref.spot_best(segs, x)[1]
        segs = [rng.integers(0, 4, (f, dim)).astype(np.float64) for f in lens]
        x = rng.integers(0, 4, (T, dim)).astype(np.float64)
        got, pieces = one(segs, x, 1024.0, INF, True)
        index, cost, start, end = paced_ref.spot_best(segs, x, True)
        assert pieces == [(index, start, end, 0, T - 1)] and got[1][0] == 1024.0 + cost


def piece_costs(pieces, cost):
    """acc = c(first cell); acc = c + acc over a piece's frames."""
    out = []
    for s, _, _, a, b in pieces:
        acc = float(cost[a])
        for j in range(a + 1, b + 1):
            acc = float(cost[j]) + acc
        out.append(acc)
    return out


def test_against_alignment():
    """(5): a piece's cost is at least paced alignment's for (segment span, the cut), and equal on exactly representable
    inputs."""
    rng = np.random.default_rng(0xA119)
    for k in range(60):
        exact = bool(k % 2)
        lens = [int(rng.integers(3, 12)) for _ in range(3)]
        T = int(rng.integers(2, 14))
        if exact:
            segs, x = [rng.integers(0, 4, (f, 2)).astype(np.float64) for f in lens], rng.integers(0, 4, (T, 2)).astype(np.float64)
        else:
            segs, x = [ref._real(rng, (f, 2)) for f in lens], ref._real(rng, (T, 2))
        got, pieces = one(segs, x, 0.5, INF, exact)
        for (s, first, last, a, b), mine in zip(pieces, piece_costs(pieces, got[5])):
            alone = paced_path_ref.align(segs[s][first:last + 1], x[a:b + 1], exact)[0]
            assert mine >= alone
            if exact:
                assert mine == alone


def test_non_finite_features():
    """(6): a NaN source frame is never on a path; a NaN target frame means no mosaic without gaps and exactly one gap frame
    with a finite gap_cost, with pieces on both sides."""
    recs, x, pieces = ref.planted_case()
    bad = [a.copy() for a in recs]
    bad[1][9] = NAN                                          # inside the first planted span
    bad[2][0, 3] = INF
    got, found = check_contract(bad, x, 1.0)
    assert got[0][0] > 0 and np.isfinite(got[1][0])
    assert not any(int(s) == 1 and int(f) == 9 for s, f in zip(got[3], got[4]))
    assert not any(int(s) == 2 and int(f) == 0 for s, f in zip(got[3], got[4]))
    y = x.copy()
    y[12, 5] = NAN
    got, _ = check_contract(recs, y, 1.0)
    assert got[0][0] == 0 and got[1][0] == INF
    got, found = check_contract(recs, y, 1.0, 1.5)
    gaps = [p for p in found if p[0] == GAP]
    assert gaps == [(GAP, NONE, NONE, 12, 12)] and found[0][0] != GAP and found[-1][0] != GAP
    assert bits(got[5][12]) == bits(1.5)


@pytest.mark.parametrize("noise", [0.0, 1e-3])
def test_planted(noise):
    """(7): the planted spans come back, cut at the joins; without noise the total is exactly penalty x pieces."""
    recs, x, pieces = ref.planted_case(noise)
    got, found = check_contract(recs, x, 1.0)
    assert found == pieces
    if not noise:
        assert got[1][0] == 3.0 and (got[5] == 0.0).all()


def test_planted_at_penalty_zero_is_frame_wise():
    """At penalty 0 the optimum is frame-wise: N wins its tie with H, so the doubled span comes back in fragments."""
    recs, x, pieces = ref.planted_case()
    got, found = check_contract(recs, x, 0.0)
    assert got[1][0] == 0.0 and len(found) > len(pieces)


def test_gaps():
    """(8): with a finite gap_cost every target has a mosaic; the intruder's frames, and only they, are gap frames."""
    recs, x, pieces, (first, last) = ref.intruder_case()
    got, found = check_contract(recs, x, 1.0, 1.5)
    assert got[1][0] == 8.0
    assert found == [pieces[0]] + [(GAP, NONE, NONE, j, j) for j in range(first, last + 1)] + [pieces[1]]
    far = [np.full((3, 2), 1e6)]
    got, found = check_contract(far, np.zeros((5, 2)), 1.0, 0.25)
    assert got[0][0] == 5 and got[1][0] == 1.25 and all(p[0] == GAP for p in found)
    assert check_contract(far, np.zeros((0, 2)), 1.0, 0.25)[0][0][0] == 0


def test_boundary():
    """A piece never crosses a segment boundary."""
    segs, x, pieces = ref.boundary_case()
    for penalty in (0.3, 20.0):
        got, found = check_contract(segs, x, penalty)
        assert found == pieces and bits(got[1][0]) == bits(penalty + penalty)


def test_ties():
    """Integer features: the smallest g wins a tie, a tie continues the piece, N keeps its tie with H, a piece keeps its tie
    with a gap."""
    segs = [np.zeros((2, 1)), np.zeros((3, 1))]
    got, found = check_contract(segs, np.ones((4, 1)), 0.0, 1.0)
    assert got[1][0] == 4.0 and all(p[0] != GAP for p in found)
    assert found[0][:2] == (0, 0)
    got, found = check_contract(segs, np.ones((4, 1)), 1.0, 1.0)          # a gap frame is cheaper than opening a piece
    assert got[1][0] == 4.0 and all(p[0] == GAP for p in found)
