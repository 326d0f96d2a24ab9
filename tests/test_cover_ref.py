"""tests/cover_ref.py held to the definition of the cover ("Cover") without a device: against the
enumeration of every tiling, against paced_match_ref on every cut, and on the consequences the contract lists."""
import numpy as np
import pytest

import cover_ref
import paced_match_ref

INF = float("inf")


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _real(rng, shape):
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def _tiles(pieces, T):
    at = 0
    for _, start, end, _ in pieces:
        assert start == at and end >= start
        at = end + 1
    assert at == T


@pytest.mark.parametrize("penalty", [0.0, 0.75])
def test_total_is_the_least_over_every_tiling(penalty):
    rng = np.random.default_rng(0x7117 + int(penalty * 4))
    covered = 0
    for case in range(60):
        src = [_real(rng, (int(rng.integers(1, 5)), 3)) for _ in range(3)]
        x = _real(rng, (int(rng.integers(1, 8)), 3))
        squared = bool(case % 2)
        pieces, total = cover_ref.cover(src, x, penalty, squared)
        want = cover_ref.brute_force(src, x, penalty, squared)
        assert _bits(total) == _bits(want), (case, total, want)
        if pieces:
            covered += 1
            _tiles(pieces, x.shape[0])
            assert _bits(cover_ref.resum(pieces, penalty)) == _bits(total)
            for s, a, e, c in pieces:
                assert _bits(c) == _bits(paced_match_ref.cost(src[s], x[a:e + 1], squared))
        else:
            assert total == INF
    assert covered >= 40


def test_one_forward_per_start_gives_every_window():
    """w(n, s, L) from one pass per (n, s) against paced_match_ref.cost on every cut, and the tables against their fold."""
    rng = np.random.default_rng(0x0F0D)
    src = [_real(rng, (n, 5)) for n in (1, 2, 3, 4, 7, 0, 6)]
    x = _real(rng, (13, 5))
    triples = 0
    for squared in (False, True):
        M, S = cover_ref.tables(src, x, squared)
        assert M.shape == (13, 14)
        want_m = np.full(M.shape, INF)
        want_s = np.full(M.shape, cover_ref.NONE, dtype=np.uint32)
        for n, a in enumerate(src):
            for s in range(x.shape[0]):
                w = cover_ref.window_costs(a, x, s, squared)
                assert w.size == min(2 * a.shape[0], x.shape[0] - s)
                for L in range(1, w.size + 1):
                    assert _bits(w[L - 1]) == _bits(paced_match_ref.cost(a, x[s:s + L], squared)), (n, s, L)
                    triples += 1
                    if w[L - 1] < want_m[s, L - 1]:
                        want_m[s, L - 1], want_s[s, L - 1] = w[L - 1], n
        assert (_bits(M) == _bits(want_m)).all() and (S == want_s).all()
    assert triples >= 500


@pytest.fixture(scope="module")
def planted():
    segs, target, pieces = cover_ref.planted_case()
    return segs, target, pieces, cover_ref.cover(segs, target)


def test_planted_exact_copies_cost_zero_and_cut_at_the_joins(planted):
    segs, target, want, (pieces, total) = planted
    assert _bits(total) == _bits(0.0)
    assert [(s, a, e) for s, a, e, _ in pieces] == want
    assert all(_bits(c) == _bits(0.0) for _, _, _, c in pieces)
    _tiles(pieces, target.shape[0])
    assert _bits(cover_ref.resum(pieces)) == _bits(total)


def test_planted_with_noise_keeps_pieces_and_cuts():
    segs, target, want = cover_ref.planted_case(noise=1e-3)
    pieces, total = cover_ref.cover(segs, target)
    assert [(s, a, e) for s, a, e, _ in pieces] == want
    assert 0.0 < total < 1.0
    assert _bits(cover_ref.resum(pieces)) == _bits(total)


def test_ties_lower_source_then_shorter_last_piece(planted):
    segs, target, want, _ = planted
    # a second copy of every segment behind the first: the lower index still wins
    pieces, total = cover_ref.cover(segs + segs, target)
    assert [(s, a, e) for s, a, e, _ in pieces] == want and total == 0.0
    # ... and in front of it: the copies win now
    pieces, _ = cover_ref.cover([s.copy() for s in segs] + segs, target)
    assert [s for s, _, _, _ in pieces] == [s for s, _, _ in want]
    # one 1-frame segment v against v v v v: every tiling into pieces of 1 or 2 frames costs exactly 0; the shorter last
    # piece wins at every step
    v = np.array([[1.0, 2.0, 3.0]])
    pieces, total = cover_ref.cover([v], np.repeat(v, 4, axis=0))
    assert [(a, e) for _, a, e, _ in pieces] == [(0, 0), (1, 1), (2, 2), (3, 3)] and total == 0.0
    # a penalty per piece breaks the tie the other way
    pieces, total = cover_ref.cover([v], np.repeat(v, 4, axis=0), 1.0)
    assert [(a, e) for _, a, e, _ in pieces] == [(0, 1), (2, 3)] and total == 2.0


def test_non_finite_features(planted):
    segs, target, want, (pieces, total) = planted
    for bad in (np.nan, np.inf, -np.inf):
        x = target.copy()
        x[57, 4] = bad
        assert cover_ref.cover(segs, x) == ([], INF)
    # a segment with a NaN frame is never chosen: the cover is the one of the dictionary with that segment empty
    rng = np.random.default_rng(5)
    x = _real(rng, (40, 13))
    for n in (0, 3, 9):
        broken = [s.copy() for s in segs]
        broken[n][broken[n].shape[0] // 2, 2] = np.nan
        emptied = [s if k != n else s[:0] for k, s in enumerate(segs)]
        got, want_cover = cover_ref.cover(broken, x), cover_ref.cover(emptied, x)
        assert got[0] == want_cover[0] and _bits(got[1]) == _bits(want_cover[1])
        assert n not in [s for s, _, _, _ in got[0]] and got[0]


def test_penalty_trades_fit_for_fewer_pieces(planted):
    segs = planted[0]
    x = _real(np.random.default_rng(40), (40, 13))
    counts, fits = [], []
    for penalty in (0.0, 2.0, 20.0):
        pieces, total = cover_ref.cover(segs, x, penalty)
        _tiles(pieces, 40)
        assert _bits(cover_ref.resum(pieces, penalty)) == _bits(total)
        counts.append(len(pieces))
        fits.append(sum(c for _, _, _, c in pieces))
    assert counts[0] > counts[1] > counts[2] >= 1
    assert fits[0] <= fits[1] <= fits[2]


def test_shapes_without_a_cover_and_the_shortest_source():
    rng = np.random.default_rng(11)
    # a 1-frame target against a 3-frame segment: the segment covers windows of 2 ... 6 frames only
    assert cover_ref.cover([_real(rng, (3, 3))], _real(rng, (1, 3))) == ([], INF)
    assert cover_ref.cover([_real(rng, (3, 3))], np.zeros((0, 3))) == ([], INF)
    # a 4-frame target against a single 1-frame segment: windows of 1 or 2 frames only, so pieces of 1 or 2 frames; in real
    # numbers every tiling sums the same four distances, so the rounding of the additions decides between them
    seen = set()
    for seed in range(40):
        rng = np.random.default_rng(seed)
        a, x = _real(rng, (1, 3)), _real(rng, (4, 3))
        pieces, total = cover_ref.cover([a], x)
        _tiles(pieces, 4)
        lens = tuple(e - s + 1 for _, s, e, _ in pieces)
        assert set(lens) <= {1, 2}
        assert _bits(total) == _bits(cover_ref.brute_force([a], x))
        seen.add(lens)
    assert (1, 1, 2) in seen
    # and against a single 2-frame segment (windows of 2 ... 4 frames): a 5-frame target is 2 + 3 or 3 + 2, never 1 + 4
    pieces, _ = cover_ref.cover([_real(rng, (2, 3))], _real(rng, (5, 3)))
    assert sorted(e - s + 1 for _, s, e, _ in pieces) == [2, 3]


def test_arrays_layout():
    rng = np.random.default_rng(3)
    src = [_real(rng, (n, 4)) for n in (2, 3, 5)]
    tg = [_real(rng, (9, 4)), np.zeros((0, 4)), _real(rng, (1, 4)), _real(rng, (6, 4))]
    count, total, s, a, e, c = cover_ref.arrays(src, tg, 0.5)
    off = [0, 9, 9, 10, 16]
    for t, x in enumerate(tg):
        pieces, tot = cover_ref.cover(src, x, 0.5)
        assert count[t] == len(pieces) and _bits(total[t]) == _bits(tot)
        k = off[t] + len(pieces)
        assert [(int(s[i]), int(a[i]), int(e[i]), float(c[i])) for i in range(off[t], k)] == pieces
        assert (s[k:off[t + 1]] == cover_ref.NONE).all() and (a[k:off[t + 1]] == cover_ref.NONE).all()
        assert (e[k:off[t + 1]] == cover_ref.NONE).all() and (c[k:off[t + 1]] == INF).all()
    assert count[1] == 0 and count[2] == 0 and total[1] == INF
