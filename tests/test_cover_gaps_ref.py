"""tests/cover_gaps_ref.py held to the definition of the cover with gaps ("Cover with gaps") without a
device: against tests/cover_ref.py at gap_cost = +inf, against the enumeration of every tiling with gaps, and on the
consequences the contract lists."""
import numpy as np
import pytest

import cover_gaps_ref as ref
import cover_ref
import live_cover_ref
import paced_match_ref

INF = float("inf")
GAP = ref.GAP


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _real(rng, shape):
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def _same(got, want):
    (gp, gt), (wp, wt) = got, want
    assert [p[:3] for p in gp] == [p[:3] for p in wp]
    assert _bits([p[3] for p in gp]).tolist() == _bits([p[3] for p in wp]).tolist()
    assert _bits(gt) == _bits(wt)


def test_gap_inf_is_the_cover_on_the_planted_case():
    for noise in (0.0, 1e-3):
        segs, target, _ = cover_ref.planted_case(noise=noise)
        for penalty in (0.0, 2.0):
            _same(ref.cover(segs, target, penalty, INF), cover_ref.cover(segs, target, penalty))


def test_gap_inf_is_the_cover_on_random_cases():
    rng = np.random.default_rng(0x1AF0)
    covered = 0
    for case in range(50):
        src = [_real(rng, (int(rng.integers(0, 7)), 3)) for _ in range(int(rng.integers(1, 5)))]
        x = _real(rng, (int(rng.integers(0, 20)), 3))
        if case % 7 == 3 and x.shape[0]:
            x[int(rng.integers(0, x.shape[0]))] = np.nan
        penalty, squared = (0.0, 0.5)[case % 2], bool(case % 3 == 0)
        want = cover_ref.cover(src, x, penalty, squared)
        _same(ref.cover(src, x, penalty, INF, squared), want)
        covered += bool(want[0])
    assert 20 <= covered < 50


@pytest.mark.parametrize("penalty", [0.0, 0.5])
def test_total_is_the_least_over_every_tiling_with_gaps(penalty):
    rng = np.random.default_rng(0x6A75 + int(penalty * 4))
    cases = gapped = sounding = mixed = 0
    for case in range(60):
        src = [_real(rng, (int(rng.integers(1, 5)), 3)) for _ in range(int(rng.integers(1, 5)))]
        x = _real(rng, (int(rng.integers(1, 9)), 3))
        if case % 9 == 4:
            x[int(rng.integers(0, x.shape[0]))] = (np.nan, INF, -INF)[case % 3]
        squared = bool(case % 2)
        for gap_cost in (0.0, 0.5, 1.5, 3.0, INF):
            pieces, total = ref.cover(src, x, penalty, gap_cost, squared)
            want = ref.brute_force(src, x, penalty, gap_cost, squared)
            assert _bits(total) == _bits(want), (case, gap_cost, total, want)
            cases += 1
            if gap_cost < INF:
                assert pieces and np.isfinite(total)         # consequence 5: every target of T >= 1 has a cover
            if not pieces:
                assert total == INF
                continue
            assert ref.tiles(pieces, x.shape[0])
            assert _bits(ref.resum(pieces, penalty)) == _bits(total)
            for s, a, e, c in pieces:
                if s == GAP:
                    assert a == e and _bits(c) == _bits(gap_cost)
                else:
                    assert _bits(c) == _bits(paced_match_ref.cost(src[s], x[a:e + 1], squared))
            n_gap = sum(p[0] == GAP for p in pieces)
            gapped += n_gap == len(pieces)
            sounding += n_gap == 0
            mixed += 0 < n_gap < len(pieces)
    assert cases >= 100 and min(gapped, sounding, mixed) >= 20, (cases, gapped, sounding, mixed)


def test_planted_intruder_is_exactly_the_gap():
    segs, x, planted, (first, last) = ref.intruder_case()
    assert last - first + 1 == 7 and 0 < first and last < x.shape[0] - 1
    # any piece over an intruder frame costs tens per frame at least: the nearest dictionary frame is that far away
    far = min(float(np.sqrt(((a - f) ** 2).sum())) for f in x[first:last + 1] for seg in segs for a in seg)
    assert far > 50.0
    pieces, total = ref.cover(segs, x, 0.0, 1.0)
    want = [(s, a, e, 0.0) for s, a, e in planted[:3]] + [(GAP, f, f, 1.0) for f in range(first, last + 1)] + \
           [(s, a, e, 0.0) for s, a, e in planted[3:]]
    _same((pieces, total), (want, 7.0))
    assert _bits(total) == _bits(7.0) and _bits(ref.resum(pieces)) == _bits(7.0)
    assert ref.merged(pieces)[3] == (GAP, first, last, 7.0) and len(ref.merged(pieces)) == len(planted) + 1
    # without gaps the intruder is tiled by whatever fits least badly, at hundreds per frame
    assert cover_ref.cover(segs, x)[1] > 7 * 50.0


def test_one_nan_frame_is_one_gap_frame():
    segs, x, planted, at = ref.nan_case()
    assert cover_ref.cover(segs, x) == ([], INF)
    pieces, total = ref.cover(segs, x, 0.0, 1.0)
    k = [p[1] for p in planted].index(at + 1)
    want = [(s, a, e, 0.0) for s, a, e in planted[:k]] + [(GAP, at, at, 1.0)] + [(s, a, e, 0.0) for s, a, e in planted[k:]]
    _same((pieces, total), (want, 1.0))
    for bad in (INF, -INF):
        y = x.copy()
        y[at] = bad
        _same(ref.cover(segs, y, 0.0, 1.0), (want, 1.0))


def test_a_target_too_short_for_every_segment_is_all_gaps():
    segs, x = ref.short_case()
    assert min(a.shape[0] for a in segs) >= 8 and x.shape[0] == 3
    assert cover_ref.cover(segs, x) == ([], INF)
    for gap_cost in (0.5, 3.0):
        pieces, total = ref.cover(segs, x, 2.0, gap_cost)
        assert pieces == [(GAP, f, f, gap_cost) for f in range(3)]
        assert total == 3 * gap_cost


def test_a_piece_wins_a_tie_against_a_gap():
    segs, x, gap_cost, want = ref.tie_case()
    M, _ = cover_ref.tables(segs, x)
    assert M[0, 1] == 2.0 and M[0, 2] == 3.0 and M[0, 3] == 4.0 and M[2, 1] == 2.0         # 1 per frame, exactly
    _same(ref.cover(segs, x, 0.0, gap_cost), (want, 4.0))
    # a hair under the tie the gaps win everywhere, a hair over it nothing changes
    pieces, total = ref.cover(segs, x, 0.0, np.nextafter(gap_cost, 0.0))
    assert [p[0] for p in pieces] == [GAP] * 4 and total < 4.0
    _same(ref.cover(segs, x, 0.0, np.nextafter(gap_cost, 2.0)), (want, 4.0))


def test_the_live_lane_with_gaps():
    """Totals after every push, the same pieces however the frames are cut, never revised, flush = the offline cover; with
    gap_cost = +inf the lane is live_cover_ref's."""
    rng = np.random.default_rng(0x11FE)
    src = [_real(rng, (n, 3)) for n in (1, 2, 3, 5, 4)]
    x = 2.0 * _real(rng, (60, 3))
    x[23] = np.nan
    for penalty, gap_cost in ((0.0, 1.0), (0.5, 2.5)):
        offline = ref.cover(src, x, penalty, gap_cost)
        runs = []
        for cuts in ([0, 60], list(range(0, 60, 16)) + [60], list(range(61))):
            lane = ref.Lane(src, penalty, gap_cost)
            emitted = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                out = lane.push(x[a:b])
                emitted += out
                assert _bits(lane.total()) == _bits(ref.cover(src, x[:b], penalty, gap_cost)[1])
                assert lane.state()[1] == b                  # every best(e) is finite: covered = n
                assert emitted == offline[0][:len(emitted)]  # never revised: a prefix of the whole's cover
            emitted += lane.flush()
            _same((emitted, lane.total()), offline)
            runs.append(lane.emitted)
        assert runs[0] == runs[1] == runs[2]
        assert (GAP, 23, 23, gap_cost) in offline[0] and offline[0][-1][2] == 59
    per_push, flush, lane = ref.run(src, x, [0, 20, 60], 0.0, INF)
    want_push, want_flush, want_lane = live_cover_ref.run(src, x, [0, 20, 60], 0.0)
    assert (per_push, flush, lane.state()) == (want_push, want_flush, want_lane.state()) and lane.state()[1] == 23
