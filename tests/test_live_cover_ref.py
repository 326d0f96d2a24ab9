"""tests/live_cover_ref.py held to tests/cover_ref.py: the consequences 1 - 6 of "Live cover"  on the
restatement, without a device.  The GPU tests hold the coverer to the restatement bit for bit, so what is shown here holds
for the coverer."""
import numpy as np
import pytest

import cover_ref
import live_cover_cases as cases
import live_cover_ref as ref

INF = float("inf")
PENALTIES = (0.0, 2.0, 20.0)
CASES = cases.small_cases()


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def _same(a, b):
    """Two piece lists: sources, cuts and cost bits."""
    return [p[:3] for p in a] == [p[:3] for p in b] and _bits([p[3] for p in a]) == _bits([p[3] for p in b])


@pytest.fixture(scope="module")
def offline():
    """(case, penalty) -> [cover_ref.cover of the prefix of every length 0 ... T], from one pair of tables per prefix."""
    out = {}
    for name, (segs, x) in CASES.items():
        per = {p: [([], INF)] for p in PENALTIES}
        for n in range(1, x.shape[0] + 1):
            M, S = cover_ref.tables(segs, x[:n])
            for p in PENALTIES:
                per[p].append(cover_ref.chain(M, S, p))
        for p in PENALTIES:
            out[name, p] = per[p]
    return out


@pytest.fixture(scope="module")
def by_frame():
    """(case, penalty) -> the lane fed frame by frame: (committed pieces after every push, the flush's, the lane)."""
    out = {}
    for name, (segs, x) in CASES.items():
        for p in PENALTIES:
            out[name, p] = ref.run(segs, x, list(range(x.shape[0] + 1)), p)
    return out


@pytest.mark.parametrize("penalty", PENALTIES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_1_total_is_the_offline_total_of_every_prefix(offline, name, penalty):
    segs, x = CASES[name]
    lane = ref.Lane(segs, penalty)
    assert lane.state() == (INF, 0, 0)
    for n in range(1, x.shape[0] + 1):
        lane.push(x[n - 1:n])
        assert _bits([lane.total()]) == _bits([offline[name, penalty][n][1]]), n


@pytest.mark.parametrize("penalty", PENALTIES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_2_cuts_do_not_matter_and_commits_only_grow(by_frame, name, penalty):
    segs, x = CASES[name]
    T = x.shape[0]
    per_frame, _, _ = by_frame[name, penalty]
    after = [0]                                          # pieces committed after n frames, frame by frame
    for out in per_frame:
        after.append(after[-1] + len(out))
    every = [p for out in per_frame for p in out]
    assert [p[1] for p in every] == sorted(p[1] for p in every)
    rng = np.random.default_rng(0xC07)
    for cuts in (cases.random_cuts(rng, T, 3), cases.random_cuts(rng, T, 20), cases.even_cuts(T, 5), [0, T]):
        pushes, _, lane = ref.run(segs, x, cuts, penalty, flush=False)
        got = []
        for out, n in zip(pushes, cuts[1:]):
            got += out
            assert _same(got, every[:after[n]]), (cuts, n)
        assert lane.emitted == got


@pytest.mark.parametrize("penalty", PENALTIES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_3_what_is_committed_is_never_revised(offline, by_frame, name, penalty):
    segs, x = CASES[name]
    T = x.shape[0]
    per_frame, _, _ = by_frame[name, penalty]
    committed, k = [], []
    for out in per_frame:
        committed += out
        k.append(len(committed))
    for n in range(1, T + 1):
        mine = committed[:k[n - 1]]
        for m in range(n, T + 1):
            pieces, total = offline[name, penalty][m]
            if pieces:
                assert _same(pieces[:len(mine)], mine), (n, m)


@pytest.mark.parametrize("penalty", PENALTIES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_4_flush_equals_cover(offline, by_frame, name, penalty):
    segs, x = CASES[name]
    per_frame, flushed, lane = by_frame[name, penalty]
    pieces, total = offline[name, penalty][x.shape[0]]
    assert pieces and np.isfinite(total)
    assert _same(lane.emitted, pieces) and _bits([lane.total()]) == _bits([total])
    assert lane.state() == (total, x.shape[0], x.shape[0]) and lane.ended
    assert flushed == lane.emitted[len(lane.emitted) - len(flushed):]
    # most of the cover was committed before the flush (the uncommitted stretch itself has no hard bound)
    assert len(flushed) < len(pieces) or len(pieces) <= 2


def test_4_the_first_frames_of_shortest5_have_no_cover(offline):
    segs, x = CASES["shortest5"]
    assert min(a.shape[0] for a in segs) == 5
    lane = ref.Lane(segs, 0.0)
    lane.push(x[:2])
    assert lane.state() == (INF, 0, 0) and lane.horizon() == [-1]
    lane.push(x[2:3])
    assert np.isfinite(lane.total()) and lane.state()[1:] == (3, 0)


def test_5_piece_costs_are_the_paced_costs_of_the_cuts(by_frame):
    import paced_match_ref
    for name in ("real", "ints"):
        segs, x = CASES[name]
        lane = by_frame[name, 2.0][2]
        for s, a, e, c in lane.emitted:
            assert _bits([c]) == _bits([paced_match_ref.cost(segs[s], x[a:e + 1])])
        assert _bits([cover_ref.resum(lane.emitted, 2.0)]) == _bits([lane.total()])


@pytest.mark.parametrize("bad", [float("nan"), INF, -INF])
def test_6_a_non_finite_target_frame_ends_the_coverable_prefix(bad):
    segs, x = CASES["real"]
    x = x.copy()
    at = 47
    x[at, 1] = bad
    for cuts in (cases.even_cuts(x.shape[0], 5), list(range(x.shape[0] + 1))):
        pushes, flushed, lane = ref.run(segs, x, cuts, 2.0)
        want, total = cover_ref.cover(segs, x[:at], 2.0)
        assert want and _same(lane.emitted, want)
        assert all(p[2] < at for p in lane.emitted)
        assert lane.state() == (INF, at, at)
        # after the frame: the total is +inf at once, and nothing is committed beyond it while the pushes go on
        for n in cuts[1:]:
            if n > at:
                probe = ref.run(segs, x[:n], [0, n], 2.0, flush=False)[2]
                assert probe.total() == INF and probe.done < at


def test_6_a_source_with_a_nan_frame_is_never_chosen():
    segs, x = CASES["real"]
    segs = [a.copy() for a in segs]
    segs[2][3, 0] = float("nan")
    _, _, lane = ref.run(segs, x, cases.even_cuts(x.shape[0], 5), 0.0)
    want, total = cover_ref.cover(segs, x, 0.0)
    assert want and _same(lane.emitted, want) and all(p[0] != 2 for p in lane.emitted)


def test_the_capacity_rule():
    assert ref.capacity([]) == 1024 and ref.capacity([1024]) == 1024 and ref.capacity([1025]) == 2048
    assert ref.capacity([5, 9, 3], initial=8) == 16 and ref.capacity([40], initial=6) == 64
