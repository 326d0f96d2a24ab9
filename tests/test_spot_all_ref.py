"""tests/spot_all_ref.py (the reference ssym_dtw_spot_all is held to) against brute force on small inputs: the profile is
the least plain DTW cost over all cuts that end at each frame, its starts are the backtrace's, the greedy restated over
the set of (delta, s, i) triples gives the same list, and the five consequences the definition promises hold."""
import numpy as np
import pytest

import dtw_path_ref
import spot_all_ref
import spot_ref

NO = spot_ref.NO_MATCH


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _cases():
    """(a, b, squared) with Fa <= 24, Fb <= 6: integer-valued (real ties) and real features, squared and not."""
    rng = np.random.default_rng(0xA11)
    out = []
    for kind in ("int", "real"):
        for squared in (True, False):
            for fa, fb in ((1, 1), (1, 4), (5, 1), (6, 6), (13, 3), (24, 6), (24, 2), (17, 5)):
                dim = 2 if kind == "int" else 3
                mk = (lambda f: rng.integers(0, 3, size=(f, dim)).astype(np.float64)) if kind == "int" else \
                     (lambda f: rng.standard_normal((f, dim)))
                out.append((mk(fa), mk(fb), squared))
    return out


CASES = _cases()


def _plain(a, b, squared):
    return float(dtw_path_ref.cumulative(a, b, squared=squared)[-1, -1])


def _independent_greedy(triples, k, limit):
    """The definition over a set of (delta, s, i) triples, without arrays: sort, take, discard what overlaps."""
    alive = sorted((t for t in triples if t[0] < np.inf and t[0] <= limit), key=lambda t: (t[0], t[2]))
    out = []
    while alive and len(out) < k:
        d, s, i = alive[0]
        out.append((d, s, i))
        alive = [t for t in alive if not (t[1] <= i and t[2] >= s)]
    return out


@pytest.mark.parametrize("case", range(len(CASES)))
def test_profile_is_the_least_plain_cost_over_all_cuts_and_its_start_the_backtraces(case):
    a, b, squared = CASES[case]
    delta, s = spot_all_ref.profile(a, b, squared)
    D, _ = spot_ref.matrices(a, b, squared)
    for i in range(a.shape[0]):
        cuts = [_plain(a[lo:i + 1], b, squared) for lo in range(i + 1)]
        assert _bits(delta[i]) == _bits(min(cuts)), i
        assert int(s[i]) == spot_ref.backtrace_start(D, i)[0], i
        assert _bits(cuts[int(s[i])]) == _bits(delta[i]), i          # the start's own cut reaches the least cost


@pytest.mark.parametrize("case", range(len(CASES)))
def test_greedy_and_the_five_consequences(case):
    a, b, squared = CASES[case]
    delta, s = spot_all_ref.profile(a, b, squared)
    triples = [(float(delta[i]), int(s[i]), i) for i in range(delta.size)]
    finite = np.sort(delta[np.isfinite(delta)])
    for k in (1, 3, 8, 64):
        for limit in (None, float(finite[0]), float(finite[len(finite) // 2]), float(finite[0]) - 1.0):
            picks = spot_all_ref.select(delta, s, k, limit)
            assert picks == _independent_greedy(triples, k, np.inf if limit is None else limit)
            count, cost, start, end = spot_all_ref.spot_all(a, b, k, limit, squared)
            assert count == len(picks) and np.isinf(cost[count:]).all()
            assert (start[count:] == NO).all() and (end[count:] == NO).all()
            assert [(c, int(x), int(y)) for c, x, y in zip(cost[:count], start[:count], end[:count])] == picks
            # 2. costs do not decrease, equal costs come in ascending end
            for m in range(1, count):
                assert cost[m - 1] < cost[m] or (cost[m - 1] == cost[m] and end[m - 1] < end[m])
            # 3. spans are pairwise disjoint in frames
            taken = np.zeros(a.shape[0], dtype=int)
            for m in range(count):
                assert start[m] <= end[m]
                taken[int(start[m]):int(end[m]) + 1] += 1
            assert taken.max(initial=0) <= 1
            # 4. every cost is the plain DTW cost of its cut
            for m in range(count):
                assert _bits(cost[m]) == _bits(_plain(a[int(start[m]):int(end[m]) + 1], b, squared))
            if limit is not None:
                assert (cost[:count] <= limit).all()
        # 1. without a threshold occurrence 0 is the spot
        count, cost, start, end = spot_all_ref.spot_all(a, b, k, None, squared)
        want = spot_ref.spot(a, b, squared)
        assert count >= 1 and (_bits(cost[0]), int(start[0]), int(end[0])) == (_bits(want[0]), want[1], want[2])
    assert spot_all_ref.select(delta, s, 8, float(finite[0]) - 1.0) == []


def test_nan_is_never_a_candidate_and_nothing_gives_count_zero():
    delta = np.array([3.0, np.nan, 1.0, np.inf, 1.0, np.nan, 2.0])
    s = np.arange(7)                                                      # one-frame spans: nothing overlaps
    assert spot_all_ref.select(delta, s, 8) == [(1.0, 2, 2), (1.0, 4, 4), (2.0, 6, 6), (3.0, 0, 0)]
    assert spot_all_ref.select(delta, s, 8, 1.0) == [(1.0, 2, 2), (1.0, 4, 4)]
    assert spot_all_ref.select(np.full(4, np.nan), np.arange(4), 3) == []
    a = np.zeros((5, 2))
    a[2, 0] = np.nan                                                      # a NaN frame: the ends that pass it are NaN
    count, cost, start, end = spot_all_ref.spot_all(a, np.zeros((2, 2)), 8)
    assert count >= 1 and np.isfinite(cost[:count]).all() and not np.isnan(cost).any()
    for fa, fb in ((0, 3), (3, 0), (0, 0)):
        count, cost, start, end = spot_all_ref.spot_all(np.zeros((fa, 2)), np.zeros((fb, 2)), 4)
        assert count == 0 and np.isinf(cost).all() and (start == NO).all() and (end == NO).all()


def test_identical_plants_come_back_in_ascending_end():
    rng = np.random.default_rng(0x91A)
    tgt = rng.integers(1, 4, size=(6, 3)).astype(np.float64)
    src = rng.integers(5, 9, size=(120, 3)).astype(np.float64)            # noise that no target frame equals
    for at in (10, 50, 90):
        src[at:at + 6] = tgt
    count, cost, start, end = spot_all_ref.spot_all(src, tgt, 6, 0.0, squared=True)
    assert count == 3 and (_bits(cost[:3]) == _bits(0.0)).all()
    assert start[:3].tolist() == [10, 50, 90] and end[:3].tolist() == [15, 55, 95]
    assert np.isinf(cost[3:]).all() and (start[3:] == NO).all() and (end[3:] == NO).all()
    assert spot_all_ref.spot_all(src, tgt, 2, 0.0, squared=True)[3].tolist() == [15, 55]
    assert spot_all_ref.spot_all(src, tgt, 6, -1.0, squared=True)[0] == 0


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf"), 1e200])
def test_profile_with_a_non_finite_frame_against_the_cell_loop(value):
    """The profile is the end column of the cell-by-cell loop in the oracle's comparison order (NaN mask, then bits), and
    on finite inputs it has the bits np.minimum gave."""
    rng = np.random.default_rng(0xBAD6)
    for a, b, squared in CASES:
        delta, _ = spot_all_ref.profile(a, b, squared)
        c = dtw_path_ref.local_costs(a, b, squared)
        D = np.full((c.shape[0] + 1, c.shape[1] + 1), np.inf)
        for i in range(c.shape[0]):
            for j in range(c.shape[1]):
                D[i + 1, j + 1] = c[i, j] + (np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j]) if j else 0.0)
        assert np.array_equal(_bits(delta), _bits(D[1:, -1]))
    for squared in (True, False):
        for side, frame in (("src", 0), ("src", 7), ("src", 23), ("tgt", 0), ("tgt", 3), ("tgt", 5)):
            a, b = rng.standard_normal((24, 3)), rng.standard_normal((6, 3))
            (a if side == "src" else b)[frame, 1] = value
            delta, s = spot_all_ref.profile(a, b, squared)
            loop = dtw_path_ref.cumulative_loop(dtw_path_ref.local_costs(a, b, squared), free_start=True)[:, -1]
            assert np.array_equal(np.isnan(delta), np.isnan(loop)) and dtw_path_ref.same_floats(delta, loop)
            count, cost, start, end = spot_all_ref.spot_all(a, b, 8, None, squared)
            assert not np.isnan(cost).any() and np.isfinite(cost[:count]).all()
            if side == "tgt":
                assert count == 0 and (np.isnan(delta).all() if np.isnan(value) and frame == 5 else np.isposinf(delta).all())
            elif np.isnan(value):
                assert np.isnan(delta[frame:]).all() and (end[:count] < frame).all() and (count >= 1) == (frame > 0)
            else:
                assert np.isposinf(delta[frame]) and np.isfinite(np.delete(delta, frame)).all()
                assert frame == 23 or (end[:count] > frame).any()             # an occurrence behind the wall
