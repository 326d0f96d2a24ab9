"""tests/paced_ref.py (the reference the paced entry points are held to) against brute-force enumeration of every
admissible path on small inputs, the consequences the definition promises (span bounds, the decimated, the doubled and
the tripled target), and its occurrences against the greedy restated over a set of triples."""
import itertools

import numpy as np
import pytest

import dtw_path_ref
import paced_ref
import spot_ref

NO = spot_ref.NO_MATCH


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _cases():
    """(a, b) integer-valued (sums are exact whatever their order, and ties are real), Fa <= 11, Fb <= 6."""
    rng = np.random.default_rng(0x9ACED)
    shapes = [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 4), (3, 6), (4, 2), (5, 3), (6, 6), (7, 1), (8, 5), (9, 4),
              (10, 6), (11, 6), (11, 5), (11, 2), (11, 3)]
    out = []
    for rep in range(4):
        for fa, fb in shapes:
            hi = 2 + rep                                  # {0, 1}: ties everywhere ... {0 ... 4}: fewer
            out.append((rng.integers(0, hi, size=(fa, 2)).astype(np.float64),
                        rng.integers(0, hi, size=(fb, 2)).astype(np.float64)))
    return out


CASES = _cases()
assert len(CASES) >= 50


def _paths(fa, fb):
    """Every admissible path as a tuple of source frames, one per target frame: steps of 0, 1 or 2 source frames (at most
    one frame skipped), never two steps of 0 in a row (a frame repeated at most once)."""
    for i0 in range(fa):
        for steps in itertools.product((0, 1, 2), repeat=fb - 1):
            if any(x == 0 and y == 0 for x, y in zip(steps, steps[1:])):
                continue
            rows = np.concatenate(([i0], i0 + np.cumsum(steps, dtype=np.int64))) if fb > 1 else np.array([i0])
            if rows[-1] < fa:
                yield tuple(int(r) for r in rows)


def _brute(a, b, squared):
    """{end: (least cost, the starts of the paths that reach it)} over every admissible path, summed in path order."""
    c = dtw_path_ref.local_costs(a, b, squared)
    best = {}
    for rows in _paths(a.shape[0], b.shape[0]):
        acc = c[rows[0], 0]
        for j in range(1, len(rows)):
            acc = c[rows[j], j] + acc
        end = rows[-1]
        if end not in best or acc < best[end][0]:
            best[end] = (acc, {rows[0]})
        elif acc == best[end][0]:
            best[end][1].add(rows[0])
    return best


@pytest.mark.parametrize("case", range(len(CASES)))
def test_profile_cost_end_and_start_against_every_admissible_path(case):
    a, b = CASES[case]
    fa, fb = a.shape[0], b.shape[0]
    lo, hi = paced_ref.span_bounds(fb)
    for squared in (True, False):
        brute = _brute(a, b, squared)
        delta, s = paced_ref.profile(a, b, squared)
        for i in range(fa):
            if i in brute:
                # consequence 2: the least sum in path order.  c + . is monotone, so the least of the sums is the sum
                # over the least prefix: bit for bit with the square root too
                assert _bits(delta[i]) == _bits(brute[i][0]), i
                assert int(s[i]) in brute[i][1], (i, s[i], brute[i])              # the start of a least path
                assert lo <= i - int(s[i]) + 1 <= hi                              # consequence 1, for every end
            else:
                assert np.isposinf(delta[i]), i                                   # no admissible path ends here
        cost, start, end = paced_ref.spot(a, b, squared)
        if not brute:
            assert (cost, start, end) == (float("inf"), NO, NO)
            continue
        least = min(v[0] for v in brute.values())
        assert _bits(cost) == _bits(least)
        assert end == min(i for i, v in brute.items() if v[0] == least)           # the first end that reaches it
        assert start in brute[end][1] and lo <= end - start + 1 <= hi


def test_square_root_costs_are_summed_in_path_order():
    """acc = c + acc along the path: for real features the restatement has the bits of the best path's own sum."""
    rng = np.random.default_rng(0x50F7)
    for fa, fb in ((6, 3), (9, 5), (11, 6)):
        a, b = rng.standard_normal((fa, 3)), rng.standard_normal((fb, 3))
        brute = _brute(a, b, False)
        delta, s = paced_ref.profile(a, b, False)
        for i, (cost, starts) in brute.items():
            assert _bits(delta[i]) == _bits(cost) and int(s[i]) in starts


def test_a_source_too_short_for_the_target_has_no_spot():
    b = np.zeros((5, 2))
    assert paced_ref.spot(np.zeros((2, 2)), b) == (float("inf"), NO, NO)          # 5 frames need at least 3
    assert paced_ref.spot(np.zeros((3, 2)), b) == (0.0, 0, 2)
    assert paced_ref.spot(np.zeros((1, 2)), np.zeros((2, 2))) == (0.0, 0, 0)      # Fb = 2: a single repeat
    assert paced_ref.spot(np.zeros((0, 2)), b) == (float("inf"), NO, NO)
    assert paced_ref.spot(b, np.zeros((0, 2))) == (float("inf"), NO, NO)
    assert paced_ref.spot_all(np.zeros((2, 2)), b, 3)[0] == 0


def _stretch(rng, frames, dim=3):
    """Noise no frame of which equals another: consecutive integers in the first value, large ones elsewhere."""
    x = rng.integers(100, 200, size=(frames, dim)).astype(np.float64)
    x[:, 0] = 1000.0 + 7.0 * np.arange(frames)
    return x


@pytest.mark.parametrize("fb", [1, 2, 3, 6, 7, 20])
def test_decimated_doubled_and_tripled_targets(fb):
    """Consequences 3, 4 and 5."""
    rng = np.random.default_rng(0xDEC1 + fb)
    src = _stretch(rng, 90)
    # 3. every second frame of a stretch: exactly 0.0, a span of 2 Fb - 1 frames
    tgt = src[20:20 + 2 * fb - 1:2]
    assert tgt.shape[0] == fb
    assert paced_ref.spot(src, tgt, True) == (0.0, 20, 20 + 2 * fb - 2)
    assert paced_ref.spot(src, tgt, False) == (0.0, 20, 20 + 2 * fb - 2)
    # 4. a stretch with each frame doubled: exactly 0.0, a span of Fb / 2 frames
    half = np.repeat(src[40:40 + fb], 2, axis=0)
    cost, start, end = paced_ref.spot(src, half, True)
    assert (cost, start, end) == (0.0, 40, 40 + fb - 1) and end - start + 1 == half.shape[0] // 2
    # 5. each frame tripled: more than 0 under the paced pattern, exactly 0.0 under the symmetric one
    third = np.repeat(src[40:40 + fb], 3, axis=0)
    cost, start, end = paced_ref.spot(src, third, True)
    assert cost > 0.0 and np.isfinite(cost)
    assert spot_ref.spot(src, third, True) == (0.0, 40, 40 + fb - 1)
    lo, hi = paced_ref.span_bounds(third.shape[0])
    assert lo <= end - start + 1 <= hi


def _independent_greedy(triples, k, limit):
    """The definition over a set of (delta, s, i) triples, without arrays: sort, take, discard what overlaps."""
    alive = sorted((t for t in triples if t[0] < np.inf and t[0] <= limit), key=lambda t: (t[0], t[2]))
    out = []
    while alive and len(out) < k:
        d, s, i = alive[0]
        out.append((d, s, i))
        alive = [t for t in alive if not (t[1] <= i and t[2] >= s)]
    return out


@pytest.mark.parametrize("case", range(0, len(CASES), 3))
def test_occurrences_against_the_greedy_over_brute_force_triples(case):
    a, b = CASES[case]
    fb = b.shape[0]
    lo, hi = paced_ref.span_bounds(fb)
    brute = _brute(a, b, True)
    delta, s = paced_ref.profile(a, b, True)
    # the triples from brute force: its costs, and the restatement's choice among the starts brute force allows
    triples = []
    for i, (cost, starts) in sorted(brute.items()):
        assert int(s[i]) in starts
        triples.append((float(cost), int(s[i]), i))
    finite = sorted(t[0] for t in triples)
    limits = [None] if not finite else [None, finite[0], finite[len(finite) // 2], finite[0] - 1.0]
    for k in (1, 3, 8, 64):
        for limit in limits:
            want = _independent_greedy(triples, k, np.inf if limit is None else limit)
            count, cost, start, end = paced_ref.spot_all(a, b, k, limit, True)
            assert count == len(want) and np.isinf(cost[count:]).all()
            assert (start[count:] == NO).all() and (end[count:] == NO).all()
            assert [(c, int(x), int(y)) for c, x, y in zip(cost[:count], start[:count], end[:count])] == want
            taken = np.zeros(a.shape[0], dtype=int)
            for m in range(count):
                assert lo <= int(end[m]) - int(start[m]) + 1 <= hi                # consequence 1 for spot_all's spans
                taken[int(start[m]):int(end[m]) + 1] += 1
                assert m == 0 or cost[m - 1] < cost[m] or (cost[m - 1] == cost[m] and end[m - 1] < end[m])
            assert taken.max(initial=0) <= 1
        count, cost, start, end = paced_ref.spot_all(a, b, k, None, True)
        want = paced_ref.spot(a, b, True)
        if want[2] == NO:
            assert count == 0
        else:
            assert (_bits(cost[0]), int(start[0]), int(end[0])) == (_bits(want[0]), want[1], want[2])


def test_three_plants_are_found_three_times_and_a_threshold_per_frame_stops_there():
    rng = np.random.default_rng(0x91A)
    tgt = rng.integers(1, 4, size=(6, 3)).astype(np.float64)
    src = rng.integers(5, 9, size=(120, 3)).astype(np.float64)            # noise that no target frame equals
    for at in (10, 50, 90):
        src[at:at + 6] = tgt
    count, cost, start, end = paced_ref.spot_all(src, tgt, 6, 0.0 * 6, squared=True)
    assert count == 3 and (_bits(cost[:3]) == _bits(0.0)).all()
    assert start[:3].tolist() == [10, 50, 90] and end[:3].tolist() == [15, 55, 95]
    assert np.isinf(cost[3:]).all() and (end[3:] == NO).all()


@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e200])
def test_non_finite_features_against_the_cell_loop(value):
    """The column-at-once evaluation has the cell-by-cell loop's NaN mask and bits, and nothing non-finite is reported."""
    rng = np.random.default_rng(0xBAD7)
    for squared in (True, False):
        for side, frame in (("src", 0), ("src", 7), ("src", 23), ("tgt", 0), ("tgt", 3), ("tgt", 5)):
            a, b = rng.standard_normal((24, 3)), rng.standard_normal((6, 3))
            (a if side == "src" else b)[frame, 1] = value
            delta, s = paced_ref.profile(a, b, squared)
            c = dtw_path_ref.local_costs(a, b, squared)
            inf = float("inf")
            N = [[inf] * 6 for _ in range(24)]
            E = [[(inf, -1)] * 6 for _ in range(24)]
            SN = [[-1] * 6 for _ in range(24)]
            for j in range(6):
                for i in range(24):
                    if j == 0:
                        N[i][0], SN[i][0], E[i][0] = float(c[i, 0]), i, (float(c[i, 0]), i)
                        continue
                    p = E[i - 1][j - 1] if i >= 1 else (inf, -1)
                    p2 = E[i - 2][j - 1] if i >= 2 else (inf, -1)
                    if p2[0] < p[0]:
                        p = p2
                    n, h = float(c[i, j]) + p[0], float(c[i, j]) + N[i][j - 1]
                    N[i][j], SN[i][j] = n, p[1]
                    E[i][j] = (h, SN[i][j - 1]) if h < n else (n, p[1])
            loop = np.array([E[i][5][0] for i in range(24)])
            assert dtw_path_ref.same_floats(delta, loop)
            keep = np.isfinite(loop)
            assert np.array_equal(s[keep], np.array([E[i][5][1] for i in range(24)])[keep])
            count, cost, start, end = paced_ref.spot_all(a, b, 8, None, squared)
            assert not np.isnan(cost).any() and np.isfinite(cost[:count]).all()
            one = paced_ref.spot(a, b, squared)
            assert np.isfinite(one[0]) == (one[2] != NO)
            if side == "tgt":
                assert count == 0 and one == (inf, NO, NO)
            else:
                assert count >= 1                                          # spans that avoid the frame remain
