"""The numpy restatement of paced alignment (tests/paced_path_ref.py) against what defines it: brute-force enumeration of
every admissible pinned path on small pairs, the consequences the definition promises (DESIGN.md section 2 "Paced
alignment" (1), (2), (4)) and the shape rule.  No device."""
import numpy as np
import pytest

import paced_path_ref as ref
import paced_ref
from dtw_path_ref import bits, local_costs


def _draw(rng, k):
    """Case k of the small draw: Fb 1 ... 7, Fa 1 ... 14, dim 1 ... 3, integer features (ties) on even k, squared on k % 4 < 2."""
    fb, fa, dim = int(rng.integers(1, 8)), int(rng.integers(1, 15)), int(rng.integers(1, 4))
    if k % 2 == 0:
        a, b = rng.integers(-2, 3, (fa, dim)).astype(np.float64), rng.integers(-2, 3, (fb, dim)).astype(np.float64)
    else:
        a, b = rng.standard_normal((fa, dim)), rng.standard_normal((fb, dim))
    return a, b, k % 4 < 2


def test_small_pairs_equal_brute_force_and_keep_the_consequences():
    rng = np.random.default_rng(0xA119)
    finite = 0
    for k in range(400):
        a, b, squared = _draw(rng, k)
        cost, path, rows = ref.align(a, b, squared)
        c = local_costs(a, b, squared)
        want = ref.brute_force(c)
        assert bits(cost) == bits(want), (k, cost, want)
        assert np.isfinite(cost) == ref.feasible(a.shape[0], b.shape[0])          # finite features: a shape that fits has a path
        if not np.isfinite(cost):
            assert path.shape == (0, 2) and rows.size == 0
            continue
        finite += 1
        assert ref.admissible(rows, a.shape[0]), (k, rows)                         # (1)
        assert np.array_equal(path[:, 0], rows) and np.array_equal(path[:, 1], np.arange(b.shape[0]))
        assert bits(ref.resum(c, rows)) == bits(cost), k                           # (2)
    assert 3 * finite >= 400, finite


def test_the_recurrence_is_the_cell_by_cell_loop():
    """forward() evaluates columns at once; the definition is per cell.  Python floats, one cell at a time."""
    rng = np.random.default_rng(0xA11A)
    inf = float("inf")
    for k in range(40):
        a, b, squared = _draw(rng, k)
        c = local_costs(a, b, squared)
        fa, fb = c.shape
        N = [[inf] * fb for _ in range(fa)]
        E = [[inf] * fb for _ in range(fa)]
        N[0][0] = E[0][0] = float(c[0, 0])
        for j in range(1, fb):
            for i in range(fa):
                p = E[i - 1][j - 1] if i >= 1 else inf
                p2 = E[i - 2][j - 1] if i >= 2 else inf
                if p2 < p:
                    p = p2
                N[i][j] = float(c[i, j]) + p
                h = float(c[i, j]) + N[i][j - 1]
                E[i][j] = h if h < N[i][j] else N[i][j]
        e, _, _ = ref.forward(a, b, squared)
        assert np.array_equal(bits(e), bits([E[i][fb - 1] for i in range(fa)]))


@pytest.mark.parametrize("squared", [False, True])
def test_a_cut_paced_span_aligns_with_the_spots_cost_bits(squared):
    """(4): for every span paced_ref.spot and spot_all report, the cut re-aligned has the span's cost bits."""
    rng = np.random.default_rng(0xA11B + squared)
    spans = 0
    for k in range(24):
        fa, fb, dim = int(rng.integers(20, 201)), int(rng.integers(1, 41)), int(rng.integers(1, 4))
        if k % 2:
            a, b = rng.integers(-1, 2, (fa, dim)).astype(np.float64), rng.integers(-1, 2, (fb, dim)).astype(np.float64)
        else:
            a, b = rng.standard_normal((fa, dim)), rng.standard_normal((fb, dim))
        cost, start, end = paced_ref.spot(a, b, squared)
        count, costs, starts, ends = paced_ref.spot_all(a, b, 6, squared=squared)
        found = [(cost, start, end)] if end != paced_ref.NO_MATCH else []
        found += [(costs[m], int(starts[m]), int(ends[m])) for m in range(int(count))]
        for want, s, e in found:
            got, _, rows = ref.align(a[s:e + 1], b, squared)
            assert bits(got) == bits(want), (k, s, e, got, want)
            assert ref.admissible(rows, e + 1 - s)
            spans += 1
    assert spans >= 100


def test_the_shape_rule_at_its_edges():
    rng = np.random.default_rng(0xA11C)
    for fb in (1, 2, 3, 4, 7, 8, 33):
        lo, hi = paced_ref.span_bounds(fb)
        b = rng.standard_normal((fb, 2))
        for fa, fits in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
            cost, path, rows = ref.align(rng.standard_normal((fa, 2)), b)
            assert np.isfinite(cost) == fits == ref.feasible(fa, fb), (fa, fb)
            assert (rows.size == fb) == fits
    assert ref.align(np.zeros((0, 2)), np.zeros((3, 2)))[0] == float("inf")
    assert ref.align(np.zeros((3, 2)), np.zeros((0, 2)))[0] == float("inf")
    # with finite features the recurrence itself finds no path outside the bounds; what the rule decides is what features
    # that are not finite give there: +inf, before the recurrence could make a NaN of it
    e, _, _ = ref.forward(np.zeros((3, 1)), np.zeros((8, 1)))
    assert e[-1] == float("inf")
    assert ref.align(np.full((3, 1), np.nan), np.zeros((8, 1)))[0] == float("inf")
