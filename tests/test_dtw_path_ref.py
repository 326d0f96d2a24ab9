"""The numpy restatement of the DTW alignment (tests/dtw_path_ref.py) held to the oracle and to hand-worked cases
(CPU only)."""
import numpy as np
import pytest

import dtw_path_ref as ref


def _col(values):
    return np.asarray(values, dtype=np.float64)[:, None]


def _pairs(seed, n, dim, lo=1, hi=24):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        fa, fb = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        yield rng.standard_normal((fa, dim)), rng.standard_normal((fb, dim))


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("band", [-1, 0, 3, 8])
def test_cost_equals_the_oracle_bit_for_bit(oracle, band, squared):
    import oracle as o
    finite = 0
    for a, b in _pairs(0xA11 + band + 100 * squared, 30, 12):
        if band >= 0 and finite < 20:                 # most banded pairs reachable: |Fa - Fb| <= band
            b = b[:max(1, min(b.shape[0], a.shape[0] + band))]
            if a.shape[0] - b.shape[0] > band:
                a = a[:b.shape[0] + band]
        cost, path, fmap = ref.align(a, b, band, squared)
        want = oracle.dtw(a.reshape(-1), b.reshape(-1), 12, band, squared)
        assert np.float64(cost).tobytes() == np.float64(want).tobytes() or (np.isinf(cost) and np.isinf(want))
        assert np.float64(cost).tobytes() == np.float64(o.np_dtw(a, b, band, squared)).tobytes()
        finite += int(np.isfinite(cost))
    assert finite >= 10


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("band", [-1, 2, 6])
def test_path_is_valid_and_resums_to_the_cost_bit_for_bit(band, squared):
    seen = 0
    for a, b in _pairs(0xB22 + band + 100 * squared, 40, 5):
        cost, path, fmap = ref.align(a, b, band, squared)
        if not np.isfinite(cost):
            assert path.shape == (0, 2) and fmap.size == 0
            continue
        seen += 1
        ref.check_path(path, a.shape[0], b.shape[0], band)
        assert ref.resum(a, b, path, squared) == cost
        assert fmap[0] == 0 and (np.diff(fmap) >= 0).all() and fmap.size == b.shape[0]
        for j in range(b.shape[0]):
            assert fmap[j] == path[path[:, 1] == j, 0].min()
    assert seen >= 8


# Hand-made answers: one value per frame, squared cost, so c(i,j) = (a_i - b_j)^2 and every D can be checked by eye.

def test_three_way_tie_takes_the_diagonal():
    # digital silence: every c and every D is 0; at (1,1) dg = up = lf = 0
    cost, path, fmap = ref.align(_col([0, 0]), _col([0, 0]), squared=True)
    assert cost == 0.0 and path.tolist() == [[0, 0], [1, 1]] and fmap.tolist() == [0, 1]
    cost, path, fmap = ref.align(np.zeros((4, 3)), np.zeros((6, 3)))
    # the shortest path through the plateau: diagonal while both indices are positive, then along row 0
    assert path.tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4], [3, 5]] and fmap.tolist() == [0, 0, 0, 1, 2, 3]


def test_diagonal_wins_a_tie_with_up():
    # c = [[1,0],[1,0]]: D = [[1,1],[2,1]]; at (1,1) dg = D(0,0) = 1 = up = D(0,1) < lf = D(1,0) = 2
    D = ref.cumulative(_col([0, 0]), _col([1, 0]), squared=True)
    assert D.tolist() == [[1, 1], [2, 1]]
    cost, path, fmap = ref.align(_col([0, 0]), _col([1, 0]), squared=True)
    assert cost == 1.0 and path.tolist() == [[0, 0], [1, 1]] and fmap.tolist() == [0, 1]


def test_up_wins_a_tie_with_left():
    # a = 0 1 0, b = 1 0 1: c = [[1,0,1],[0,1,0],[1,0,1]], D = [[1,1,2],[1,2,1],[2,1,2]].  At (2,2) dg = 2 and
    # up = D(1,2) = 1 = lf = D(2,1): up.  At (1,2) dg = D(0,1) = 1 < up = lf = 2: diagonal.  (0,1) is in row 0: left.
    D = ref.cumulative(_col([0, 1, 0]), _col([1, 0, 1]), squared=True)
    assert D.tolist() == [[1, 1, 2], [1, 2, 1], [2, 1, 2]]
    cost, path, fmap, ties = ref.align(_col([0, 1, 0]), _col([1, 0, 1]), squared=True, want_ties=True)
    assert cost == 2.0 and path.tolist() == [[0, 0], [0, 1], [1, 2], [2, 2]] and fmap.tolist() == [0, 0, 1]
    assert ties == 1


def test_first_row_and_first_column():
    cost, path, fmap = ref.align(_col([0]), _col([0, 1, 2]), squared=True)
    assert cost == 5.0 and path.tolist() == [[0, 0], [0, 1], [0, 2]] and fmap.tolist() == [0, 0, 0]
    cost, path, fmap = ref.align(_col([0, 1, 2]), _col([0]), squared=True)
    assert cost == 5.0 and path.tolist() == [[0, 0], [1, 0], [2, 0]] and fmap.tolist() == [0]
    cost, path, fmap = ref.align(_col([0, 3]), _col([0]), squared=False)
    assert cost == 3.0 and path.tolist() == [[0, 0], [1, 0]]


def test_one_frame_on_both_sides():
    cost, path, fmap = ref.align(_col([2]), _col([-1]), squared=True)
    assert cost == 9.0 and path.tolist() == [[0, 0]] and fmap.tolist() == [0]
    cost, path, fmap = ref.align(_col([2]), _col([-1]), squared=False)
    assert cost == 3.0 and path.tolist() == [[0, 0]]


def test_band_that_cuts_the_end_cell_and_empty_segments():
    cost, path, fmap = ref.align(_col([0]), _col([0, 0, 0]), band=1, squared=True)     # (0,2): |0 - 2| > 1
    assert np.isinf(cost) and path.shape == (0, 2) and fmap.size == 0
    cost, path, fmap = ref.align(_col([0, 0, 0]), _col([0, 0, 0]), band=0, squared=True)
    assert cost == 0.0 and path.tolist() == [[0, 0], [1, 1], [2, 2]]
    cost, path, fmap = ref.align(np.zeros((0, 1)), _col([0, 0]))
    assert np.isinf(cost) and path.shape == (0, 2) and fmap.size == 0
    cost, path, fmap = ref.align(_col([0, 0]), np.zeros((0, 1)))
    assert np.isinf(cost) and path.shape == (0, 2)


def test_band_keeps_the_path_inside():
    # a ramp against a delayed ramp wants to run along row 0 first; r = 1 allows one step of it
    a, b = _col([0, 1, 2, 3]), _col([0, 0, 0, 1, 2])
    _, free, _ = ref.align(a, b, squared=True)
    assert free.tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4], [3, 4]]
    cost, path, _ = ref.align(a, b, band=1, squared=True)
    ref.check_path(path, 4, 5, 1)
    assert cost == ref.resum(a, b, path, True) and cost > 1.0


# ---- the comparison order of min3, which only a NaN can tell apart ------------------------------------------------------

POISON = [float("nan"), float("inf"), float("-inf"), 1e200]          # 1e200: the squared difference overflows to +inf


def _cumulative_np_minimum(a, b, band=-1, squared=False):
    """cumulative() as it was before min3: np.minimum, which is order-free and returns NaN for any NaN operand."""
    c = ref.local_costs(a, b, squared)
    fa, fb = c.shape
    D = np.full((fa + 1, fb + 1), np.inf)
    for s in range(fa + fb - 1):
        i = np.arange(max(0, s - fb + 1), min(fa - 1, s) + 1)
        j = s - i
        if band >= 0:
            keep = np.abs(i - j) <= band
            i, j = i[keep], j[keep]
            if i.size == 0:
                continue
        best = np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j])
        if s == 0:
            best = np.zeros(1)
        D[i + 1, j + 1] = c[i, j] + best
    return D[1:, 1:]


def poisoned(rng, fa, fb, dim, value, side, frame):
    """A real-valued pair with one poisoned value: in source frame `frame` (side "src") or target frame `frame`."""
    a, b = rng.standard_normal((fa, dim)), rng.standard_normal((fb, dim))
    (a if side == "src" else b)[frame, int(rng.integers(0, dim))] = value
    return a, b


def test_min3_orders_its_comparisons_as_the_oracle_does():
    nan, inf = float("nan"), float("inf")
    up, lf, dg = np.array([nan, 1.0, 1.0, nan, 2.0, inf]), np.array([1.0, nan, 2.0, nan, nan, nan]), np.array([2.0, 2.0, nan, 0.0, 3.0, nan])
    got = ref.min3(up, lf, dg)
    assert ref.same_floats(got, [nan, 1.0, 1.0, nan, 2.0, inf])       # a NaN up stays; a NaN lf or dg is passed over
    assert np.isnan(np.minimum(np.minimum(up, lf), dg)).all()         # what np.minimum makes of the same operands
    assert ref.same_floats([nan, 1.0, -0.0], [-nan, 1.0, -0.0]) and not ref.same_floats([0.0], [-0.0])
    assert not ref.same_floats([nan, 1.0], [1.0, nan]) and not ref.same_floats([1.0], [1.0, 1.0])


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("band", [-1, 0, 3, 8])
def test_finite_inputs_give_the_bits_np_minimum_gave(band, squared):
    for a, b in _pairs(0xA11 + band + 100 * squared, 30, 12):
        assert np.array_equal(ref.bits(ref.cumulative(a, b, band, squared)), ref.bits(_cumulative_np_minimum(a, b, band, squared)))


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("value", POISON)
def test_non_finite_inputs_against_the_cell_loop_and_the_oracle(oracle, value, squared):
    rng = np.random.default_rng(0xBAD + squared)
    differs = nans = infs = 0
    for side, frame in (("src", 0), ("src", 4), ("src", 9), ("tgt", 0), ("tgt", 2), ("tgt", 5)):
        a, b = poisoned(rng, 10, 6, 3, value, side, frame)
        D = ref.cumulative(a, b, squared=squared)
        loop = ref.cumulative_loop(ref.local_costs(a, b, squared))
        assert np.array_equal(np.isnan(D), np.isnan(loop)), (side, frame)
        assert ref.same_floats(D, loop), (side, frame)
        want = oracle.dtw(a.reshape(-1), b.reshape(-1), 3, -1, squared)
        assert np.isnan(D[-1, -1]) == np.isnan(want) and ref.same_floats(D[-1, -1], want), (side, frame)
        cost, path, fmap = ref.align(a, b, squared=squared)
        assert not np.isfinite(cost) and path.shape == (0, 2) and fmap.size == 0
        old = _cumulative_np_minimum(a, b, squared=squared)
        differs += int(not ref.same_floats(D, old))
        nans += int(np.isnan(D[-1, -1]))
        infs += int(np.isposinf(D[-1, -1]))
    if np.isnan(value):
        assert differs >= 1 and nans >= 1 and infs >= 1               # the order shows: np.minimum gives other matrices
    else:
        assert differs == 0 and nans == 0 and infs == 6               # +inf costs: no NaN arises, the order is moot
