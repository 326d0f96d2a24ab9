"""The spotting restatement (tests/spot_ref.py) against brute force over every span of the source, with the plain DTW of
tests/dtw_path_ref.py: the spot's cost has the bits of the plain cost of its span, is the least plain cost over all
spans, ends at the first end that reaches it, and starts where the alignment backtrace reaches column 0."""
import numpy as np
import pytest

import dtw_path_ref as ref
import spot_ref


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _brute(a, b, squared):
    """cost[s, e] of plain DTW (source[s ... e], target) for every span, +inf where s > e."""
    fa = a.shape[0]
    cost = np.full((fa, fa), np.inf)
    for s in range(fa):
        for e in range(s, fa):
            cost[s, e] = ref.align(a[s:e + 1], b, squared=squared)[0]
    return cost


def _cases(kind, n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        fa, fb, dim = int(rng.integers(1, 13)), int(rng.integers(1, 9)), int(rng.integers(1, 4))
        if kind == "int":
            yield rng.integers(0, 3, size=(fa, dim)).astype(np.float64), rng.integers(0, 3, size=(fb, dim)).astype(np.float64), True
        else:
            yield rng.standard_normal((fa, dim)), rng.standard_normal((fb, dim)), bool(rng.integers(0, 2))


@pytest.mark.parametrize("kind", ["int", "real"])
def test_restatement_against_brute_force_over_all_spans(kind):
    end_ties = start_ties = 0
    for a, b, squared in _cases(kind, 150, 0x5B07 + (kind == "int")):
        cost, start, end, n_end, n_start = spot_ref.spot(a, b, squared, want_ties=True)
        brute = _brute(a, b, squared)
        assert 0 <= start <= end < a.shape[0]
        assert _bits(cost) == _bits(brute[start, end])                    # property 2: the plain cost of the span
        assert _bits(cost) == _bits(brute.min())                          # property 3: the least over all spans
        assert end == int(np.flatnonzero(brute.min(axis=0) == brute.min())[0])      # the first end that reaches it
        D, S = spot_ref.matrices(a, b, squared)
        assert start == spot_ref.backtrace_start(D, end)[0] == int(S[end, -1])      # property 1
        # the span's own alignment is the backtrace: it starts at the span's first frame and ends at its last
        _, path, _ = ref.align(a[start:end + 1], b, squared=squared)
        assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (end - start, b.shape[0] - 1)
        end_ties += int(n_end > 1)
        start_ties += int(n_start > 0)
    if kind == "int":
        assert end_ties > 10 and start_ties > 10, (end_ties, start_ties)    # the tie rules are exercised


def test_planted_span_is_found_exactly():
    rng = np.random.default_rng(0x57A7)
    a = rng.standard_normal((200, 13))
    b = a[57:97].copy()
    for squared in (False, True):
        assert spot_ref.spot(a, b, squared) == (0.0, 57, 96)
    assert spot_ref.spot_best([a[:50], a, a], b) == (1, 0.0, 57, 96)


def test_source_shorter_than_target_and_single_frames():
    rng = np.random.default_rng(0x1F)
    for fa, fb in [(3, 8), (1, 5), (7, 1), (1, 1), (2, 2)]:
        for squared in (False, True):
            a, b = rng.standard_normal((fa, 4)), rng.standard_normal((fb, 4))
            cost, start, end = spot_ref.spot(a, b, squared)
            brute = _brute(a, b, squared)
            assert _bits(cost) == _bits(brute.min()) == _bits(brute[start, end])
            assert end == int(np.flatnonzero(brute.min(axis=0) == brute.min())[0])
            if fb == 1:
                c = ref.local_costs(a, b, squared)[:, 0]
                assert start == end == int(np.argmin(c)) and cost == c.min()
            if fa == 1:
                assert (start, end) == (0, 0) and _bits(cost) == _bits(ref.align(a, b, squared=squared)[0])


def test_nothing_to_spot():
    none = (float("inf"), spot_ref.NO_MATCH, spot_ref.NO_MATCH)
    assert spot_ref.spot(np.zeros((0, 3)), np.zeros((4, 3))) == none
    assert spot_ref.spot(np.zeros((4, 3)), np.zeros((0, 3))) == none
    assert spot_ref.spot_best([], np.zeros((2, 3))) == (spot_ref.NO_MATCH,) + none
    assert spot_ref.spot_best([np.zeros((0, 3))], np.zeros((2, 3))) == (spot_ref.NO_MATCH,) + none


# ---- the comparison order of min3, which only a NaN can tell apart ------------------------------------------------------

def _matrices_np_minimum(a, b, squared):
    """D of matrices() as it was before min3 (np.minimum: order-free, NaN for any NaN operand)."""
    c = ref.local_costs(a, b, squared)
    fa, fb = c.shape
    D = np.full((fa + 1, fb + 1), np.inf)
    for s in range(fa + fb - 1):
        i = np.arange(max(0, s - fb + 1), min(fa - 1, s) + 1)
        j = s - i
        cur = c[i, j] + np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j])
        D[i + 1, j + 1] = np.where(j == 0, c[i, j], cur)
    return D[1:, 1:]


def _starts_loop(D):
    """st of every cell by the predecessor rule, one cell at a time, from a given D."""
    fa, fb = D.shape
    S = np.zeros((fa, fb), dtype=np.int64)
    inf = float("inf")
    for i in range(fa):
        S[i, 0] = i
        for j in range(1, fb):
            dg = D[i - 1, j - 1] if i > 0 else inf
            up = D[i - 1, j] if i > 0 else inf
            lf = D[i, j - 1]
            S[i, j] = (S[i - 1, j - 1] if i > 0 else -1) if (dg <= up and dg <= lf) else \
                      (S[i - 1, j] if i > 0 else -1) if up <= lf else S[i, j - 1]
    return S


@pytest.mark.parametrize("kind", ["int", "real"])
def test_finite_inputs_give_the_bits_np_minimum_gave(kind):
    for a, b, squared in _cases(kind, 150, 0x5B07 + (kind == "int")):
        assert np.array_equal(_bits(spot_ref.matrices(a, b, squared)[0]), _bits(_matrices_np_minimum(a, b, squared)))


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf"), 1e200])
def test_non_finite_inputs_against_the_cell_loop(value, squared):
    rng = np.random.default_rng(0xBAD5 + squared)
    for side, frame in (("src", 0), ("src", 4), ("src", 9), ("tgt", 0), ("tgt", 2), ("tgt", 5)):
        a, b = rng.standard_normal((10, 3)), rng.standard_normal((6, 3))
        (a if side == "src" else b)[frame, int(rng.integers(0, 3))] = value
        D, S = spot_ref.matrices(a, b, squared)
        loop = ref.cumulative_loop(ref.local_costs(a, b, squared), free_start=True)
        assert np.array_equal(np.isnan(D), np.isnan(loop)), (side, frame)
        assert ref.same_floats(D, loop), (side, frame)
        assert np.array_equal(S, _starts_loop(loop)), (side, frame)
        old = _matrices_np_minimum(a, b, squared)
        cost, start, end = spot_ref.spot(a, b, squared)
        if side == "tgt":
            # a poisoned target frame: NaN in its own column, +inf in every later one -- where np.minimum gave NaN
            assert (np.isnan(D[:, frame]) if np.isnan(value) else np.isposinf(D[:, frame])).all()
            assert np.isposinf(D[:, frame + 1:]).all() and (cost, start, end) == (float("inf"), spot_ref.NO_MATCH, spot_ref.NO_MATCH)
            assert ref.same_floats(D, old) == (not np.isnan(value) or frame == 5)
        elif np.isnan(value):
            # a NaN source frame: its row, and through `up` every later row from column 1 on; column 0 restarts
            assert np.isnan(D[frame]).all() and np.isnan(D[frame + 1:, 1:]).all() and np.isfinite(D[:frame]).all()
            assert np.isfinite(D[frame + 1:, 0]).all()
            assert (end < frame) if frame else (end == spot_ref.NO_MATCH)
        else:
            # a +inf row is a wall, not a poison: the rows behind it spot again
            assert np.isposinf(D[frame]).all() and np.isfinite(np.delete(D, frame, axis=0)).all() and np.isfinite(cost)
            assert ref.same_floats(D, old)
    a = np.zeros((5, 2))
    a[2, 0] = np.nan                     # one target frame: column 0 alone, which restarts -- the rows after the NaN live
    assert ref.same_floats(spot_ref.matrices(a, np.ones((1, 2)), True)[0][:, 0], [2.0, 2.0, np.nan, 2.0, 2.0])
