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
