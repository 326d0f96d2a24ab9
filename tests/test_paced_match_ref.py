"""tests/paced_match_ref.py on the CPU: the matrix against enumeration of every admissible path, the fold's tie, NaN and
distance rules, and the case that motivates paced matching."""
import numpy as np

import paced_match_ref as ref
import paced_path_ref
from dtw_path_ref import cumulative, local_costs

INF, NAN = float("inf"), float("nan")


def test_matrix_entries_are_the_least_admissible_path_sums():
    rng = np.random.default_rng(0x7A6)
    src = [rng.standard_normal((fa, 3)) for fa in range(0, 8)]
    tgt = [rng.standard_normal((fb, 3)) for fb in range(0, 7)]
    for squared in (False, True):
        mat = ref.matrix(src, tgt, squared)
        assert mat.shape == (8, 7)
        for s, a in enumerate(src):
            for t, b in enumerate(tgt):
                fa, fb = a.shape[0], b.shape[0]
                if fa == 0 or fb == 0:
                    assert mat[s, t] == INF
                    continue
                want = paced_path_ref.brute_force(local_costs(a, b, squared))
                assert mat[s, t] == want, (fa, fb)
                assert np.isfinite(mat[s, t]) == ((fb - 1) // 2 + 1 <= fa <= 2 * fb - 1), (fa, fb)


def test_the_fold_keeps_the_first_minimum():
    mat = np.array([[3.0, 2.0], [1.0, 2.0], [1.0, 5.0], [0.5, 2.0]])
    idx, cost = ref.fold(mat)
    assert idx.tolist() == [3, 0] and cost.tolist() == [0.5, 2.0]
    idx, cost = ref.fold(mat[:3], index_base=7)
    assert idx.tolist() == [8, 7] and cost.tolist() == [1.0, 2.0]


def test_a_nan_or_infinite_key_never_wins():
    mat = np.array([[NAN, INF, NAN], [4.0, INF, INF], [INF, INF, NAN]])
    idx, cost = ref.fold(mat, index_base=5)
    assert idx.tolist() == [6, 5, 5] and cost[0] == 4.0 and cost[1] == INF and cost[2] == INF
    # a distance that is not finite makes every key NaN or +inf
    for d in (NAN, INF, -INF):
        idx, cost = ref.fold(np.array([[1.0], [2.0]]), [d], index_base=3)
        assert idx.tolist() == [3] and cost[0] == INF


def test_the_distance_rule():
    mat = np.array([[1.0, 10.0], [4.0, 6.0], [7.0, 2.0], [INF, 9.0]])
    idx, cost = ref.fold(mat, [5.0, 4.0])
    assert idx.tolist() == [1, 1] and cost.tolist() == [4.0, 6.0]      # |4 - 5| first among two keys of 1; |6 - 4| = |2 - 4|: the first
    idx, cost = ref.fold(mat, [100.0, 0.0])
    assert idx.tolist() == [2, 2] and cost.tolist() == [7.0, 2.0]


def test_the_motivating_case():
    """The symmetric search picks A at cost 0.0; A has no paced path; the best paced match is B."""
    src, tgt = ref.abc_case()
    u = tgt[0]
    assert [s.shape for s in src] == [(30, 13), (10, 13), (10, 13)] and u.shape == (10, 13)
    sym = [float(cumulative(s, u)[-1, -1]) for s in src]
    assert sym[0] == 0.0 and int(np.argmin(sym)) == 0 and sym[1] > 0.0
    assert not paced_path_ref.feasible(30, 10) and 30 > 2 * 10 - 1
    mat = ref.matrix(src, tgt)
    assert mat[0, 0] == INF and 0.0 < mat[1, 0] < mat[2, 0] < INF
    idx, cost = ref.fold(mat)
    assert idx.tolist() == [1] and cost[0] == mat[1, 0]
    # the winner is a pair the paced alignment aligns, at that cost, with one cell per target frame
    c, path, fmap = paced_path_ref.align(src[1], u)
    assert c == cost[0] and len(fmap) == 10


def test_planted_cuts_cost_exactly_zero():
    """A target that is a cut of an entry with every second frame dropped, or with every frame doubled, matches it at 0.0."""
    rng = np.random.default_rng(0x2E0)
    entry = rng.standard_normal((21, 5))
    other = rng.standard_normal((21, 5))
    halved, doubled = entry[::2], np.repeat(entry[:11], 2, axis=0)[:21]
    src = [other, entry, entry[:11]]
    mat = ref.matrix(src, [halved, doubled])
    assert mat[1, 0] == 0.0 and mat[2, 1] == 0.0
    idx, cost = ref.fold(mat)
    assert idx.tolist() == [1, 2] and cost.tolist() == [0.0, 0.0]
