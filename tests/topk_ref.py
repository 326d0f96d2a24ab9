"""Plain numpy restatement of ssym_match_queries / ssym_match_topk's selection (TEST INFRASTRUCTURE ONLY).

Written from include/soundsym_amd.h and the reference's fold (src/sound.rs:351-370), not from the kernels: it takes a
value matrix [n_sources][n_targets] (cosine similarities or dtw costs, from the CPU oracle) and says which sources a
target's row holds and in which order.

    key       = |value - distance|              (src/sound.rs:359)
    enters    : key < fold_start, strictly      (src/sound.rs:362: NaN keys and infinite dtw keys never enter)
    order     : (key, index) ascending          (the first minimum wins, then the next one above it)
    missing   : index -1, value NaN             (SSYM_NO_MATCH / NaN in the library)
    reported  : report="key": the key (refcos); report="value": the matrix entry itself (dtw: the winner's cost)
    index_base: added to every real entry, modulo 2^32; a missing entry stays -1

The k = 1 form (`first`) is the reference's fold itself: when nothing enters, index 0 + index_base and the fold's start.

The helpers at the end compare the library's rows with these and check the tie-separation precondition of the dtw
cases; none of them calls the oracle library or the GPU.
"""
import numpy as np

NO_MATCH = 0xFFFFFFFF
REFCOS = dict(default_distance=1.0, fold_start=2.0, report="key")
DTW = dict(default_distance=0.0, fold_start=float("inf"), report="value")


def keys(values, distance=None, default_distance=1.0):
    """[n][m] keys |value - distance[t]| (distance None: the default for every target)."""
    values = np.asarray(values, dtype=np.float64)
    n, m = values.shape
    d = np.full(m, float(default_distance)) if distance is None else np.asarray(distance, dtype=np.float64).reshape(m)
    with np.errstate(invalid="ignore"):
        return np.abs(values - d[None, :])


def topk(values, k, distance=None, default_distance=1.0, fold_start=2.0, index_base=0, report="key"):
    """(idx int64 [m][k], val f64 [m][k]) by the rules above."""
    values = np.asarray(values, dtype=np.float64)
    n, m = values.shape
    key = keys(values, distance, default_distance)
    idx = np.full((m, k), -1, dtype=np.int64)
    val = np.full((m, k), np.nan)
    for t in range(m):
        col = key[:, t]
        with np.errstate(invalid="ignore"):
            enters = np.flatnonzero(col < fold_start)            # (NaN < x is False)
        order = enters[np.argsort(col[enters], kind="stable")][:k]      # stable over the natural index order
        idx[t, :order.size] = (order + int(index_base)) & 0xFFFFFFFF
        val[t, :order.size] = col[order] if report == "key" else values[order, t]
    return idx, val


def first(values, distance=None, default_distance=1.0, fold_start=2.0, index_base=0, report="key"):
    """(idx int64 [m], val f64 [m]): the fold of src/sound.rs:361-367 per target, sequentially."""
    values = np.asarray(values, dtype=np.float64)
    n, m = values.shape
    key = keys(values, distance, default_distance)
    idx = np.zeros(m, dtype=np.int64)
    val = np.full(m, float(fold_start))
    for t in range(m):
        best_i, best = 0, float(fold_start)
        won = False
        for s in range(n):
            if key[s, t] < best:
                best_i, best, won = s, float(key[s, t]), True
        idx[t] = (best_i + int(index_base)) & 0xFFFFFFFF
        val[t] = (best if report == "key" else float(values[best_i, t])) if won else float(fold_start)
    return idx, val


def rows(values, k, distance=None, default_distance=1.0, fold_start=2.0, index_base=0, report="key"):
    """What ssym_match_topk returns, [m][k]: `topk` for k > 1; for k = 1 the call is ssym_match_queries, so a target
    nothing enters for has `first`'s index 0 + index_base and the fold's start, not a missing entry."""
    if k > 1:
        return topk(values, k, distance, default_distance, fold_start, index_base, report)
    idx, val = first(values, distance, default_distance, fold_start, index_base, report)
    return idx[:, None], val[:, None]


# -- comparing the library's rows -------------------------------------------------------------------------------------
def rows_as_int64(idx_u32):
    """uint32 rows of the library -> int64 with -1 for SSYM_NO_MATCH."""
    idx_u32 = np.asarray(idx_u32)
    return np.where(idx_u32 == NO_MATCH, -1, idx_u32.astype(np.int64))


def check_rows(idx, val, want_idx, want_val, rtol=0.0):
    """Indices equal; values bit for bit (rtol 0) or within rtol relative; missing entries NaN."""
    idx, val = np.asarray(idx), np.asarray(val)
    assert idx.shape == want_idx.shape, (idx.shape, want_idx.shape)
    got = rows_as_int64(idx)
    bad = np.argwhere(got != want_idx)
    assert bad.size == 0, "rows differ first at (target, rank) %s: got %s, want %s" % (
        bad[0], got[bad[0][0]], want_idx[bad[0][0]])
    have = want_idx >= 0
    assert np.isnan(val[~have]).all(), "a missing entry's value is not NaN"
    if rtol == 0.0:
        assert np.array_equal(val[have], want_val[have]), "values differ in their bits"
    else:
        g, w = val[have], want_val[have]
        with np.errstate(invalid="ignore"):
            ok = (g == w) | (np.abs(g - w) <= rtol * np.abs(w))      # (equal: also the fold's start +inf of k = 1)
        assert ok.all(), "values outside %g relative" % rtol


def check_first_entry(idx_row, val_row, one_idx, one_val):
    """Entry 0 of every row that has an entry is ssym_match_queries' answer for the same arguments, bit for bit."""
    has = np.asarray(idx_row)[:, 0] != NO_MATCH
    if np.asarray(idx_row).shape[1] == 1:
        has[:] = True                      # (k = 1 is that call)
    assert np.array_equal(np.asarray(one_idx)[has], np.asarray(idx_row)[has, 0])
    assert np.array_equal(np.asarray(one_val)[has], np.asarray(val_row)[has, 0])


def assert_separated(values, k, distance=None, default_distance=0.0, fold_start=float("inf"), rel=1e-9):
    """The precondition of every dtw case, on the oracle's matrix alone: within a target's first k + 1 keys any two
    unequal keys differ by more than `rel` relative -- of the larger of the two keys and the two costs behind them, so a
    distance close to the costs does not hide a near-tie -- hence a last-place difference between two f64 evaluations
    cannot reorder a row.  Equal keys are intended ties (bit-identical duplicates, or exact integer costs)."""
    values = np.asarray(values, dtype=np.float64)
    key = keys(values, distance, default_distance)
    n, m = values.shape
    for t in range(m):
        col = key[:, t]
        with np.errstate(invalid="ignore"):
            enters = np.flatnonzero(col < fold_start)
        order = enters[np.argsort(col[enters], kind="stable")][:k + 1]
        ks, vs = col[order], np.abs(values[order, t])
        for a in range(order.size - 1):
            gap = ks[a + 1] - ks[a]
            scale = max(ks[a + 1], ks[a], vs[a + 1], vs[a])
            assert gap == 0.0 or gap > rel * scale, \
                "target %d: keys %r and %r of sources %d and %d are closer than %g relative: change the seed" % (
                    t, ks[a], ks[a + 1], order[a], order[a + 1], rel)
