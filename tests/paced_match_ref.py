"""Plain numpy restatement of paced matching ("Paced matching") -- TEST INFRASTRUCTURE, the reference
ssym_match_queries_step and ssym_pair_matrix_step are held to under SSYM_STEP_PACED.

    cost(s, t)  the cost of "Paced alignment" (tests/paced_path_ref.py): +inf where paced_path_ref.feasible says no, decided
                before the recurrence, else E(Fa-1, Fb-1) of paced_path_ref.forward
    fold        ssym_match_queries' dtw rule as a plain loop: key = |cost(s, t) - distance[t]| (no distances: 0), the fold
                starts at (0, +inf) and a key replaces the held one only if it is < it -- the first minimum wins, a NaN or
                +inf key never does; the reported cost is the winner's, +inf (and index 0 + index_base) where nothing won"""
import numpy as np

import paced_path_ref

INF = float("inf")


def cost(a, b, squared=False):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if not paced_path_ref.feasible(a.shape[0], b.shape[0]):
        return INF
    return float(paced_path_ref.forward(a, b, squared)[0][-1])


def matrix(src, tgt, squared=False):
    """[len(src)][len(tgt)] f64."""
    out = np.full((len(src), len(tgt)), INF)
    for s, a in enumerate(src):
        for t, b in enumerate(tgt):
            out[s, t] = cost(a, b, squared)
    return out


def fold(mat, distance=None, index_base=0):
    """(idx uint32 [m], cost f64 [m]) of a cost matrix [n][m]."""
    n, m = mat.shape
    idx = np.zeros(m, dtype=np.uint32)
    out = np.full(m, INF)
    for t in range(m):
        delta = 0.0 if distance is None else float(distance[t])
        best, best_key, best_cost = 0, INF, INF
        for s in range(n):
            with np.errstate(invalid="ignore"):
                key = abs(float(mat[s, t]) - delta)
            if key < best_key:
                best, best_key, best_cost = s, key, float(mat[s, t])
        idx[t] = best + index_base
        out[t] = best_cost
    return idx, out


def match(src, tgt, distance=None, index_base=0, squared=False):
    return fold(matrix(src, tgt, squared), distance, index_base)


def abc_case(seed=0xABC):
    """The motivating case: the target u (10 frames x 13 values); A = u with every frame three times (30 frames: the
    symmetric cost is 0.0, and no paced path exists since 30 > 2 * 10 - 1), B = u + 1e-3 noise, C random.
    Returns ([A, B, C], [u])."""
    rng = np.random.default_rng(seed)
    real = lambda shape: rng.standard_normal(shape).astype(np.float32).astype(np.float64)    # (f32 values: both dtypes hold them)
    u = real((10, 13))
    a = np.repeat(u, 3, axis=0)
    b = (u + 1e-3 * rng.standard_normal((10, 13))).astype(np.float32).astype(np.float64)
    c = real((10, 13))
    return [a, b, c], [u]
