"""Plain numpy restatement of the cover ("Cover") -- TEST INFRASTRUCTURE, the reference ssym_dtw_cover
is held to.

c, the squared option and the arithmetic are those of "Paced alignment" (tests/paced_path_ref.py).  For one target X of T
frames and sources n = 0 ... N-1 of Fa[n] frames:

    w(n,s,L)  = paced_match_ref.cost(source n, X[s ... s+L-1]): +inf where paced_path_ref.feasible says no, decided before
                the recurrence, else E(Fa-1, L-1) -- a source of Fa frames covers windows of ceil((Fa+1)/2) ... 2 Fa frames
    M(s,L)    = the first least w(n,s,L) over n ascending from (none, +inf), strict <  (NaN and +inf never win) -> src(s,L)
    best(-1)  = 0
    best(e)   = scan L = 1 ... min(e+1, 2 Fmax) ascending from (none, +inf), strict <, over the L that have a src(e-L+1, L):
                v = (M(e-L+1, L) + piece_penalty) + best(e-L)  -> the first least v, its (L, src, M)
    cover     : walk back from e = T-1 while best is finite: piece (src, start = e-L+1, end = e, cost = M); e <- e-L
    total     = best(T-1);  count = pieces;  pieces reported in ascending start
    no cover  : T = 0, or best(T-1) not finite -> count 0, total +inf

A column of the paced recurrence depends on the column before it alone, so one forward pass per (n, s) over the longest
window yields w(n,s,L) for every L: window_costs.  tables() runs that pass for every start of a source at once -- column j
of start s is target frame s + j, the operations are paced_path_ref.forward's, elementwise IEEE f64, so the bits are those of
one pass per start (tests/test_cover_ref.py holds the three to each other)."""
import numpy as np

import paced_match_ref
import paced_path_ref
from dtw_path_ref import local_costs

INF = float("inf")
NONE = 0xFFFFFFFF


def window_costs(a, x, s, squared=False):
    """w(n, s, L) for L = 1 ... min(2 Fa, T - s) as f64 [that many] (entry L - 1), from ONE forward pass of source a over
    x[s:]: paced_path_ref.forward's recurrence, with the bottom row kept after every column."""
    a = np.asarray(a, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    fa = a.shape[0]
    cols = min(2 * fa, x.shape[0] - s)
    out = np.full(max(cols, 0), INF)
    if fa == 0 or cols <= 0:
        return out
    c = local_costs(a, x[s:s + cols], squared)
    n = np.full(fa, np.inf)
    n[0] = c[0, 0]
    e = n.copy()
    with np.errstate(invalid="ignore"):
        for j in range(cols):
            if j:
                p, p2 = paced_path_ref._down(e, 1, np.inf), paced_path_ref._down(e, 2, np.inf)
                p = np.where(p2 < p, p2, p)
                h = c[:, j] + n
                n = c[:, j] + p
                e = np.where(h < n, h, n)
            if paced_path_ref.feasible(fa, j + 1):
                out[j] = e[-1]
    return out


def tables(src, x, squared=False):
    """(M f64 [T][W], src uint32 [T][W]) with W = 2 Fmax (at least 2): entry [s][L - 1]; NONE and +inf where no source has
    a finite w(n, s, L) or the window leaves the target."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    W = 2 * max([np.asarray(a).shape[0] for a in src] + [1])
    M = np.full((T, W), INF)
    S = np.full((T, W), NONE, dtype=np.uint32)
    for idx, a in enumerate(src):
        a = np.asarray(a, dtype=np.float64)
        fa = a.shape[0]
        if fa == 0 or T == 0:
            continue
        c = local_costs(a, x, squared)                  # [Fa][T]
        n = np.full((fa, T), np.inf)
        n[0] = c[0]
        e = n.copy()                                    # column s: the pass that starts at target frame s
        with np.errstate(invalid="ignore"):
            for j in range(min(2 * fa, T)):
                k = T - j                               # the starts that still have a column j
                if j:
                    e, n = e[:, :k], n[:, :k]
                    p = np.full((fa, k), np.inf)
                    p[1:] = e[:-1]
                    p2 = np.full((fa, k), np.inf)
                    p2[2:] = e[:-2]
                    p = np.where(p2 < p, p2, p)
                    cj = c[:, j:]
                    h = cj + n
                    n = cj + p
                    e = np.where(h < n, h, n)
                if paced_path_ref.feasible(fa, j + 1):
                    w = e[-1]
                    win = w < M[:k, j]                  # sources ascend: the first minimum stays
                    M[:k, j] = np.where(win, w, M[:k, j])
                    S[:k, j] = np.where(win, idx, S[:k, j])
    return M, S


def chain(M, S, penalty=0.0):
    """(pieces [(src, start, end, cost)], total) of the tables of one target."""
    T, W = M.shape
    penalty = float(penalty)
    best = np.full(T + 1, INF)                          # best[e + 1]
    best[0] = 0.0
    back = [None] * T
    for e in range(T):
        held, pick = INF, None
        for L in range(1, min(e + 1, W) + 1):
            s = e - L + 1
            if S[s, L - 1] == NONE:
                continue
            v = (float(M[s, L - 1]) + penalty) + float(best[s])
            if v < held:
                held, pick = v, (L, int(S[s, L - 1]), float(M[s, L - 1]))
        best[e + 1], back[e] = held, pick
    if T == 0 or not np.isfinite(best[T]):
        return [], INF
    pieces, e = [], T - 1
    while e >= 0:
        L, s, m = back[e]
        pieces.append((s, e - L + 1, e, m))
        e -= L
    return pieces[::-1], float(best[T])


def cover(src, x, penalty=0.0, squared=False):
    """(pieces [(src, start, end, cost)] in ascending start, total); ([], +inf) without a cover."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return [], INF
    return chain(*tables(src, x, squared), penalty)


def all_tables(src, targets, squared=False):
    """tables() of every target with frames (None for one without): what arrays() takes as tabs, so that several penalties
    share one forward pass."""
    return [tables(src, x, squared) if np.asarray(x).shape[0] else None for x in targets]


def arrays(src, targets, penalty=0.0, squared=False, tabs=None):
    """What ssym_dtw_cover returns for a query set: (count uint32 [m], total f64 [m], src, start, end uint32 [F], cost f64
    [F]), target t's pieces from slot (frames before t) on, NONE and +inf in the unused slots."""
    if tabs is None:
        tabs = all_tables(src, targets, squared)
    off = np.concatenate([[0], np.cumsum([np.asarray(x).shape[0] for x in targets])]).astype(np.int64)
    F, m = int(off[-1]), len(targets)
    count, total = np.zeros(m, dtype=np.uint32), np.full(m, INF)
    s, a, e = (np.full(F, NONE, dtype=np.uint32) for _ in range(3))
    c = np.full(F, INF)
    for t, x in enumerate(targets):
        pieces, total[t] = chain(*tabs[t], penalty) if tabs[t] is not None else ([], INF)
        count[t] = len(pieces)
        for k, (ps, pa, pe, pc) in enumerate(pieces):
            s[off[t] + k], a[off[t] + k], e[off[t] + k], c[off[t] + k] = ps, pa, pe, pc
    return count, total, s, a, e, c


def resum(pieces, penalty=0.0):
    """acc = 0; acc = (cost_k + piece_penalty) + acc in piece order: the chain's own additions."""
    acc = 0.0
    for _, _, _, cost in pieces:
        acc = (float(cost) + float(penalty)) + acc
    return acc


def brute_force(src, x, penalty=0.0, squared=False):
    """The least total over EVERY tiling of x and every choice of sources, each tiling summed in piece order, every piece
    cost paced_match_ref.cost on the cut; +inf when no tiling has a finite sum."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    piece = {}
    for s in range(T):
        for e in range(s, T):
            held = INF
            for a in src:
                w = paced_match_ref.cost(a, x[s:e + 1], squared)
                if w < held:
                    held = w
            piece[s, e] = held
    best = INF

    def go(s, acc):
        nonlocal best
        if s == T:
            if acc < best:
                best = acc
            return
        for e in range(s, T):
            if piece[s, e] < INF:
                go(e + 1, (piece[s, e] + float(penalty)) + acc)

    if T:
        go(0, 0.0)
    return best


def _real(rng, shape):
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)     # (f32 values: both engine dtypes hold them)


def planted_case(noise=0.0, seed=0xC0FE, dim=13):
    """The planted case: 10 segments of 1 ... 40 frames x dim values; the target is segments 3, 0, 7, 5, 2, 9, 6 in that
    order, as an exact copy, a copy with every frame doubled, or (odd lengths only) every second frame of a copy, the three
    variants alternating.  noise > 0: that much Gaussian noise on the target (rounded to f32 values).
    Returns (segments, target, planted pieces [(src, start, end)])."""
    rng = np.random.default_rng(seed)
    lens = [40, 17, 9, 25, 33, 5, 1, 21, 12, 29]
    segs = [_real(rng, (n, dim)) for n in lens]
    parts, pieces, at, variant = [], [], 0, 0
    for s in (3, 0, 7, 5, 2, 9, 6):
        a = segs[s]
        kind = variant % 3
        if kind == 2 and a.shape[0] % 2 == 0:
            kind = 0                                     # every second frame pins both ends only for an odd length
        part = a if kind == 0 else np.repeat(a, 2, axis=0) if kind == 1 else a[::2]
        variant += 1
        parts.append(part)
        pieces.append((s, at, at + part.shape[0] - 1))
        at += part.shape[0]
    target = np.concatenate(parts, axis=0)
    if noise:
        target = (target + noise * rng.standard_normal(target.shape)).astype(np.float32).astype(np.float64)
    return segs, target, pieces
