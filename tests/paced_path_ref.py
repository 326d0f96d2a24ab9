"""Full-matrix numpy restatement of the paced alignment definition ("Paced alignment") -- TEST
INFRASTRUCTURE, the reference ssym_dtw_align_step is held to under SSYM_STEP_PACED.

c(i,j) is dtw_path_ref.local_costs' (the oracle's operation order), i a source frame, j a target frame, both ends pinned:

    shape   : Fa = 0, Fb = 0, or Fa outside paced_ref.span_bounds(Fb)  ->  cost +inf, no path, before the recurrence
    N(0,0) = c(0,0);  N(i,0) = +inf for i >= 1;  H(i,0) = +inf
    E(i,j) = N(i,j); if H(i,j) < N(i,j): H(i,j)                        (strict <: a tie keeps N)           -> rep(i,j)
    j >= 1:  P = E(i-1,j-1); if E(i-2,j-1) < P: E(i-2,j-1)              (strict <; outside the matrix +inf) -> skip(i,j)
             N(i,j) = c(i,j) + P;   H(i,j) = c(i,j) + N(i,j-1)
    cost    = E(Fa-1,Fb-1);  a path only if it is finite
    backward: at (Fa-1,Fb-1) the state is H if rep there, else N.
              state H at (i,j): the cell before is (i, j-1), in state N.
              state N at (i,j): the cell before is (i-2,j-1) if skip(i,j), else (i-1,j-1); its state is H if rep there, else N.
    path[j] = (i_j, j);  map[j] = i_j

A column depends on the column before it alone and every operation is elementwise IEEE f64, so evaluating a whole column
at once gives the bits of the cell-by-cell loop (paced_ref.profile's argument).  The comparisons are strict < on arrays:
a NaN on either side is false, so a NaN P stays, a NaN second diagonal is passed over and a NaN H never replaces N --
over the WHOLE matrix, cells the start cannot reach included."""
import numpy as np

from dtw_path_ref import local_costs
from paced_ref import _down, span_bounds

EMPTY = (np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64))


def feasible(fa, fb):
    """Whether a source of fa frames and a target of fb frames admit a pinned paced path at all."""
    if fa == 0 or fb == 0:
        return False
    lo, hi = span_bounds(fb)
    return lo <= fa <= hi


def forward(a, b, squared=False):
    """(E(., Fb-1) f64 [Fa], skip bool [Fa, Fb], rep bool [Fa, Fb]); Fa, Fb >= 1."""
    c = local_costs(a, b, squared)
    fa, fb = c.shape
    skip = np.zeros((fa, fb), dtype=bool)
    rep = np.zeros((fa, fb), dtype=bool)
    n = np.full(fa, np.inf)
    n[0] = c[0, 0]
    e = n.copy()
    with np.errstate(invalid="ignore"):
        for j in range(1, fb):
            p, p2 = _down(e, 1, np.inf), _down(e, 2, np.inf)
            skip[:, j] = p2 < p
            p = np.where(skip[:, j], p2, p)
            h = c[:, j] + n
            n = c[:, j] + p
            rep[:, j] = h < n
            e = np.where(rep[:, j], h, n)
    return e, skip, rep


def walk(skip, rep):
    """The source frame of every target frame, int64 [Fb], walked back from (Fa-1, Fb-1); only for a finite cost."""
    fa, fb = skip.shape
    rows = np.zeros(fb, dtype=np.int64)
    i, want_e = fa - 1, True
    for j in range(fb - 1, 0, -1):
        rows[j] = i
        if want_e and rep[i, j]:
            want_e = False                       # state H: the cell before is (i, j-1), in state N
        else:
            i -= 2 if skip[i, j] else 1          # state N
            want_e = True
    rows[0] = i
    return rows


def align(a, b, squared=False):
    """(cost, path [Fb, 2] int64, map [Fb] int64); an empty path and map when the cost is not finite."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if not feasible(a.shape[0], b.shape[0]):
        return (float("inf"),) + EMPTY
    e, skip, rep = forward(a, b, squared)
    cost = float(e[-1])
    if not np.isfinite(cost):
        return (cost,) + EMPTY
    rows = walk(skip, rep)
    return cost, np.stack([rows, np.arange(rows.size, dtype=np.int64)], axis=1), rows


def admissible(rows, fa):
    """Whether i_0 ... i_{Fb-1} is a pinned paced path: from 0 to fa - 1, steps of 0, 1 or 2, never two 0 steps in a row."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0 or rows[0] != 0 or rows[-1] != fa - 1:
        return False
    d = np.diff(rows)
    return bool(((d >= 0) & (d <= 2)).all() and not ((d[:-1] == 0) & (d[1:] == 0)).any())


def resum(c, rows):
    """c summed along the path in path order, acc = c(p_0), acc = c(p_j) + acc: the recurrence's own additions."""
    acc = c[rows[0], 0]
    for j in range(1, len(rows)):
        acc = c[rows[j], j] + acc
    return float(acc)


def brute_force(c):
    """(least cost, or +inf when no admissible pinned path has a finite sum) by enumeration of every admissible pinned
    path, each summed in path order."""
    fa, fb = c.shape
    best = float("inf")

    def go(j, i, acc, stood):
        nonlocal best
        if j == fb - 1:
            if i == fa - 1 and acc < best:
                best = float(acc)
            return
        for step in ((1, 2) if stood else (0, 1, 2)):
            if i + step < fa:
                go(j + 1, i + step, c[i + step, j + 1] + acc, step == 0)

    go(0, 0, c[0, 0], False)
    return best
