"""Full-matrix numpy restatement of the DTW spotting definition ("Spotting") -- TEST
INFRASTRUCTURE, the reference ssym_dtw_spot and ssym_spot_queries are held to.

c(i,j) is dtw_path_ref.local_costs' (the oracle's operation order), i a source frame, j a target frame:

    D(i,0)  = c(i,0)                                             a path may start at any source frame
    D(i,j)  = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)),  j >= 1, outside the matrix +inf
    st(i,0) = i;  st(i,j) = st of the predecessor the alignment rule picks: with dg = D(i-1,j-1), up = D(i-1,j),
              lf = D(i,j-1): diagonal if dg <= up and dg <= lf, else up if up <= lf, else left
    end     = the smallest i at which D(i,Fb-1) is least (i ascending from (none, +inf), strict <)
    cost    = D(end,Fb-1);  start = st(end,Fb-1);  nothing to spot: (+inf, NO_MATCH, NO_MATCH)

Every operation is elementwise IEEE f64, so evaluating a whole anti-diagonal at once gives the bits of the cell-by-cell
loop.  min is dtw_path_ref.min3, the oracle's comparisons in the oracle's order (from up, then lf, then dg, strict <),
which matters as soon as an operand is NaN: a NaN up stays, a NaN lf or dg is passed over.  A NaN source frame i
therefore makes D(i, .) NaN and D(i', j) NaN for every i' > i and j >= 1 (column 0 restarts, so a one-frame target is
alive again in row i + 1); a NaN target frame j makes D(., j) NaN and D(., j') = +inf for j' > j.  The predecessor
rule's <= comparisons are false on NaN: a NaN in up or lf picks left whatever dg holds, a NaN dg is never picked and
leaves up against lf.  The end rule's strict < keeps NaN and +inf from winning."""
import numpy as np

from dtw_path_ref import local_costs, min3

NO_MATCH = 0xFFFFFFFF


def matrices(a, b, squared=False):
    """(D, st), both [Fa, Fb]; Fa, Fb >= 1."""
    c = local_costs(a, b, squared)
    fa, fb = c.shape
    D = np.full((fa + 1, fb + 1), np.inf)        # D[i+1, j+1] = D(i, j); row / column 0 are the +inf border
    S = np.full((fa + 1, fb + 1), -1, dtype=np.int64)
    for s in range(fa + fb - 1):
        i = np.arange(max(0, s - fb + 1), min(fa - 1, s) + 1)
        j = s - i
        dg, up, lf = D[i, j], D[i, j + 1], D[i + 1, j]
        cur = c[i, j] + min3(up, lf, dg)
        st = np.where((dg <= up) & (dg <= lf), S[i, j], np.where(up <= lf, S[i, j + 1], S[i + 1, j]))
        first = j == 0
        D[i + 1, j + 1] = np.where(first, c[i, j], cur)
        S[i + 1, j + 1] = np.where(first, i, st)
    return D[1:, 1:], S[1:, 1:]


def first_end(last_column):
    """(end, cost) of a column D(., Fb-1): the first least value, strict <, from (NO_MATCH, +inf)."""
    end, cost = NO_MATCH, np.inf
    for i, v in enumerate(last_column):
        if v < cost:
            end, cost = i, float(v)
    return end, cost


def backtrace_start(D, end):
    """(the source frame at which the alignment backtrace from (end, Fb-1) first reaches column 0, the number of cells
    on the way at which the smallest predecessor was not unique)."""
    i, j = end, D.shape[1] - 1
    ties = 0
    while j > 0:
        dg = D[i - 1, j - 1] if i > 0 else np.inf
        up = D[i - 1, j] if i > 0 else np.inf
        lf = D[i, j - 1]
        m = min(dg, up, lf)
        ties += int(int(dg == m) + int(up == m) + int(lf == m) > 1)
        if dg <= up and dg <= lf:
            i, j = i - 1, j - 1
        elif up <= lf:
            i -= 1
        else:
            j -= 1
    return i, ties


def spot(a, b, squared=False, want_ties=False):
    """(cost, start, end) of target b inside source a; with want_ties also (rows of the end column that hold the least
    value, tied cells on the backtrace from the end to column 0)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    none = (float("inf"), NO_MATCH, NO_MATCH)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return none + (0, 0) if want_ties else none
    D, S = matrices(a, b, squared)
    end, cost = first_end(D[:, -1])
    if end == NO_MATCH:
        return none + (0, 0) if want_ties else none
    out = (cost, int(S[end, -1]), end)
    if want_ties:
        out += (int(np.count_nonzero(D[:, -1] == cost)), backtrace_start(D, end)[1])
    return out


def spot_best(sources, target, squared=False):
    """(index, cost, start, end): the first least spot cost over the sources in ascending order, strict < from
    (NO_MATCH, +inf) -- ssym_spot_queries' fold for one target."""
    best = (NO_MATCH, float("inf"), NO_MATCH, NO_MATCH)
    for s, a in enumerate(sources):
        cost, start, end = spot(a, target, squared)
        if cost < best[1]:
            best = (s, cost, start, end)
    return best
