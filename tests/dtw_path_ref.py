"""Full-matrix numpy restatement of the DTW alignment definition ("Alignment") -- TEST
INFRASTRUCTURE, the reference the GPU paths of ssym_dtw_align are held to.

D is formed as oracle.np_dtw forms it: c(i,j) = sum_k (a_ik - b_jk)^2 with k ascending, subtraction, product and sum
rounded separately in f64, the square root rounded separately unless `squared`; D(i,j) = c(i,j) + min(D(i-1,j),
D(i,j-1), D(i-1,j-1)), D(0,0) = c(0,0), cells with |i - j| > band are +inf.  (Every operation is elementwise IEEE f64,
so evaluating a whole anti-diagonal at once gives the bits of the cell-by-cell loop.)

The minimum is min3 below, the oracle's comparisons in the oracle's order: best = D(i-1,j); if D(i,j-1) < best, take it;
if D(i-1,j-1) < best, take it.  Among numbers the order does not matter; with a NaN operand it does, because every
comparison with NaN is false: a NaN in D(i-1,j) stays, a NaN in D(i,j-1) or D(i-1,j-1) is passed over.  So a NaN feature
does not simply flood the matrix: a NaN source frame i makes row i NaN and, through `up`, every later row from column 1
on; a NaN target frame j makes column j NaN and every later column +inf (column j + 1 sees NaN in `lf` and `dg`, passes
over both, and is left with the +inf above row 0).

The path is found backwards from (Fa-1, Fb-1): at (i,j) != (0,0), with dg = D(i-1,j-1), up = D(i-1,j), lf = D(i,j-1)
(+inf outside the matrix or the band), go diagonally if dg <= up and dg <= lf, else up if up <= lf, else left.  With a
NaN operand the comparisons that name it are false: a NaN in up or in lf gives left, whatever dg holds (the diagonal
has to pass both comparisons, up has to pass up <= lf); a NaN dg is never taken and leaves up against lf.  (A path is
only asked for when the cost is finite, and then no cell on it is NaN; the rule matters for the starts that spot_ref
carries through every cell.)
map[j] = the smallest i with (i,j) on the path.  A cost that is not finite gives an empty path and an empty map."""
import numpy as np


def min3(up, lf, dg):
    """The oracle's minimum of D(i-1,j), D(i,j-1), D(i-1,j-1), elementwise: starts from `up`, replaces it by strict <.
    Not np.minimum, which returns NaN whenever an operand is NaN."""
    best = np.where(lf < up, lf, up)
    return np.where(dg < best, dg, best)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same_floats(got, want):
    """Whether two f64 arrays hold the same values: NaN where the other has NaN (whatever its sign and payload: the
    default NaN differs between processors), the same bits everywhere else."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    keep = ~np.isnan(want)
    return np.array_equal(bits(got[keep]), bits(want[keep]))


def local_costs(a, b, squared=False):
    """c(i,j) for every cell, [Fa, Fb] f64, in the oracle's operation order."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):      # a huge or non-finite feature: +inf or NaN, as IEEE has it
        for k in range(a.shape[1]):
            df = a[:, k][:, None] - b[:, k][None, :]
            acc = acc + df * df
        return acc if squared else np.sqrt(acc)


def cumulative(a, b, band=-1, squared=False):
    """D, [Fa, Fb] f64 (+inf outside the band)."""
    c = local_costs(a, b, squared)
    fa, fb = c.shape
    D = np.full((fa + 1, fb + 1), np.inf)        # D[i+1, j+1] = D(i, j); row / column 0 are the +inf border
    for s in range(fa + fb - 1):
        i = np.arange(max(0, s - fb + 1), min(fa - 1, s) + 1)
        j = s - i
        if band >= 0:
            keep = np.abs(i - j) <= band
            i, j = i[keep], j[keep]
            if i.size == 0:
                continue
        best = min3(D[i, j + 1], D[i + 1, j], D[i, j])
        if s == 0:
            best = np.zeros(1)
        D[i + 1, j + 1] = c[i, j] + best
    return D[1:, 1:]


def cumulative_loop(c, free_start=False):
    """D from local costs c, one cell at a time with Python floats, written as oracle/ssym_oracle.c writes its inner loop
    (no band).  free_start: column 0 restarts in every row (spotting) instead of accumulating (plain DTW).  Slow: what
    the vectorised forms are checked against."""
    fa, fb = c.shape
    inf = float("inf")
    D = [[inf] * fb for _ in range(fa)]
    for i in range(fa):
        for j in range(fb):
            cij = float(c[i, j])
            if j == 0 and (free_start or i == 0):
                D[i][j] = cij
                continue
            best = D[i - 1][j] if i > 0 else inf
            lf = D[i][j - 1] if j > 0 else inf
            dg = D[i - 1][j - 1] if i > 0 and j > 0 else inf
            if lf < best:
                best = lf
            if dg < best:
                best = dg
            D[i][j] = cij + best
    return np.array(D, dtype=np.float64).reshape(fa, fb)


def backtrace(D):
    """(path [L, 2] int64 in forward order, ties) from a finite D(Fa-1, Fb-1); ties = cells at which the smallest
    predecessor was not unique."""
    fa, fb = D.shape
    i, j = fa - 1, fb - 1
    cells = [(i, j)]
    ties = 0
    while i > 0 or j > 0:
        dg = D[i - 1, j - 1] if i > 0 and j > 0 else np.inf
        up = D[i - 1, j] if i > 0 else np.inf
        lf = D[i, j - 1] if j > 0 else np.inf
        m = min(dg, up, lf)
        ties += int(int(dg == m) + int(up == m) + int(lf == m) > 1)
        if dg <= up and dg <= lf:
            i, j = i - 1, j - 1
        elif up <= lf:
            i -= 1
        else:
            j -= 1
        cells.append((i, j))
    return np.array(cells[::-1], dtype=np.int64), ties


def frame_map(path, fb):
    """map[j] = the smallest i with (i, j) on the path."""
    out = np.full(fb, -1, dtype=np.int64)
    for i, j in path[::-1]:
        out[j] = i                      # walking backwards, the last write per column is the smallest i
    return out


def align(a, b, band=-1, squared=False, want_ties=False):
    """(cost, path [L, 2] int64, map [Fb] int64); an empty path and map when the cost is not finite."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    empty = (np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64))
    if a.shape[0] == 0 or b.shape[0] == 0:
        out = (float("inf"),) + empty
        return out + (0,) if want_ties else out
    D = cumulative(a, b, band, squared)
    cost = float(D[-1, -1])
    if not np.isfinite(cost):
        out = (cost,) + empty
        return out + (0,) if want_ties else out
    path, ties = backtrace(D)
    out = (cost, path, frame_map(path, b.shape[0]))
    return out + (ties,) if want_ties else out


def resum(a, b, path, squared=False):
    """c summed along the path in path order, acc = c(p_k) + acc from c(0,0): the recurrence's own additions, so it
    reproduces D(Fa-1, Fb-1) bit for bit on an optimal path."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    acc = None
    for i, j in path:
        s = 0.0
        for k in range(a.shape[1]):
            df = float(a[i, k]) - float(b[j, k])
            s = s + df * df
        c = s if squared else float(np.sqrt(np.float64(s)))
        acc = c if acc is None else c + acc
    return acc


def check_path(path, fa, fb, band=-1):
    """Assert the structural properties of a warping path."""
    path = np.asarray(path, dtype=np.int64)
    L = path.shape[0]
    assert max(fa, fb) <= L <= fa + fb - 1, (L, fa, fb)
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (fa - 1, fb - 1)
    d = np.diff(path, axis=0)
    ok = ((d[:, 0] == 1) & (d[:, 1] == 1)) | ((d[:, 0] == 1) & (d[:, 1] == 0)) | ((d[:, 0] == 0) & (d[:, 1] == 1))
    assert ok.all(), "a step outside (+1,+1), (+1,0), (0,+1)"
    if band >= 0:
        assert (np.abs(path[:, 0] - path[:, 1]) <= band).all(), "a cell outside the band"
