"""Full-matrix numpy restatement of the paced spotting definition ("Paced spotting") -- TEST
INFRASTRUCTURE, the reference ssym_dtw_spot_step, ssym_spot_queries_step and ssym_dtw_spot_all_step are held to under
SSYM_STEP_PACED.

c(i,j) is dtw_path_ref.local_costs' (the oracle's operation order), i a source frame, j a target frame.  Every cell has
two states, N (entered by a source step) and H (entered by repeating the source frame):

    N(i,0) = c(i,0), sN(i,0) = i;   H(i,0) = +inf (no start)
    E(i,j) = the cell's better state: (N, sN); if H(i,j) < N(i,j): (H, sH)          (strict <: a tie keeps N)
    j >= 1:
      P      = E(i-1,j-1); if E(i-2,j-1) < P: E(i-2,j-1)      (strict <: a tie keeps the diagonal; outside = +inf)
      N(i,j) = c(i,j) + P.value,       sN(i,j) = P.start
      H(i,j) = c(i,j) + N(i,j-1),      sH(i,j) = sN(i,j-1)     (a repeat may only follow a source step)
    delta(i) = E(i,Fb-1).value,  s(i) = E(i,Fb-1).start        (the end-column profile)
    end  = the smallest i at which delta(i) is least (i ascending from (none, +inf), strict <)
    cost = delta(end),  start = s(end);   nothing to spot: (+inf, NO_MATCH, NO_MATCH)

A column depends on the column before it alone and every operation is elementwise IEEE f64, so evaluating a whole column
at once gives the bits of the cell-by-cell loop.  The comparisons are np.where on strict <, never np.minimum: a NaN on
either side of < is false, so a NaN P stays (the diagonal is kept), a NaN second diagonal is passed over, and a NaN H
never replaces N.  Occurrences are spot_all_ref's selection, as it is, on this profile."""
import numpy as np

from dtw_path_ref import local_costs
from spot_all_ref import padded, select
from spot_ref import NO_MATCH, first_end


def _down(v, n, fill):
    """v moved n rows down: out[i] = v[i - n], `fill` above."""
    out = np.full_like(v, fill)
    if n < v.size:
        out[n:] = v[:v.size - n]
    return out


def profile(a, b, squared=False):
    """(delta f64 [Fa], s int64 [Fa]); Fa, Fb >= 1."""
    c = local_costs(a, b, squared)
    fa, fb = c.shape
    n, sn = c[:, 0].copy(), np.arange(fa, dtype=np.int64)
    e, se = n.copy(), sn.copy()
    with np.errstate(invalid="ignore"):
        for j in range(1, fb):
            p, sp = _down(e, 1, np.inf), _down(se, 1, -1)
            p2, sp2 = _down(e, 2, np.inf), _down(se, 2, -1)
            skip = p2 < p
            p, sp = np.where(skip, p2, p), np.where(skip, sp2, sp)
            h, sh = c[:, j] + n, sn
            n, sn = c[:, j] + p, sp
            rep = h < n
            e, se = np.where(rep, h, n), np.where(rep, sh, sn)
    return e, se


def spot(a, b, squared=False):
    """(cost, start, end) of target b inside source a."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return (float("inf"), NO_MATCH, NO_MATCH)
    delta, s = profile(a, b, squared)
    end, cost = first_end(delta)
    if end == NO_MATCH:
        return (float("inf"), NO_MATCH, NO_MATCH)
    return (cost, int(s[end]), end)


def spot_best(sources, target, squared=False):
    """(index, cost, start, end): the first least paced cost over the sources in ascending order, strict < from
    (NO_MATCH, +inf) -- ssym_spot_queries_step's fold for one target."""
    best = (NO_MATCH, float("inf"), NO_MATCH, NO_MATCH)
    for k, a in enumerate(sources):
        cost, start, end = spot(a, target, squared)
        if cost < best[1]:
            best = (k, cost, start, end)
    return best


def spot_all(a, b, k, max_cost=None, squared=False):
    """(count, cost [k], start [k], end [k]) of target b inside source a."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return padded([], k)
    delta, s = profile(a, b, squared)
    return padded(select(delta, s, k, max_cost), k)


def span_bounds(fb):
    """(least, most) frames of a paced span of a target of fb frames."""
    return (fb - 1) // 2 + 1, 2 * fb - 1
