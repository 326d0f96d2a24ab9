"""Numpy restatement of the occurrences definition ("Occurrences") -- TEST INFRASTRUCTURE, the
reference ssym_dtw_spot_all is held to.  c, D and st are spot_ref.matrices' (the definition of "Spotting"):

    delta(i) = D(i,Fb-1),  s(i) = st(i,Fb-1)                the end-column profile
    candidate: an end i with delta(i) finite and delta(i) <= max_cost (+inf when none is given), not yet dead
    pick m   : the candidate with the least delta, among equals the smallest i (i ascending from (none, +inf), strict <)
    kill     : every end i with s(i) <= i* and i >= s(i*) is dead from now on
    stop     : after K picks, or when no candidate is left
    count    = picks made;  slots count ... K-1 hold (+inf, NO_MATCH, NO_MATCH);  no frames on either side: count 0"""
import numpy as np

from spot_ref import NO_MATCH, matrices


def profile(a, b, squared=False):
    """(delta f64 [Fa], s int64 [Fa]); Fa, Fb >= 1."""
    D, S = matrices(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), squared)
    return D[:, -1].copy(), S[:, -1].copy()


def select(delta, s, k, max_cost=None):
    """The picks from a profile: a list of at most k (cost, start, end)."""
    limit = np.inf if max_cost is None else float(max_cost)
    dead = np.zeros(delta.size, dtype=bool)
    ends = np.arange(delta.size)
    out = []
    while len(out) < k:
        # what is no candidate counts as +inf (NaN fails delta <= limit); argmin names the first least value, and a
        # least value of +inf means that no candidate is left
        vals = np.where(~dead & (delta <= limit), delta, np.inf)
        best = int(np.argmin(vals))
        if not vals[best] < np.inf:
            break
        out.append((float(vals[best]), int(s[best]), best))
        dead |= (s <= best) & (ends >= s[best])
    return out


def padded(picks, k):
    """(count, cost f64 [k], start uint32 [k], end uint32 [k]) as the call lays a pair's picks out."""
    cost = np.full(k, np.inf)
    start = np.full(k, NO_MATCH, dtype=np.uint32)
    end = np.full(k, NO_MATCH, dtype=np.uint32)
    for m, (c, st, en) in enumerate(picks):
        cost[m], start[m], end[m] = c, st, en
    return len(picks), cost, start, end


def spot_all(a, b, k, max_cost=None, squared=False):
    """(count, cost [k], start [k], end [k]) of target b inside source a."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return padded([], k)
    delta, s = profile(a, b, squared)
    return padded(select(delta, s, k, max_cost), k)
