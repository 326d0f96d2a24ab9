"""Numpy restatement of the watching definition ("Watching") -- TEST INFRASTRUCTURE, the reference
ssym_spotter_* is held to.  The profile (delta(i), s(i)) of a lane against a target is spot_all_ref.profile's of everything
the lane has consumed: row i depends on rows 0 ... i alone, so the first n rows of the whole's profile are the profile of
the first n frames.  Per (lane, target):

    best    : the first least delta(i) over i ascending from (none, +inf), strict <
    report  : state pend = none, last = none.  For i ascending with (d, s) = (delta(i), s(i)):
                1. if pend and s > pend.end:            emit pend;  last = pend.end;  pend = none
                2. candidate  iff  d is finite, d <= max_cost (+inf when none is given; NaN fails) and
                                   (last = none or s > last)
                3. if candidate and (pend = none or d < pend.cost):   pend = (d, s, i)
    flush   : if pend: emit pend; last = pend.end; pend = none
    nothing : a target without frames never has a candidate; its best is (+inf, NO_MATCH, NO_MATCH)"""
import numpy as np

import spot_all_ref
from spot_ref import NO_MATCH


class Reporter:
    """The reporting state of one (lane, target) and the running best; `stats` counts what the rule did:
    events, replacements in step 3, candidates rejected by `last` alone."""

    def __init__(self, max_cost=None):
        self.limit = np.inf if max_cost is None else float(max_cost)
        self.pend = None                      # (cost, start, end)
        self.last = None
        self.best = (float("inf"), NO_MATCH, NO_MATCH)
        self.stats = {"events": 0, "replaced": 0, "rejected_by_last": 0}

    def _emit(self, out):
        out.append(self.pend)
        self.last = self.pend[2]
        self.pend = None
        self.stats["events"] += 1

    def rows(self, first, delta, s):
        """Consume rows first ... first + len(delta) - 1; returns the events emitted, in order."""
        out = []
        for x in range(len(delta)):
            d, st, i = float(delta[x]), int(s[x]), first + x
            if d < self.best[0]:
                self.best = (d, st, i)
            if self.pend is not None and st > self.pend[2]:
                self._emit(out)
            fits = np.isfinite(d) and d <= self.limit
            if fits and self.last is not None and not st > self.last:
                self.stats["rejected_by_last"] += 1
            if fits and (self.last is None or st > self.last):
                if self.pend is None:
                    self.pend = (d, st, i)
                elif d < self.pend[0]:
                    self.pend = (d, st, i)
                    self.stats["replaced"] += 1
        return out

    def flush(self):
        out = []
        if self.pend is not None:
            self._emit(out)
        return out


def whole_profile(source, target, squared=False):
    """(delta f64 [Fa], s int64 [Fa]) of a lane's whole source; empty arrays when either side has no frames."""
    a, b = np.asarray(source, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    return spot_all_ref.profile(a, b, squared)


def drive(delta, s, cuts, max_cost=None, flush_after=()):
    """One (lane, target): the profile of the whole, consumed push by push -- push p takes rows cuts[p] ... cuts[p+1] - 1
    (cuts ascends from 0 to the number of rows; equal neighbours are empty pushes); after every push named in flush_after
    the lane is flushed and goes on.  A target without frames has an empty profile whatever the cuts say.  Returns (events
    per push: a list of lists of (cost, start, end); the best after every push; {push: the events of the flush after it};
    the Reporter)."""
    rep = Reporter(max_cost)
    per_push, bests, flushed = [], [], {}
    n = len(delta)
    for p in range(len(cuts) - 1):
        lo, hi = min(int(cuts[p]), n), min(int(cuts[p + 1]), n)
        per_push.append(rep.rows(lo, delta[lo:hi], s[lo:hi]))
        bests.append(rep.best)
        if p in flush_after:
            flushed[p] = rep.flush()
    return per_push, bests, flushed, rep


def watch(source, target, cuts, max_cost=None, squared=False, flush_after=()):
    """drive() on the profile of (source, target)."""
    delta, s = whole_profile(source, target, squared)
    return drive(delta, s, cuts, max_cost, flush_after)
