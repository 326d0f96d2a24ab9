"""Plain numpy restatement of the live cover ("Live cover") -- TEST INFRASTRUCTURE, the reference the
coverer (ssym_coverer_*) is held to.  It is plain and recomputes freely: a lane keeps every frame it consumed and every
best(e) and back-pointer, and asks cover_ref.tables for the windows again at every push.

c, w, M, src, best, the tie rules and the arithmetic are those of "Cover" (tests/cover_ref.py), word for word.  For one lane,
X is everything consumed so far and n its frame count, W = 2 max(Fmax, 1):

    resume   : consuming frames n ... n+m-1 computes M(s,L) for every window that ends in them (s >= n-W+1) and best(e) and
               the back-pointers for e = n ... n+m-1, exactly as "Cover" does
    horizon  : H(n) = { e : max(-1, n-W) <= e <= n-1, best(e) finite }   (-1 belongs to it while n < W)
    walk(e)  : the pieces the back-pointers give from e down to -1, in ascending start   (walk(-1) is empty)
    commit   : C(n) = the longest common prefix of walk(e) over e in H(n); H(n) empty: nothing new.
               A push emits the pieces of C(n) not emitted before, and done = the end of the last of them.
    flush    : emits the pieces of walk(lastFinite) not emitted before; the lane has then ended
    best     : total = best(n-1) (+inf for n = 0 or when not finite), covered = lastFinite + 1, committed = done + 1
"""
import numpy as np

import cover_ref

INF = float("inf")
NONE = cover_ref.NONE
BACK_MIN = 1024                                          # frames of the back-pointer ring at creation


def width(src):
    return 2 * max([np.asarray(a).shape[0] for a in src] + [1])


def chain_step(M, S, lo, e, best, penalty):
    """best(e) and its back-pointer (L, src, M) -- cover_ref.chain's step -- from tables that start at target frame lo."""
    W = M.shape[1]
    held, pick = INF, None
    for L in range(1, min(e + 1, W) + 1):
        s = e - L + 1
        if s < lo or S[s - lo, L - 1] == NONE:
            continue
        v = (float(M[s - lo, L - 1]) + penalty) + float(best[s])
        if v < held:
            held, pick = v, (L, int(S[s - lo, L - 1]), float(M[s - lo, L - 1]))
    return held, pick


class Lane:
    """One growing target.  push / flush return the pieces [(src, start, end, cost)] they emit, in ascending start."""

    def __init__(self, src, penalty=0.0, squared=False):
        self.src, self.penalty, self.squared = src, float(penalty), squared
        self.W = width(src)
        self.x = None                                    # every frame consumed
        self.best = [0.0]                                # best[e + 1]
        self.back = []                                   # back[e]
        self.done, self.last_finite, self.ended = -1, -1, False
        self.emitted = []
        self.stretch = 0                                 # the largest uncommitted stretch n - 1 - done after a push

    @property
    def n(self):
        return 0 if self.x is None else self.x.shape[0]

    def walk_ends(self, e, stop=-1):
        """The ends of the pieces of walk(e) beyond `stop`, ascending.  Every walk the lane takes passes through done (what
        is committed is shared by every end of the horizon and by lastFinite): the assertion holds that."""
        ends = []
        while e > stop:
            ends.append(e)
            e -= self.back[e][0]
        assert e == stop, (e, stop)
        return ends[::-1]

    def _emit(self, upto):
        """The pieces of walk(upto) beyond done."""
        out = []
        for e in self.walk_ends(upto, self.done):
            L, s, m = self.back[e]
            out.append((s, e - L + 1, e, m))
        if out:
            self.done = out[-1][2]
        self.emitted += out
        return out

    def horizon(self):
        n = self.n
        return [e for e in range(max(-1, n - self.W), n) if np.isfinite(self.best[e + 1])]

    def push(self, frames):
        frames = np.asarray(frames, dtype=np.float64)
        if frames.shape[0] == 0:
            return []
        assert not self.ended, "the lane has ended"
        n = self.n
        self.x = frames.copy() if self.x is None else np.concatenate([self.x, frames], axis=0)
        lo = max(0, n - self.W + 1)
        M, S = cover_ref.tables(self.src, self.x[lo:], self.squared)
        for e in range(n, self.n):
            held, pick = chain_step(M, S, lo, e, self.best, self.penalty)
            self.best.append(held)
            self.back.append(pick)
            if np.isfinite(held):
                self.last_finite = e
        out = []
        walks = [self.walk_ends(e, self.done) for e in self.horizon()]
        if walks:
            k = 0
            while all(len(w) > k for w in walks) and len({w[k] for w in walks}) == 1:
                k += 1
            if k:
                out = self._emit(walks[0][k - 1])
        self.stretch = max(self.stretch, self.n - 1 - self.done)
        return out

    def flush(self):
        out = self._emit(self.last_finite) if self.last_finite > self.done else []
        self.ended = True
        return out

    def total(self):
        return float(self.best[self.n]) if self.n and np.isfinite(self.best[self.n]) else INF

    def state(self):
        """(total, covered, committed): what ssym_coverer_best reports."""
        return self.total(), self.last_finite + 1, self.done + 1


def run(src, x, cuts, penalty=0.0, squared=False, flush=True):
    """One lane fed x[cuts[i]:cuts[i+1]]: (the pieces each push emitted, the flush's pieces or None, the lane)."""
    lane = Lane(src, penalty, squared)
    per_push = [lane.push(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return per_push, (lane.flush() if flush else None), lane


def capacity(stretches_and_slices, initial=BACK_MIN):
    """The back-pointer ring's capacity by the rule of consequence 7: a power of two, `initial` at first, grown to the next
    power of two that holds (uncommitted stretch + slice) whenever that would not fit.  `initial` is rounded up to a power
    of two as the store is.  stretches_and_slices: per slice, the largest over the lanes that consume frames of (uncommitted
    frames before the slice + frames of the slice)."""
    cap = 1
    while cap < initial:
        cap *= 2
    for need in stretches_and_slices:
        while cap < need:
            cap *= 2
    return cap
