"""Plain numpy restatement of the live mosaic ("Live mosaic") -- TEST INFRASTRUCTURE, the reference
ssym_mosaicker_* is held to.  c, S, P, open, Q, H, N, E, best, arg, the tie rules and the arithmetic are those of "Mosaic"
(tests/mosaic_ref.py), word for word: the columns come from mosaic_ref.forward, and a column depends on the columns before
it alone, so the forward pass of the whole X holds the forward pass of every prefix.

    key      : a position of the backward walk at column j: (g, H), (g, N) or GAP.  A walk steps from a key at column j to
               one at column j-1 by the "backward" rule of "Mosaic"; two walks that share a key at a column are the same
               from there back.
    live(n)  : S' = piece_penalty + best(n-1).  Every g with E(g, n-1) finite and <= S' in the state that bit 0 says (H if
               H < N, else N); every g whose bit 0 is set and whose N(g, n-1) is finite and <= S', in state N; GAP if
               arg(n-1) = GAP and best(n-1) is finite.  NaN is never live.
    commit   : c(n) = the largest column <= n-1 at which all walks of live(n) hold the same key, -1 if there is none;
               unchanged when live(n) is empty.
    flush    : the walk from arg(lastFinite) at column lastFinite.

rule: "full" is the definition; "no_n" (no N-state hypotheses) and "arg_only" (arg(n-1) alone) are the weakened rules the
tests show to be revised."""
import numpy as np

import mosaic_ref
from mosaic_ref import GAP, INF, NONE, OPEN, SKIP

H, N = 1, 0
GAPKEY = (GAP, N)


class Columns:
    """The forward pass of X with E and N of every column (rebuilt from the direction bytes with the recurrence's own
    additions, so they have its bits)."""

    def __init__(self, segs, x, penalty=0.0, gap_cost=INF, squared=False):
        x = np.asarray(x, dtype=np.float64)
        self.segs, self.penalty, self.gap_cost = segs, float(penalty), float(gap_cost)
        self.best, self.arg, self.rep, self.code, self.c = mosaic_ref.forward(segs, x, penalty, gap_cost, squared)
        G, T = self.rep.shape
        self.G, self.T = G, T
        _, self.seg, self.pos = mosaic_ref.layout(segs, x.shape[1] if x.ndim == 2 else None)
        self.E, self.N = np.full((G, T), INF), np.full((G, T), INF)
        e, n, before = np.full(G, INF), np.full(G, INF), 0.0
        g = np.arange(G)
        with np.errstate(invalid="ignore"):
            for j in range(T):
                S = self.penalty + before
                prev = e[np.maximum(g - 1 - (self.code[:, j] == SKIP), 0)] if G else e
                q = np.where(self.code[:, j] == OPEN, S, prev)
                h = self.c[:, j] + n if j else np.full(G, INF)
                n = self.c[:, j] + q
                e = np.where(self.rep[:, j], h, n)
                self.E[:, j], self.N[:, j] = e, n
                before = self.best[j]

    def key_e(self, g, j):
        """the key of source frame g (or GAP) at column j in its E state"""
        g = int(g)
        return GAPKEY if g == GAP else (g, H if self.rep[g, j] else N)

    def back(self, key, j):
        """the key at column j-1 of the walk that holds `key` at column j >= 1"""
        g, s = key
        if g == GAP:
            return self.key_e(self.arg[j - 1], j - 1)
        if s == H:
            return (g, N)
        if self.code[g, j] == OPEN:
            return self.key_e(self.arg[j - 1], j - 1)
        return self.key_e(g - 2 if self.code[g, j] == SKIP else g - 1, j - 1)

    def starts(self, key, j):
        g, s = key
        return g == GAP or (s == N and (self.code[g, j] == OPEN or j == 0))

    def live(self, n, rule="full"):
        """the keys of live(n) at column n-1 (n >= 1)"""
        j = n - 1
        if not np.isfinite(self.best[j]):
            return set()
        if rule == "arg_only":
            return {self.key_e(self.arg[j], j)}
        S = self.penalty + self.best[j]
        keys = set()
        with np.errstate(invalid="ignore"):
            for g in np.nonzero(np.isfinite(self.E[:, j]) & (self.E[:, j] <= S))[0]:
                keys.add(self.key_e(g, j))
            if rule != "no_n":
                for g in np.nonzero(self.rep[:, j] & np.isfinite(self.N[:, j]) & (self.N[:, j] <= S))[0]:
                    keys.add((int(g), N))
        if int(self.arg[j]) == GAP:
            keys.add(GAPKEY)
        return keys

    def commit(self, n, before=-1, rule="full"):
        """(c(n), the key at it or None); before: c(n-1), kept when live(n) is empty"""
        keys = self.live(n, rule)
        if not keys:
            return before, None
        j = n - 1
        while len(keys) > 1 and j > 0:
            keys = {self.back(k, j) for k in keys}
            j -= 1
        if len(keys) > 1:
            return -1, None
        return j, next(iter(keys))

    def walk(self, key, j):
        """{column: key} of the walk that holds `key` at column j, down to column 0"""
        out = {j: key}
        while j > 0:
            key = self.back(key, j)
            j -= 1
            out[j] = key
        return out

    def offline(self, n):
        """the walk of the mosaic of X[:n], or None without one"""
        if n == 0 or not np.isfinite(self.best[n - 1]):
            return None
        return self.walk(self.key_e(self.arg[n - 1], n - 1), n - 1)

    def last_finite(self, n):
        fin = np.nonzero(np.isfinite(self.best[:n]))[0]
        return int(fin[-1]) if fin.size else -1

    def frame(self, key, j):
        """(column, src, frame, cost, start) as the mosaicker emits frame j"""
        g, _ = key
        if g == GAP:
            return (j, GAP, NONE, self.gap_cost, True)
        return (j, int(self.seg[g]), int(self.pos[g]), float(self.c[g, j]), bool(self.starts(key, j)))


def commits(segs, x, penalty=0.0, gap_cost=INF, squared=False, rule="full"):
    """[c(1), ..., c(T)]"""
    col = Columns(segs, x, penalty, gap_cost, squared)
    out, c = [], -1
    for n in range(1, col.T + 1):
        c, _ = col.commit(n, c, rule)
        out.append(c)
    return out


def revised(segs, x, penalty=0.0, gap_cost=INF, squared=False, rule="full"):
    """True if some c(n) decreases, or if the mosaic of some longer prefix X[:n'] does not hold the key committed at c(n)"""
    col = Columns(segs, x, penalty, gap_cost, squared)
    held, c = [], -1
    for n in range(1, col.T + 1):
        c2, key = col.commit(n, c, rule)
        if c2 < c:
            return True
        c = c2
        if key is not None:
            held.append((c, key))
        off = col.offline(n)
        if off is not None and any(off[j] != k for j, k in held):
            return True
    return False


class Lane:
    """One lane of a mosaicker: push frames, get the frames committed; flush gives the rest."""

    def __init__(self, segs, dim, penalty=0.0, gap_cost=INF, squared=False):
        self.segs, self.dim, self.penalty, self.gap_cost, self.squared = segs, dim, penalty, gap_cost, squared
        self.x = np.zeros((0, dim))
        self.n, self.done, self.ended = 0, -1, False
        self.col = None

    def _emit(self, key, j):
        walk = self.col.walk(key, j)
        out = [self.col.frame(walk[k], k) for k in range(self.done + 1, j + 1)]
        self.done = max(self.done, j)
        return out

    def push(self, frames):
        """[(column, src, frame, cost, start)] of the frames this push commits (c(n) after the last of them: commits
        depend on the frames consumed, not on the pushes)"""
        frames = np.asarray(frames, dtype=np.float64).reshape(-1, self.dim)
        if frames.shape[0] == 0:
            return []
        assert not self.ended
        self.x = np.concatenate([self.x, frames], axis=0)
        self.col = Columns(self.segs, self.x, self.penalty, self.gap_cost, self.squared)
        c = self.done
        for n in range(self.n + 1, self.x.shape[0] + 1):
            c2, key = self.col.commit(n, c)
            if c2 > c:
                c, tip = c2, (key, c2)
        self.n = self.x.shape[0]
        return self._emit(*tip) if c > self.done else []

    def flush(self):
        self.ended = True
        last = self.col.last_finite(self.n) if self.col is not None else -1
        if last <= self.done:
            return []
        return self._emit(self.col.key_e(self.col.arg[last], last), last)

    def best(self):
        """(total, covered, committed)"""
        if self.n == 0:
            return INF, 0, 0
        v = float(self.col.best[self.n - 1])
        return (v if np.isfinite(v) else INF), self.col.last_finite(self.n) + 1, self.done + 1


def frames_to_arrays(frames, T):
    """The six arrays of mosaic_ref.arrays for one target of T frames from the frames emitted for it (all of them, or those
    of the prefix a dead lane has a mosaic of): (count, start [T], src [T], frame [T], cost [T])."""
    start, src, frame = (np.full(T, NONE, dtype=np.uint32) for _ in range(3))
    cost = np.full(T, INF)
    starts = [f[0] for f in frames if f[4]]
    start[:len(starts)] = starts
    for j, s, f, c, _ in frames:
        src[j], frame[j], cost[j] = s, f, c
    return len(starts), start, src, frame, cost
