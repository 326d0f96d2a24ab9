"""Plain numpy restatement of the cover with gaps ("Cover with gaps") -- TEST INFRASTRUCTURE, the
reference ssym_dtw_cover_gaps and a coverer made by ssym_coverer_create_gaps are held to.

Everything of "Cover" (tests/cover_ref.py) holds word for word: c, w, M, src, the scan over L, best(-1) = 0; the tables are
cover_ref.tables.  One candidate is added to each step:

    best(e) : the scan of "Cover" gives (v, L, src, M) or (+inf, none)
              vg = gap_cost + best(e-1)
              if vg < v (strict):  best(e) = vg, back-pointer (L = 1, src = GAP, M = gap_cost)
    cover   : walk back as before; a gap frame is the piece (GAP, start = e, end = e, cost = gap_cost)
    total   : acc = 0; a piece: acc = (cost + piece_penalty) + acc; a gap frame: acc = gap_cost + acc  -> total's bits

A gap is reported frame by frame, piece_penalty is not charged on it, and a piece wins a tie against it.  gap_cost = +inf
never wins, so the cover is cover_ref's."""
import numpy as np

import cover_ref
import live_cover_ref
import paced_match_ref

INF = float("inf")
NONE = cover_ref.NONE
GAP = 0xFFFFFFFE


def with_gap(held, pick, before, gap_cost):
    """The step's result after the gap candidate: `held`, `pick` from the scan of "Cover", `before` = best(e-1)."""
    vg = float(gap_cost) + float(before)
    if vg < held:
        return vg, (1, GAP, float(gap_cost))
    return held, pick


def chain(M, S, penalty=0.0, gap_cost=INF):
    """(pieces [(src, start, end, cost)] with one (GAP, e, e, gap_cost) per gap frame, total) of the tables of one target."""
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
        best[e + 1], back[e] = with_gap(held, pick, best[e], gap_cost)
    if T == 0 or not np.isfinite(best[T]):
        return [], INF
    pieces, e = [], T - 1
    while e >= 0:
        L, s, m = back[e]
        pieces.append((s, e - L + 1, e, m))
        e -= L
    return pieces[::-1], float(best[T])


def cover(src, x, penalty=0.0, gap_cost=INF, squared=False):
    """(pieces in ascending start, total); ([], +inf) without a cover."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return [], INF
    return chain(*cover_ref.tables(src, x, squared), penalty, gap_cost)


def arrays(src, targets, penalty=0.0, gap_cost=INF, squared=False, tabs=None):
    """What ssym_dtw_cover_gaps returns for a query set: cover_ref.arrays' layout."""
    if tabs is None:
        tabs = cover_ref.all_tables(src, targets, squared)
    off = np.concatenate([[0], np.cumsum([np.asarray(x).shape[0] for x in targets])]).astype(np.int64)
    F, m = int(off[-1]), len(targets)
    count, total = np.zeros(m, dtype=np.uint32), np.full(m, INF)
    s, a, e = (np.full(F, NONE, dtype=np.uint32) for _ in range(3))
    c = np.full(F, INF)
    for t in range(m):
        pieces, total[t] = chain(*tabs[t], penalty, gap_cost) if tabs[t] is not None else ([], INF)
        count[t] = len(pieces)
        for k, (ps, pa, pe, pc) in enumerate(pieces):
            s[off[t] + k], a[off[t] + k], e[off[t] + k], c[off[t] + k] = ps, pa, pe, pc
    return count, total, s, a, e, c


def resum(pieces, penalty=0.0):
    """acc = 0; a piece: acc = (cost + piece_penalty) + acc; a gap frame: acc = gap_cost + acc -- the chain's additions."""
    acc = 0.0
    for src, _, _, cost in pieces:
        acc = (float(cost) + acc) if src == GAP else ((float(cost) + float(penalty)) + acc)
    return acc


def tiles(pieces, T):
    """True when the pieces and gap frames tile [0, T) and every gap is one frame."""
    at = 0
    for src, start, end, _ in pieces:
        if start != at or end < start or (src == GAP and end != start):
            return False
        at = end + 1
    return at == T


def merged(pieces):
    """Runs of gap frames as one (GAP, start, end, gap_cost x frames): what the Python API's Gap holds."""
    out = []
    for src, start, end, cost in pieces:
        if src == GAP and out and out[-1][0] == GAP and out[-1][2] + 1 == start:
            out[-1] = (GAP, out[-1][1], end, cost * (end - out[-1][1] + 1))
        else:
            out.append((src, start, end, cost))
    return out


def brute_force(src, x, penalty=0.0, gap_cost=INF, squared=False):
    """The least total over EVERY tiling of x by pieces and gap frames and every choice of sources, each tiling summed in
    tile order (a piece: (cost + penalty) + acc, a gap frame: gap_cost + acc), every piece cost paced_match_ref.cost on
    the cut; +inf when no tiling has a finite sum."""
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
        if float(gap_cost) < INF:
            go(s + 1, float(gap_cost) + acc)
        for e in range(s, T):
            if piece[s, e] < INF:
                go(e + 1, (piece[s, e] + float(penalty)) + acc)

    if T:
        go(0, 0.0)
    return best


class Lane(live_cover_ref.Lane):
    """live_cover_ref.Lane with the gap candidate in the step: horizon, walk, commit, flush and best are its own (a gap
    frame is a piece of one frame, and 1 <= W)."""

    def __init__(self, src, penalty=0.0, gap_cost=INF, squared=False):
        super().__init__(src, penalty, squared)
        self.gap_cost = float(gap_cost)

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
            held, pick = live_cover_ref.chain_step(M, S, lo, e, self.best, self.penalty)
            held, pick = with_gap(held, pick, self.best[e], self.gap_cost)
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


def run(src, x, cuts, penalty=0.0, gap_cost=INF, squared=False, flush=True):
    """One lane fed x[cuts[i]:cuts[i+1]]: (the pieces each push emitted, the flush's pieces or None, the lane)."""
    lane = Lane(src, penalty, gap_cost, squared)
    per_push = [lane.push(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return per_push, (lane.flush() if flush else None), lane


def intruder_case(frames=7, offset=100.0, join=3, dim=13):
    """cover_ref.planted_case() with `frames` frames of the same kind of values, moved by +offset in every coordinate,
    inserted at the join before planted piece `join`: (segments, target, the planted pieces at their new cuts, (first,
    last) intruder frame).  The values are f32 values, as the planted case's are."""
    segs, target, pieces = cover_ref.planted_case(dim=dim)
    at = pieces[join][1]
    rng = np.random.default_rng(0x6A95)
    block = (rng.standard_normal((frames, target.shape[1])) + float(offset)).astype(np.float32).astype(np.float64)
    x = np.concatenate([target[:at], block, target[at:]], axis=0)
    moved = [(s, a, b) if k < join else (s, a + frames, b + frames) for k, (s, a, b) in enumerate(pieces)]
    return segs, x, moved, (at, at + frames - 1)


def nan_case(join=4):
    """cover_ref.planted_case() with ONE all-NaN frame inserted inside the target, at the join before planted piece `join`:
    (segments, target, the planted pieces at their new cuts, the NaN frame)."""
    segs, target, pieces = cover_ref.planted_case()
    at = pieces[join][1]
    x = np.concatenate([target[:at], np.full((1, target.shape[1]), np.nan), target[at:]], axis=0)
    moved = [(s, a, b) if k < join else (s, a + 1, b + 1) for k, (s, a, b) in enumerate(pieces)]
    return segs, x, moved, at


def short_case(dim=13):
    """A 3-frame target against segments of 8, 11 and 20 frames: a segment of Fa frames covers windows of ceil((Fa+1)/2)
    frames at least, 5 here, so no window of the target has a source.  (segments, target)."""
    rng = np.random.default_rng(0x5407)
    return [cover_ref._real(rng, (n, dim)) for n in (8, 11, 20)], cover_ref._real(rng, (3, dim))


def tie_case():
    """dim 1, integer features, so every c is an exact integer: one source of two frames [0, 0] and the target [1, 1, 1, 1].
    Every window of 2 ... 4 frames costs 1 per frame exactly, which is the gap_cost to use: at e = 1, 2 and 3 a piece and the
    gap candidate tie, and the piece must win -- the cover is two pieces of two frames, total 4.  (segments, target, the
    gap_cost of the tie, the pieces [(src, start, end, cost)])."""
    return [np.zeros((2, 1))], np.ones((4, 1)), 1.0, [(0, 0, 1, 2.0), (0, 2, 3, 2.0)]
