"""Plain numpy restatement of the mosaic ("Mosaic") -- TEST INFRASTRUCTURE, the reference
ssym_dtw_mosaic is held to.

c, the squared option and the arithmetic are those of "Paced spotting" (tests/paced_ref.py), word for word.  The
dictionary's segments are laid end to end: g = 0 ... G-1 is a global source frame, seg(g) its segment, pos(g) its frame
within it; empty segments contribute nothing.  Every cell has the states N and H of the paced pattern.  For one target X of
T frames:

    best(-1) = 0
    column j = 0 ... T-1:
      S      = piece_penalty + best(j-1)                              (the price of opening a piece at column j)
      P(g)   = E(g-1, j-1) if pos(g) >= 1, else +inf
               if pos(g) >= 2 and E(g-2, j-1) < P: E(g-2, j-1)         (strict <; j = 0: P = +inf)
      open(g)= not (P(g) <= S)                                        (a tie continues the piece; a NaN P opens)
      Q      = S if open(g) else P(g)
      H(g,j) = c(g,j) + N(g,j-1)                                      (+inf at j = 0)
      N(g,j) = c(g,j) + Q
      E(g,j) = N(g,j); if H(g,j) < N(g,j): H(g,j)                     (strict <: a tie keeps N)
      (v,arg)= the first least E(g,j) over g ascending from (+inf, none), strict <   (NaN and +inf never win)
      vg     = gap_cost + best(j-1);  if vg < v (strict): best(j) = vg, arg(j) = GAP;  else best(j) = v, arg(j) = arg
    total    = best(T-1);  no mosaic: T = 0, or total not finite -> count 0, total +inf
    backward : j = T-1, at arg(j).  GAP: frame j is a gap frame, go to arg(j-1).  Otherwise the state is H if H < N there,
               else N.  State H at (g,j): the cell before is (g, j-1) in state N.  State N at (g,j): if open(g) at column
               j, a piece starts here, go to arg(j-1); else the cell before is (g-2, j-1) if the P rule took it, else
               (g-1, j-1), in its E state.

A column depends on the column before it alone and every operation is elementwise IEEE f64, so a whole column at once has
the bits of the cell-by-cell loop; the comparisons are np.where on strict <, never np.minimum (paced_ref.profile)."""
import numpy as np

from dtw_path_ref import local_costs
from paced_ref import _down

INF = float("inf")
NONE = 0xFFFFFFFF
GAP = 0xFFFFFFFE
DIAGONAL, SKIP, OPEN = 0, 1, 2


def layout(segs, dim=None):
    """(A [G, dim] the segments end to end, seg int64 [G], pos int64 [G])."""
    segs = [np.asarray(a, dtype=np.float64) for a in segs]
    if dim is None:
        dim = max([a.shape[1] for a in segs if a.ndim == 2] + [1])
    segs = [a.reshape(-1, dim) for a in segs]
    A = np.concatenate(segs, axis=0) if segs else np.zeros((0, dim))
    seg = np.concatenate([np.full(a.shape[0], k, dtype=np.int64) for k, a in enumerate(segs)] + [np.zeros(0, dtype=np.int64)])
    pos = np.concatenate([np.arange(a.shape[0], dtype=np.int64) for a in segs] + [np.zeros(0, dtype=np.int64)])
    return A, seg, pos


def forward(segs, x, penalty=0.0, gap_cost=INF, squared=False):
    """(best f64 [T], arg int64 [T] (a g, GAP or NONE), rep bool [G, T] (H < N), code int8 [G, T], c [G, T])."""
    x = np.asarray(x, dtype=np.float64)
    A, _, pos = layout(segs, x.shape[1] if x.ndim == 2 else None)
    G, T = A.shape[0], x.shape[0]
    penalty, gap_cost = float(penalty), float(gap_cost)
    c = local_costs(A, x.reshape(T, A.shape[1]), squared)
    best, arg = np.full(T, INF), np.full(T, NONE, dtype=np.int64)
    rep, code = np.zeros((G, T), dtype=bool), np.zeros((G, T), dtype=np.int8)
    e, n, before = np.full(G, INF), np.full(G, INF), 0.0
    with np.errstate(invalid="ignore"):
        for j in range(T):
            S = penalty + before
            p = np.where(pos >= 1, _down(e, 1, INF), INF)
            p2 = _down(e, 2, INF)
            skip = (pos >= 2) & (p2 < p)
            p = np.where(skip, p2, p)
            opened = ~(p <= S)
            q = np.where(opened, S, p)
            h = c[:, j] + n if j else np.full(G, INF)
            n = c[:, j] + q
            rep[:, j] = h < n
            e = np.where(rep[:, j], h, n)
            code[:, j] = np.where(opened, OPEN, np.where(skip, SKIP, DIAGONAL))
            v, a = INF, NONE
            wins = e < INF                                   # NaN and +inf never win
            if wins.any():
                a = int(np.where(wins, e, INF).argmin())     # argmin: the first of the least
                v = float(e[a])
            vg = gap_cost + before
            if vg < v:
                v, a = vg, GAP
            best[j], arg[j] = v, a
            before = v
    return best, arg, rep, code, c


def backward(arg, rep, code):
    """(gmap int64 [T]: the global source frame of every target frame or GAP, starts: the frames at which a piece or a gap
    frame starts, ascending); only for a finite total."""
    T = arg.shape[0]
    gmap, starts = np.zeros(T, dtype=np.int64), []
    j, g, force_n = T - 1, int(arg[T - 1]), False
    while j >= 0:
        if g == GAP:
            gmap[j] = GAP
            starts.append(j)
            g, force_n = (int(arg[j - 1]) if j else NONE), False
        elif rep[g, j] and not force_n:
            gmap[j] = g
            force_n = True
        else:
            gmap[j], force_n = g, False
            if code[g, j] == OPEN:
                starts.append(j)
                g = int(arg[j - 1]) if j else NONE
            else:
                g = g - 2 if code[g, j] == SKIP else g - 1
        j -= 1
    return gmap, starts[::-1]


def mosaic(segs, x, penalty=0.0, gap_cost=INF, squared=False):
    """(total, gmap, starts, frame_cost) of one target; (+inf, None, None, None) without a mosaic."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return INF, None, None, None
    best, arg, rep, code, c = forward(segs, x, penalty, gap_cost, squared)
    if not np.isfinite(best[-1]):
        return INF, None, None, None
    gmap, starts = backward(arg, rep, code)
    cost = np.array([float(gap_cost) if g == GAP else c[g, j] for j, g in enumerate(gmap)])
    return float(best[-1]), gmap, starts, cost


def arrays(segs, targets, penalty=0.0, gap_cost=INF, squared=False):
    """What ssym_dtw_mosaic returns for a query set: (count, total, start, src, frame, frame_cost)."""
    off = np.concatenate([[0], np.cumsum([np.asarray(x).shape[0] for x in targets])]).astype(np.int64)
    F, m = int(off[-1]), len(targets)
    dim = max([np.asarray(a).shape[1] for a in list(segs) + list(targets) if np.asarray(a).ndim == 2] + [1])
    _, seg, pos = layout(segs, dim)
    count, total = np.zeros(m, dtype=np.uint32), np.full(m, INF)
    start, src, frame = (np.full(F, NONE, dtype=np.uint32) for _ in range(3))
    cost = np.full(F, INF)
    for t, x in enumerate(targets):
        x = np.asarray(x, dtype=np.float64).reshape(-1, dim)
        total[t], gmap, starts, fc = mosaic(segs, x, penalty, gap_cost, squared)
        if gmap is None:
            continue
        count[t] = len(starts)
        start[off[t]:off[t] + len(starts)] = starts
        gap = gmap == GAP
        at = np.where(gap, 0, gmap)
        src[off[t]:off[t + 1]] = np.where(gap, GAP, seg[at] if seg.size else 0)
        frame[off[t]:off[t + 1]] = np.where(gap, NONE, pos[at] if pos.size else 0)
        cost[off[t]:off[t + 1]] = fc
    return count, total, start, src, frame, cost


def pieces_of(got, off, t):
    """[(src, first, last, start, end)] of target t from the six arrays, one (GAP, NONE, NONE, j, j) per gap frame."""
    count, _, start, src, frame, _ = got
    a, T = int(off[t]), int(off[t + 1] - off[t])
    cuts = [int(s) for s in start[a:a + int(count[t])]] + [T]
    return [(int(src[a + s]), int(frame[a + s]), int(frame[a + e - 1]), s, e - 1) for s, e in zip(cuts[:-1], cuts[1:])]


def resum(start, src, frame_cost, penalty=0.0):
    """acc = 0; a frame that opens a piece: acc = c + (piece_penalty + acc); one that continues a piece: acc = c + acc; a gap
    frame: acc = gap_cost + acc -- the recurrence's own additions.  start: the starts of one target; src, frame_cost: its
    frames."""
    opens, acc = set(int(s) for s in start if int(s) != NONE), 0.0
    for j, cj in enumerate(frame_cost):
        if int(src[j]) == GAP:
            acc = float(cj) + acc
        elif j in opens:
            acc = float(cj) + (float(penalty) + acc)
        else:
            acc = float(cj) + acc
    return acc


def tiles(start, src, frame, seg_frames, T):
    """Consequence (1): the starts ascend from 0, every gap frame is a start, and within a piece the source frame stays in
    one segment, advances by 0, 1 or 2 per target frame and never by 0 twice in a row."""
    starts = [int(s) for s in start if int(s) != NONE]
    if T == 0:
        return not starts
    if not starts or starts[0] != 0 or any(b <= a for a, b in zip(starts[:-1], starts[1:])) or starts[-1] >= T:
        return False
    opens = set(starts)
    for j in range(T):
        if int(src[j]) == GAP:
            if j not in opens:
                return False
            continue
        if not (0 <= int(frame[j]) < seg_frames[int(src[j])]):
            return False
        if j in opens:
            continue
        step = int(frame[j]) - int(frame[j - 1])
        if int(src[j - 1]) != int(src[j]) or step not in (0, 1, 2):
            return False
        if step == 0 and j - 1 not in opens and int(frame[j - 1]) == int(frame[j - 2]):
            return False
    return True


def brute_force(segs, x, penalty=0.0, gap_cost=INF, squared=False):
    """The least total over EVERY mosaic of x: every frame a gap frame, the opening of a piece at any source frame, or the
    continuation of the piece before it by 0 (not twice in a row), 1 or 2 source frames inside the segment, each mosaic
    summed in frame order with resum's additions; +inf when none has a finite sum."""
    x = np.asarray(x, dtype=np.float64)
    A, seg, pos = layout(segs, x.shape[1] if x.ndim == 2 else None)
    G, T = A.shape[0], x.shape[0]
    penalty, gap_cost = float(penalty), float(gap_cost)
    c = local_costs(A, x.reshape(T, A.shape[1]), squared)
    best = INF

    def go(j, acc, g, repeated):
        nonlocal best
        if j == T:
            if acc < best:
                best = acc
            return
        if gap_cost < INF:
            go(j + 1, gap_cost + acc, -1, False)
        for k in range(G):
            go(j + 1, c[k, j] + (penalty + acc), k, False)
        if g >= 0:
            if not repeated:
                go(j + 1, c[g, j] + acc, g, True)
            for k in (g + 1, g + 2):
                if k < G and seg[k] == seg[g]:
                    go(j + 1, c[k, j] + acc, k, False)

    if T:
        go(0, 0.0, -1, False)
    return best


def _real(rng, shape):
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)     # (f32 values: both engine dtypes hold them)


PLANTED = ((1, 5, 14, "copy"), (0, 20, 25, "doubled"), (2, 3, 19, "second"))


def _span(a, first, last, kind):
    part = a[first:last + 1]
    return part if kind == "copy" else np.repeat(part, 2, axis=0) if kind == "doubled" else part[::2]


def planted_case(noise=0.0, seed=0x305A1C, dim=13, plan=PLANTED):
    """Three recordings of 40 / 33 / 50 frames x dim values; the target concatenates span 5 ... 14 of recording 1 as a copy,
    span 20 ... 25 of recording 0 with every frame doubled and every second frame of span 3 ... 19 of recording 2.  noise > 0:
    that much Gaussian noise on the target (rounded to f32 values).
    Returns (recordings, target, planted pieces [(src, first, last, start, end)])."""
    rng = np.random.default_rng(seed)
    recs = [_real(rng, (n, dim)) for n in (40, 33, 50)]
    parts, pieces, at = [], [], 0
    for s, first, last, kind in plan:
        part = _span(recs[s], first, last, kind)
        parts.append(part)
        pieces.append((s, first, last, at, at + part.shape[0] - 1))
        at += part.shape[0]
    target = np.concatenate(parts, axis=0)
    if noise:
        target = (target + noise * rng.standard_normal(target.shape)).astype(np.float32).astype(np.float64)
    return recs, target, pieces


def intruder_case(frames=4, offset=100.0, dim=13):
    """The first two planted pieces with `frames` frames of the same kind of values, moved by +offset in every coordinate,
    inserted at their join: (recordings, target, the planted pieces at their new cuts, (first, last) intruder frame).  At
    penalty 1 and gap_cost 1.5 the mosaic is the two pieces around four gap frames: total 2 + 4 x 1.5 = 8."""
    recs, target, pieces = planted_case(dim=dim, plan=PLANTED[:2])
    at = pieces[1][3]
    rng = np.random.default_rng(0x6A95)
    block = _real(rng, (frames, dim)) + float(offset)
    block = block.astype(np.float32).astype(np.float64)
    x = np.concatenate([target[:at], block, target[at:]], axis=0)
    s, first, last, a, b = pieces[1]
    return recs, x, [pieces[0], (s, first, last, a + frames, b + frames)], (at, at + frames - 1)


def boundary_case(dim=13, seed=0xB0DA):
    """Two segments of 6 and 5 frames; the target is the last frame of segment 0 followed by the first of segment 1 -- which
    are neighbours in the global numbering.  The mosaic must be two pieces of one frame, total 2 x penalty exactly, never
    one piece across the boundary (which would cost one penalty).  (segments, target, pieces [(src, first, last, start, end)])."""
    rng = np.random.default_rng(seed)
    segs = [64.0 * _real(rng, (6, dim)), 64.0 * _real(rng, (5, dim))]      # (so far apart that no repeat is worth a penalty)
    x = np.stack([segs[0][-1], segs[1][0]])
    return segs, x, [(0, 5, 5, 0, 0), (1, 0, 0, 1, 1)]
