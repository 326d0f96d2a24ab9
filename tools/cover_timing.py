#!/usr/bin/env python3
"""tools/cover_timing.py -- the cover (ssym_dtw_cover) at the reference's shape, with long sources, and against the only
route that gave the same answer before it (LAB.md).

    (a)  4096 ragged sources of 5 ... 40 frames x 13 values, one target of 4096 and one of 16 384 frames: forward ms, chain
         ms and DP cells per second (cells: 2 Fa^2 per source and start, clipped at the target's end -- what the forward
         pass computes).
    (b)  512 sources of 128 frames, a 4096-frame target.
    (c)  the earlier route at 256 ragged sources x a 512-frame target: every window (s, L) of the target as a query set
         (about 41 000 windows), ssym_pair_matrix_step(SSYM_STEP_PACED) over sources x windows (about 10 M pairs, an 84 MB
         matrix), the first minimum per window and the chain in numpy.  It uses calls that existed before the cover only, so
         its time is the same on the commit before.  The covers must agree piece for piece and bit for bit.

One MI355X, one process.  A host clock around each call, which ends in its own synchronisation: median of --reps calls
after --warmup calls; beside it the device time of the call's kernels (ssym_get_timings: main_ms, reduce_ms).

    python tools/cover_timing.py [--reps 10] [--warmup 3] [--only a4096,a16384,b,c] [--gap-cost X]

--gap-cost X times ssym_dtw_cover_gaps at that price per frame in place of ssym_dtw_cover on the same shapes; (c) then times
the call alone (the earlier route has no gaps to compare with).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine  # noqa: E402
from soundsym_amd.engine import pack_segments  # noqa: E402

INF = float("inf")
NONE = 0xFFFFFFFF


def median_ms(call, reps, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def fmt(t):
    return f"{t[0]:10.3f} ms [{t[1]:.3f} ... {t[2]:.3f}]"


def forward_cells(fa, frames):
    """Cells the forward pass computes: per source and start, Fa rows x min(2 Fa, frames left) columns."""
    total = 0.0
    left = np.arange(frames, 0, -1, dtype=np.float64)
    for f in np.unique(fa):
        total += float((fa == f).sum()) * float(f) * float(np.minimum(2.0 * f, left).sum())
    return total


def shape(name, src, target, dim, reps, warmup, penalty=0.0, gap_cost=None):
    e = Engine(metric="dtw", dtype="f32")
    d, q = e.dictionary(*pack_segments(src, dim, np.float32), dim), e.queries(*pack_segments([target], dim, np.float32), dim)
    fa = np.array([s.shape[0] for s in src])
    cells = forward_cells(fa, target.shape[0])
    call = lambda: e.dtw_cover(d, q, penalty, gap_cost=gap_cost)
    t = median_ms(call, reps, warmup)
    count, total = call()[:2]
    tm = e.timings()
    print(f"{name}: {len(src)} sources x {target.shape[0]} frames, {cells:.3e} cells: cover {fmt(t)}  forward {tm['main_ms']:.3f} ms  "
          f"chain {tm['reduce_ms']:.3f} ms  {cells / tm['main_ms'] * 1e-6:7.2f} Gcell/s  ({int(count[0])} pieces, "
          f"{total[0] / target.shape[0]:.4f} per frame)", flush=True)
    e.close()


def earlier_route(e, d, src, target, dim, penalty):
    """Every window as a query, the paced matrix, the first minimum per window and the chain on the host."""
    T, width = target.shape[0], 2 * max(s.shape[0] for s in src)
    wins = [(s, L) for s in range(T) for L in range(1, min(width, T - s) + 1)]
    q = e.queries(*pack_segments([target[s:s + L] for s, L in wins], dim, np.float32), dim)
    mat = e.pair_matrix(d, q, step="paced")
    q.close()
    key = np.where(np.isfinite(mat), mat, INF)
    first = key.argmin(axis=0)                                      # the first minimum: the lower index on a tie
    m = key[first, np.arange(len(wins))]
    M = np.full((T, width), INF)
    S = np.full((T, width), NONE, dtype=np.uint32)
    ws, wl = np.array([w[0] for w in wins]), np.array([w[1] for w in wins])
    ok = m < INF
    M[ws[ok], wl[ok] - 1], S[ws[ok], wl[ok] - 1] = m[ok], first[ok]
    best = np.full(T + 1, INF)
    best[0] = 0.0
    back = [None] * T
    for end in range(T):
        held, pick = INF, None
        for L in range(1, min(end + 1, width) + 1):
            s = end - L + 1
            if S[s, L - 1] == NONE:
                continue
            v = (float(M[s, L - 1]) + penalty) + float(best[s])
            if v < held:
                held, pick = v, (L, int(S[s, L - 1]), float(M[s, L - 1]))
        best[end + 1], back[end] = held, pick
    pieces, end = [], T - 1
    while np.isfinite(best[T]) and end >= 0:
        L, s, c = back[end]
        pieces.append((s, end - L + 1, end, c))
        end -= L
    return pieces[::-1], float(best[T]), len(wins)


def against_the_earlier_route(src, target, dim, reps, warmup, penalty=0.0, gap_cost=None):
    e = Engine(metric="dtw", dtype="f32")
    d = e.dictionary(*pack_segments(src, dim, np.float32), dim)

    def new():
        q = e.queries(*pack_segments([target], dim, np.float32), dim)       # (the upload is part of both routes)
        out = e.dtw_cover(d, q, penalty, gap_cost=gap_cost)
        q.close()
        return out
    t_new = median_ms(new, reps, warmup)
    count, total, s, a, b, c = new()
    tm = e.timings()
    if gap_cost is not None:
        gaps = int((s[:int(count[0])] == 0xFFFFFFFE).sum())
        print(f"(c) {len(src)} sources x {target.shape[0]} frames, gap_cost {gap_cost}: cover with gaps {fmt(t_new)} (forward "
              f"{tm['main_ms']:.3f}, chain {tm['reduce_ms']:.3f})  {gaps} gap frames", flush=True)
        e.close()
        return
    old = lambda: earlier_route(e, d, src, target, dim, penalty)
    t_old = median_ms(old, max(3, reps // 3), 1)
    pieces, old_total, windows = old()
    got = [(int(s[k]), int(a[k]), int(b[k]), float(c[k])) for k in range(int(count[0]))]
    same = (len(got) == len(pieces) and all(g[:3] == p[:3] and np.float64(g[3]).view(np.uint64) == np.float64(p[3]).view(np.uint64)
                                            for g, p in zip(got, pieces))
            and np.float64(total[0]).view(np.uint64) == np.float64(old_total).view(np.uint64))
    print(f"(c) {len(src)} sources x {target.shape[0]} frames: cover {fmt(t_new)} (forward {tm['main_ms']:.3f}, chain "
          f"{tm['reduce_ms']:.3f})  earlier route ({windows} windows, {len(src) * windows} pairs) {fmt(t_old)}  "
          f"new / earlier {t_new[0] / t_old[0]:.5f}  covers agree piece for piece and bit for bit: {same}", flush=True)
    e.close()
    if not same:
        raise SystemExit("the cover differs from the earlier route")
    if t_new[0] > t_old[0]:
        raise SystemExit("the cover is slower than the earlier route")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="a4096,a16384,b,c")
    ap.add_argument("--gap-cost", type=float, default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))
    rng = np.random.default_rng(0x5EED0C07)
    mk = lambda f, dim: rng.standard_normal((f, dim)).astype(np.float32)
    ragged = lambda count: [mk(int(f), 13) for f in rng.integers(5, 41, size=count)]
    src = ragged(4096)
    if "a4096" in only:
        shape("(a) ragged 5...40 f x 13 d", src, mk(4096, 13), 13, args.reps, args.warmup, gap_cost=args.gap_cost)
    if "a16384" in only:
        shape("(a) ragged 5...40 f x 13 d", src, mk(16384, 13), 13, args.reps, args.warmup, gap_cost=args.gap_cost)
    if "b" in only:
        shape("(b) 128 f x 13 d", [mk(128, 13) for _ in range(512)], mk(4096, 13), 13, args.reps, args.warmup,
              gap_cost=args.gap_cost)
    if "c" in only:
        against_the_earlier_route(ragged(256), mk(512, 13), 13, args.reps, args.warmup, gap_cost=args.gap_cost)


if __name__ == "__main__":
    main()
