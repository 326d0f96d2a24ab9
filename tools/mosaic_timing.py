#!/usr/bin/env python3
"""tools/mosaic_timing.py -- the mosaic (ssym_dtw_mosaic) on the family's yardstick and on one compute unit (DESIGN.md 5.25,
LAB.md).

    (a)  256 targets of 512 frames against four 4096-frame recordings x 13 values, beside ssym_spot_queries_step(
         SSYM_STEP_PACED) on the same two sets: both evaluate G x F = 16 384 x 131 072 cells, so the ratio of the two times
         is a ratio over equal cells.  The two calls alternate in one process.
    (b)  one target of 4096 frames against the same 16 384 source frames: one workgroup, one compute unit.

One MI355X, one process.  A host clock around each call, which ends in its own synchronisation: median of --reps calls after
--warmup calls; beside it the device time of the call's kernels (ssym_get_timings: main_ms) and cells per second over it.

    python tools/mosaic_timing.py [--reps 5] [--warmup 2] [--only a,b] [--penalty 1.0] [--gap-cost X]
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


def timed(call):
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def fmt(ts):
    ts = np.array(ts)
    return f"{float(np.median(ts)):10.3f} ms [{ts.min():.3f} ... {ts.max():.3f}]"


def planted(rng, recs, frames, dim):
    """A target of `frames` frames: spans of the recordings, copied or doubled, with a little noise."""
    parts, left = [], frames
    while left > 0:
        a = recs[int(rng.integers(len(recs)))]
        n = int(min(left, rng.integers(20, 120)))
        at = int(rng.integers(0, a.shape[0] - n))
        part = a[at:at + n] if rng.integers(2) else np.repeat(a[at:at + (n + 1) // 2], 2, axis=0)[:n]
        parts.append(part)
        left -= part.shape[0]
    x = np.concatenate(parts, axis=0)
    return (x + 1e-3 * rng.standard_normal(x.shape)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="a,b")
    ap.add_argument("--penalty", type=float, default=1.0)
    ap.add_argument("--gap-cost", type=float, default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))
    dim = 13
    rng = np.random.default_rng(0x5EED305A)
    recs = [rng.standard_normal((4096, dim)).astype(np.float32) for _ in range(4)]
    G = sum(a.shape[0] for a in recs)
    e = Engine(metric="dtw", dtype="f32")
    d = e.dictionary(*pack_segments(recs, dim, np.float32), dim)
    if "a" in only:
        tgt = [planted(rng, recs, 512, dim) for _ in range(256)]
        q = e.queries(*pack_segments(tgt, dim, np.float32), dim)
        cells = float(G) * 512 * 256
        mosaic = lambda: e.dtw_mosaic(d, q, args.penalty, args.gap_cost)
        spot = lambda: e.spot_queries(d, q, step="paced")
        for _ in range(args.warmup):
            mosaic(), spot()
        tm_, ts_, dm, ds = [], [], [], []
        for _ in range(args.reps):                           # alternating: the two see the same machine
            tm_.append(timed(mosaic))
            dm.append(e.timings()["main_ms"])
            launches = e.timings()["main_launches"]
            ts_.append(timed(spot))
            ds.append(e.timings()["total_ms"])
        count, total = mosaic()[:2]
        print(f"(a) 256 targets x 512 frames against 4 x 4096 frames, {cells:.3e} cells each:", flush=True)
        print(f"    mosaic {fmt(tm_)}  kernels {float(np.median(dm)):.3f} ms in {launches} rounds  "
              f"{cells / float(np.median(dm)) * 1e-6:7.2f} Gcell/s  ({float(count.mean()):.1f} pieces per target, "
              f"{float(total.mean()) / 512:.4f} per frame)", flush=True)
        print(f"    paced spot_queries {fmt(ts_)}  device {float(np.median(ds)):.3f} ms  "
              f"{cells / float(np.median(ds)) * 1e-6:7.2f} Gcell/s", flush=True)
        print(f"    mosaic / spot over equal cells: {float(np.median(tm_)) / float(np.median(ts_)):.3f} (host clock), "
              f"{float(np.median(dm)) / float(np.median(ds)):.3f} (device)", flush=True)
        q.close()
    if "b" in only:
        x = planted(rng, recs, 4096, dim)
        q = e.queries(*pack_segments([x], dim, np.float32), dim)
        cells = float(G) * 4096
        mosaic = lambda: e.dtw_mosaic(d, q, args.penalty, args.gap_cost)
        for _ in range(args.warmup):
            mosaic()
        ts, dm = [], []
        for _ in range(args.reps):
            ts.append(timed(mosaic))
            dm.append(e.timings()["main_ms"])
        count, total = mosaic()[:2]
        med = float(np.median(dm))
        print(f"(b) one target of 4096 frames against {G} source frames, {cells:.3e} cells, one workgroup: mosaic {fmt(ts)}  "
              f"kernels {med:.3f} ms  {med / 4096 * 1e3:.2f} us per column  {cells / med * 1e-6:7.2f} Gcell/s  "
              f"({int(count[0])} pieces, {float(total[0]) / 4096:.4f} per frame)", flush=True)
        q.close()
    e.close()


if __name__ == "__main__":
    main()
