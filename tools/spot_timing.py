#!/usr/bin/env python3
"""tools/spot_timing.py -- ssym_dtw_spot against the exact f64 kernel over the same number of DP cells (DESIGN.md 5.15,
LAB.md 5.15).

For each shape M targets are spotted in ONE recording of 16 384 frames (M pairs, 16 384 x Fb cells each).  The yardstick:
the same recording cut into 128 segments of 128 frames, every segment against the same targets with the exact kernel
(ssym_match_queries with SSYM_DTW_FORCE_EXACT: 128 x M pairs, the same 16 384 x Fb cells per target) -- the same
arithmetic per cell without the start bookkeeping.  Both are device time between events from ssym_get_timings
(spot: main_ms; exact: refine_ms), median of --reps calls after --warmup calls, same process, same run.  For the ragged
shape the lane utilisation is printed beside the measured figures, mean over the targets and weighted by their cells:
min(Fb, 64) / 64 (the lanes of a wave a target shorter than 64 frames can keep busy at once) and Fb / (Fb + 63) (a
64-row chunk takes Fb + 63 steps for its 64 x Fb cells: fill and drain of the wavefront included).

    python tools/spot_timing.py [--reps 20] [--warmup 3]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine  # noqa: E402
from soundsym_amd.engine import pack_segments  # noqa: E402

REC_FRAMES, SEG_FRAMES = 16384, 128


def median_ms(call, read, reps, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        call()
        ts.append(read())
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def shape(name, tgt, dim, reps, warmup, seed):
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((REC_FRAMES, dim)).astype(np.float32)
    e = Engine(metric="dtw", dtype="f32")
    whole = e.dictionary(rec.reshape(-1), np.array([0, REC_FRAMES], dtype=np.uint64), dim)
    cutup = e.dictionary(rec.reshape(-1), np.arange(0, REC_FRAMES + 1, SEG_FRAMES, dtype=np.uint64), dim)
    tf, to = pack_segments(tgt, dim, np.float32)
    q = e.queries(tf, to, dim)
    m = len(tgt)
    zeros = np.zeros(m, dtype=np.uint32)
    frames = np.array([t.shape[0] for t in tgt], dtype=np.float64)
    cells = float(frames.sum()) * REC_FRAMES
    spot = median_ms(lambda: e.dtw_spot(whole, q, zeros), lambda: e.timings()["main_ms"], reps, warmup)
    exact = median_ms(lambda: e.match(cutup, q, force_exact=True), lambda: e.timings()["refine_ms"], reps, warmup)
    util = frames / (frames + 63.0)
    wide = np.minimum(frames, 64.0) / 64.0
    print(f"{name:28s} M {m:5d}  cells {cells:.3e}  spot {spot[0]:8.3f} ms [{spot[1]:.3f} ... {spot[2]:.3f}]  "
          f"exact {exact[0]:8.3f} ms [{exact[1]:.3f} ... {exact[2]:.3f}]  spot / exact {spot[0] / exact[0]:5.2f}  "
          f"{cells / spot[0] * 1e-6:7.1f} Gcell/s  lane utilisation by Fb / (Fb + 63): mean {util.mean():.2f}, "
          f"cell-weighted {float((util * frames).sum() / frames.sum()):.2f}; by min(Fb, 64) / 64: mean {wide.mean():.2f}, "
          f"cell-weighted {float((wide * frames).sum() / frames.sum()):.2f}", flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0151)
    shape("4096 x 128 f x 13 d", [rng.standard_normal((128, 13)).astype(np.float32) for _ in range(4096)], 13,
          args.reps, args.warmup, 1)
    shape("4096 x ragged 5..40 f x 13 d", [rng.standard_normal((int(rng.integers(5, 41)), 13)).astype(np.float32)
                                           for _ in range(4096)], 13, args.reps, args.warmup, 2)
    shape("4096 x 256 f x 40 d", [rng.standard_normal((256, 40)).astype(np.float32) for _ in range(4096)], 40,
          args.reps, args.warmup, 3)


if __name__ == "__main__":
    main()
