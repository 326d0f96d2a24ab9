#!/usr/bin/env python3
"""tools/spot_all_timing.py -- what keeping the end column and picking K occurrences adds to a spotting call (DESIGN.md
5.16, LAB.md 5.16).

On the shapes tools/spot_timing.py records (M targets against ONE recording of 16 384 frames) the same pairs go through
ssym_dtw_spot and then through ssym_dtw_spot_all with K = 1 and K = 8, without a threshold: every pair makes all its K
picks, the most the selection can cost.  All three are device time between events from ssym_get_timings (main_ms), median
of --reps calls after --warmup calls, same process, same run.  The gate: K = 8 at 128 f x 13 d within 1.10 x ssym_dtw_spot;
the other ratios are reported.  Exit status 1 when the gate is missed.

    python tools/spot_all_timing.py [--reps 10] [--warmup 2]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine  # noqa: E402
from soundsym_amd.engine import pack_segments  # noqa: E402

REC_FRAMES = 16384
GATE = 1.10


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
    tf, to = pack_segments(tgt, dim, np.float32)
    q = e.queries(tf, to, dim)
    m = len(tgt)
    zeros = np.zeros(m, dtype=np.uint32)
    read = lambda: e.timings()["main_ms"]
    spot = median_ms(lambda: e.dtw_spot(whole, q, zeros), read, reps, warmup)
    k1 = median_ms(lambda: e.dtw_spot_all(whole, q, zeros, max_spots=1), read, reps, warmup)
    k8 = median_ms(lambda: e.dtw_spot_all(whole, q, zeros, max_spots=8), read, reps, warmup)
    count = e.dtw_spot_all(whole, q, zeros, max_spots=8)[0]
    fmt = lambda t: f"{t[0]:8.3f} ms [{t[1]:.3f} ... {t[2]:.3f}]"
    print(f"{name:28s} M {m:5d}  spot {fmt(spot)}  spot_all K=1 {fmt(k1)}  K=8 {fmt(k8)}  "
          f"K=1 / spot {k1[0] / spot[0]:5.3f}  K=8 / spot {k8[0] / spot[0]:5.3f}  "
          f"occurrences per pair (K=8): {count.mean():.2f}", flush=True)
    e.close()
    return k8[0] / spot[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0151)
    gated = shape("4096 x 128 f x 13 d", [rng.standard_normal((128, 13)).astype(np.float32) for _ in range(4096)], 13,
                  args.reps, args.warmup, 1)
    shape("4096 x ragged 5..40 f x 13 d", [rng.standard_normal((int(rng.integers(5, 41)), 13)).astype(np.float32)
                                           for _ in range(4096)], 13, args.reps, args.warmup, 2)
    shape("4096 x 256 f x 40 d", [rng.standard_normal((256, 40)).astype(np.float32) for _ in range(4096)], 40,
          args.reps, args.warmup, 3)
    print(f"gate: K=8 / spot at 128 f x 13 d = {gated:.3f} (at most {GATE:.2f}): {'ok' if gated <= GATE else 'MISSED'}")
    return 0 if gated <= GATE else 1


if __name__ == "__main__":
    sys.exit(main())
