#!/usr/bin/env python3
"""tools/paced_timing.py -- the paced spot kernel against ssym_dtw_spot on the same pairs (LAB.md 5.18).

The three workloads of tools/spot_timing.py: M targets spotted in ONE recording of 16 384 frames (M pairs, 16 384 x Fb
cells each).  The yardstick is ssym_dtw_spot, the symmetric kernel; beside it ssym_dtw_spot_step(SSYM_STEP_PACED) on the
same pairs, and on the first workload ssym_dtw_spot_all_step(SSYM_STEP_PACED) with K = 8.  All are device time between
events from ssym_get_timings (main_ms), median of --reps calls after --warmup calls, same process, same run.

    python tools/paced_timing.py [--reps 10] [--warmup 3]
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


def median_ms(call, read, reps, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        call()
        ts.append(read())
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def shape(name, tgt, dim, reps, warmup, seed, with_all):
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((REC_FRAMES, dim)).astype(np.float32)
    e = Engine(metric="dtw", dtype="f32")
    whole = e.dictionary(rec.reshape(-1), np.array([0, REC_FRAMES], dtype=np.uint64), dim)
    tf, to = pack_segments(tgt, dim, np.float32)
    q = e.queries(tf, to, dim)
    m = len(tgt)
    zeros = np.zeros(m, dtype=np.uint32)
    cells = float(sum(t.shape[0] for t in tgt)) * REC_FRAMES
    main = lambda: e.timings()["main_ms"]
    spot = median_ms(lambda: e.dtw_spot(whole, q, zeros), main, reps, warmup)
    paced = median_ms(lambda: e.dtw_spot(whole, q, zeros, step="paced"), main, reps, warmup)
    line = (f"{name:28s} M {m:5d}  cells {cells:.3e}  spot {spot[0]:8.3f} ms [{spot[1]:.3f} ... {spot[2]:.3f}]  "
            f"paced {paced[0]:8.3f} ms [{paced[1]:.3f} ... {paced[2]:.3f}]  paced / spot {paced[0] / spot[0]:5.2f}  "
            f"{cells / paced[0] * 1e-6:7.1f} Gcell/s")
    if with_all:
        alls = median_ms(lambda: e.dtw_spot_all(whole, q, zeros, max_spots=8, step="paced"), main, reps, warmup)
        line += (f"  paced spot_all K = 8 {alls[0]:8.3f} ms [{alls[1]:.3f} ... {alls[2]:.3f}]  / paced {alls[0] / paced[0]:5.2f}")
    print(line, flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0151)
    shape("4096 x 128 f x 13 d", [rng.standard_normal((128, 13)).astype(np.float32) for _ in range(4096)], 13,
          args.reps, args.warmup, 1, True)
    shape("4096 x ragged 5..40 f x 13 d", [rng.standard_normal((int(rng.integers(5, 41)), 13)).astype(np.float32)
                                           for _ in range(4096)], 13, args.reps, args.warmup, 2, False)
    shape("4096 x 256 f x 40 d", [rng.standard_normal((256, 40)).astype(np.float32) for _ in range(4096)], 40,
          args.reps, args.warmup, 3, False)


if __name__ == "__main__":
    main()
