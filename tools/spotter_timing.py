#!/usr/bin/env python3
"""tools/spotter_timing.py -- what a spotter's push costs against spotting the recording again (LAB.md
5.17).

Catch-up: ONE lane fed a recording of 16 384 frames in one push, against the target sets tools/spot_all_timing.py uses, and
ssym_dtw_spot over the same pairs in the same process.  The spotter's time is total_ms of ssym_get_timings (forward
kernel + reporting, device time between events); ssym_dtw_spot's is main_ms.  The gate: the push at 128 f x 13 d within
1.10 x ssym_dtw_spot; the other shapes are reported.  Live: the same targets, pushes of 4, 16, 64 and 172 frames onto the
lane that holds the 16 384: device ms and wall ms per push, true cells per second (new rows x target frames, per device
time), and beside them what a user does today: ssym_dtw_spot on the whole recording.  Median of --reps calls after
--warmup calls.  Exit status 1 when the gate is missed.

--paced: every workload runs twice in the same process, under the symmetric and under the paced step
pattern (Engine.spotter(step="paced") against ssym_dtw_spot_step with SSYM_STEP_PACED on the same pairs), and a line per
workload gives paced push / paced spot, paced push / symmetric push and paced spot / symmetric spot.  The gate stays on the
symmetric run.

    python tools/spotter_timing.py [--reps 10] [--warmup 2] [--paced]
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

REC_FRAMES = 16384
GATE = 1.10
LIVE = (4, 16, 64, 172)


def median(values):
    v = np.array(values)
    return float(np.median(v)), float(v.min()), float(v.max())


def shape(name, tgt, dim, reps, warmup, seed, step="symmetric"):
    """One workload under one step pattern: prints its lines, returns (push / spot, push ms, spot ms)."""
    kw = {} if step == "symmetric" else {"step": step}
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((REC_FRAMES + max(LIVE) * (reps + warmup) * len(LIVE), dim)).astype(np.float32).astype(np.float64)
    e = Engine(metric="dtw", dtype="f32")
    whole = e.dictionary(rec[:REC_FRAMES].astype(np.float32).reshape(-1), np.array([0, REC_FRAMES], dtype=np.uint64), dim)
    tf, to = pack_segments(tgt, dim, np.float32)
    q = e.queries(tf, to, dim)
    m = len(tgt)
    cells_per_row = float(sum(t.shape[0] for t in tgt))
    zeros = np.zeros(m, dtype=np.uint32)
    sp = e.spotter(q, 1, **kw)
    spot, push, wall = [], [], []
    for r in range(warmup + reps):
        e.dtw_spot(whole, q, zeros, **kw)
        spot.append(e.timings()["main_ms"])
        sp.reset(0)
        t0 = time.perf_counter()
        sp.push(rec[:REC_FRAMES])
        wall.append((time.perf_counter() - t0) * 1e3)
        tm = e.timings()
        push.append((tm["total_ms"], tm["main_ms"], tm["reduce_ms"]))
    spot, wall = median(spot[warmup:]), median(wall[warmup:])
    tot, fwd, rep = (median([p[k] for p in push[warmup:]]) for k in range(3))
    fmt = lambda t: f"{t[0]:8.3f} ms [{t[1]:.3f} ... {t[2]:.3f}]"
    ratio = tot[0] / spot[0]
    print(f"{name + ('' if step == 'symmetric' else ' [' + step + ']'):28s} M {m:5d}  catch-up: spot {fmt(spot)}  push {fmt(tot)} (forward {fwd[0]:.3f}, reporting {rep[0]:.3f}, "
          f"wall {wall[0]:.3f})  push / spot {ratio:5.3f}  events {sp.n_events}", flush=True)
    at = REC_FRAMES
    for rows in LIVE:
        dev, wl = [], []
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            sp.push(rec[at:at + rows])
            wl.append((time.perf_counter() - t0) * 1e3)
            dev.append(e.timings()["total_ms"])
            at += rows
        dev, wl = median(dev[warmup:]), median(wl[warmup:])
        print(f"    live push of {rows:4d} rows: device {fmt(dev)}  wall {wl[0]:7.3f} ms  {rows * cells_per_row / dev[0] / 1e6:8.2f} "
              f"Gcells/s  expected by rows {spot[0] * rows / REC_FRAMES:7.3f} ms  re-spotting the whole {spot[0]:8.3f} ms", flush=True)
    sp.close()
    e.close()
    return ratio, tot[0], spot[0]


def workload(paced, name, tgt, dim, reps, warmup, seed):
    """The symmetric run, and with --paced the paced one beside it with the three ratios; returns the symmetric push / spot."""
    sym = shape(name, tgt, dim, reps, warmup, seed)
    if paced:
        pac = shape(name, tgt, dim, reps, warmup, seed, "paced")
        print(f"    paced push / paced spot {pac[0]:5.3f} (symmetric {sym[0]:5.3f})  paced push / symmetric push "
              f"{pac[1] / sym[1]:5.3f}  paced spot / symmetric spot {pac[2] / sym[2]:5.3f}", flush=True)
    return sym[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paced", action="store_true", help="every workload under the paced step pattern too (DESIGN.md 5.20)")
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0151)
    # (each target set is drawn once, in this order, whatever the options: the default run is the run of 5.17)
    sets = [[rng.standard_normal((128, 13)).astype(np.float32) for _ in range(4096)],
            [rng.standard_normal((int(rng.integers(5, 41)), 13)).astype(np.float32) for _ in range(4096)],
            [rng.standard_normal((256, 40)).astype(np.float32) for _ in range(4096)]]
    gated = workload(args.paced, "4096 x 128 f x 13 d", sets[0], 13, args.reps, args.warmup, 1)
    workload(args.paced, "4096 x ragged 5..40 f x 13 d", sets[1], 13, args.reps, args.warmup, 2)
    workload(args.paced, "4096 x 256 f x 40 d", sets[2], 40, args.reps, args.warmup, 3)
    print(f"gate: push / spot at 128 f x 13 d = {gated:.3f} (at most {GATE:.2f}): {'ok' if gated <= GATE else 'MISSED'}")
    return 0 if gated <= GATE else 1


if __name__ == "__main__":
    sys.exit(main())
