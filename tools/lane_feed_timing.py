#!/usr/bin/env python3
"""tools/lane_feed_timing.py -- the host paths around the lane feed and the output stager (csrc/lane_feed.hpp,
dtw_wave.hpp's StagedOut), timed with a host clock around each call; every call ends in its own synchronisation (LAB.md).

    follow   a spotter following a one-lane stream that is fed blocks of 4096 samples (16 frames of 12 coefficients at
             44.1 kHz: examples/watch.py's loop), 8 targets of 20 ... 80 frames: ms per follow, the median over the blocks
             after --warmup.
    cover    ssym_dtw_cover with host outputs, f64 engine (examples/cover.py): 512 segments of 5 ... 40 frames x 12 values,
             one target of 2048 frames: ms per call, the median of --reps calls.
    mosaic   ssym_dtw_mosaic with host outputs, f64 engine (examples/mosaic.py): 8 recordings of 512 frames x 12 values, one
             target of 1024 frames: ms per call, the median of --reps calls.

One MI355X, one process.  SSYM_LIB names another build of the library to time (soundsym_amd/_native.py).

    python tools/lane_feed_timing.py [--blocks 256] [--reps 10] [--warmup 3]
"""
import argparse
import json
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
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def row(name, ms, **more):
    ms = np.array(ms)
    print(json.dumps(dict(what=name, calls=int(ms.size), ms_median=float(np.median(ms)), ms_min=float(ms.min()),
                          ms_max=float(ms.max()), **more)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED1A9E)
    mk = lambda f: rng.standard_normal((int(f), 12))
    e = Engine(metric="dtw", dtype="f64")

    q = e.queries(*pack_segments([mk(f) for f in rng.integers(20, 81, size=8)], 12, np.float64), 12)
    st, sp = e.stream(1, 44100.0, 12), e.spotter(q, 1)
    wave = rng.standard_normal(1024 + 4096 * args.blocks) * 0.3
    st.push(wave[:1024])
    ms, events = [], 0
    for b in range(args.blocks):
        st.push(wave[1024 + 4096 * b:1024 + 4096 * (b + 1)])
        t, n = timed(lambda: sp.follow(st))
        ms.append(t)
        events += n
    row("follow", ms[args.warmup:], frames=int(sp.counts()[0]), events=events)
    for h in (sp, st, q):
        h.close()

    d = e.dictionary(*pack_segments([mk(f) for f in rng.integers(5, 41, size=512)], 12, np.float64), 12)
    q = e.queries(*pack_segments([mk(2048)], 12, np.float64), 12)
    ms = [timed(lambda: e.dtw_cover(d, q, 0.0)) for _ in range(args.warmup + args.reps)][args.warmup:]
    row("cover", [t for t, _ in ms], pieces=int(ms[-1][1][0][0]))
    for h in (q, d):
        h.close()

    d = e.dictionary(*pack_segments([mk(512) for _ in range(8)], 12, np.float64), 12)
    q = e.queries(*pack_segments([mk(1024)], 12, np.float64), 12)
    ms = [timed(lambda: e.dtw_mosaic(d, q, 1.0)) for _ in range(args.warmup + args.reps)][args.warmup:]
    row("mosaic", [t for t, _ in ms], pieces=int(ms[-1][1][0][0]))
    for h in (q, d):
        h.close()
    e.close()


if __name__ == "__main__":
    main()
