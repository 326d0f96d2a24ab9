#!/usr/bin/env python3
"""Time per push of a streaming sound (LAB.md 5.11) against what the library offered before streams:

  stream   Stream.push of one block per lane (no host output: the frames stay resident), one synchronisation;
  before   the tail re-analysis a caller had to do after every block: Engine.mfcc on samples[num_frames * 256:] for one
           sound, Engine.mfcc_batch on the 64 tails for 64 sounds, plus the host max_power (io.max_power) of each tail.

    python tools/stream_timing.py [--reps 200] [--rounds 5] [--only-stream]

Rows: blocks of 256, 1024, 4096 and 44100 samples pushed onto sounds of 1 s and 30 s (44.1 kHz), 1 lane and 64 lanes.
Both sides end in their own host synchronisation, so a host clock around a call is the call's time.  Every row is
warmed up, then timed `reps` times in each of `rounds` rounds; the table gives the median of all calls and the spread
of the round medians (max - min), which is the run-to-run noise a difference has to exceed.  The stream is reset and
re-seeded with the start sound before every round, outside the timed region (a push's work does not depend on the
length already held); growth is outside the timed region too: the capacity of a whole round is reserved.
--only-stream runs just the stream side (one short pass per row): the input of a kernel trace.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine  # noqa: E402
from soundsym_amd.io import max_power  # noqa: E402

RATE = 44100.0
HOP = 256


def medians(fn, reps, rounds, between=None):
    for _ in range(5):
        fn()
    meds, every = [], []
    for _ in range(rounds):
        if between:
            between()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        meds.append(float(np.median(ts)))
        every += ts
    return 1e6 * float(np.median(every)), 1e6 * (max(meds) - min(meds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-stream", action="store_true")
    args = ap.parse_args()
    e = Engine(metric="refcos", dtype="f64")
    rng = np.random.default_rng(0)
    print(f"{'lanes':>5} {'sound':>6} {'block':>6} {'stream us':>10} {'spread':>7} {'before us':>10} {'spread':>7} {'ratio':>6}",
          flush=True)
    for lanes in (1, 64):
        for seconds in (1, 30):
            n0 = int(seconds * RATE)
            base = 0.3 * rng.normal(size=n0)
            for block in (256, 1024, 4096, 44100):
                reps = args.reps if block < 44100 else max(args.reps // 4, 10)
                if args.only_stream:
                    reps = min(reps, 20)
                chunk = 0.3 * rng.normal(size=lanes * block)
                off = np.arange(lanes + 1, dtype=np.uint64) * block
                st = e.stream(lanes, RATE, capacity=n0 + (reps + 8) * block)

                def reseed():
                    for l in range(lanes):
                        st.reset(l)
                        st.seed(l, base)
                reseed()
                s_us, s_sp = medians(lambda: st.push(chunk, off), reps, 1 if args.only_stream else args.rounds, reseed)
                st.close()
                if args.only_stream:
                    print(f"{lanes:5d} {seconds:5d}s {block:6d} {s_us:10.1f}", flush=True)
                    continue
                # the tail a caller re-analyses after this block: from the first frame the old sound did not hold
                f0 = Engine.mfcc_num_frames(n0)
                tail = np.concatenate([base[f0 * HOP:], chunk[:block]])
                if lanes == 1:
                    def before():
                        e.mfcc(tail, RATE)
                        max_power(tail)
                else:
                    tails = np.concatenate([tail] * lanes)
                    toff = np.arange(lanes + 1, dtype=np.uint64) * tail.size

                    def before():
                        e.mfcc_batch(tails, toff, RATE)
                        for l in range(lanes):
                            max_power(tails[l * tail.size:(l + 1) * tail.size])
                b_us, b_sp = medians(before, reps, args.rounds)
                print(f"{lanes:5d} {seconds:5d}s {block:6d} {s_us:10.1f} {s_sp:7.1f} {b_us:10.1f} {b_sp:7.1f} "
                      f"{b_us / s_us:6.2f}", flush=True)
    e.close()


if __name__ == "__main__":
    main()
