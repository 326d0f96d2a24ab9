#!/usr/bin/env python3
"""Partitioner timings (LAB.md): train (5 EM iterations), discretize (up to 1000), predict + vote, and
the numpy restatement of tests/partition_ref.py on one core, for 2^14, 2^17 and 2^20 frames x 12 values.

    python tools/partition_timing.py [--reps 5] [--sizes 14,17,20] [--no-numpy]

Every GPU call ends in its one host synchronisation, so a host clock around the call is the call's time; each line is
the median of --reps calls after one warm-up call of the same shape.  Data: 26 separated Gaussian clusters (seeded).
"""
import argparse
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"          # the restatement on one core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from soundsym_amd import Engine  # noqa: E402
from soundsym_amd.api import init_rows  # noqa: E402


def mixture(n, K=26, d=12, seed=1):
    rng = np.random.default_rng(seed)
    centers = rng.normal(scale=6.0, size=(K, d))
    lab = rng.integers(0, K, n)
    return centers[lab] + rng.normal(size=(n, d)) * rng.uniform(0.5, 1.5, size=(K, 1))[lab]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="14,17,20")
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    e = Engine(metric="refcos", dtype="f64")
    for p in [int(v) for v in args.sizes.split(",")]:
        n = 1 << p
        x = mixture(n)
        rows = init_rows(n, 26, seed=0)

        def train(iters):
            g = e.gmm_train(x, 12, rows, 0.1, iters)
            g.close()
            return g.iters

        ms, it = timed(lambda: train(5), args.reps)
        print(f"n=2^{p} train (5 iterations)            {ms:9.3f} ms  iterations {it}", flush=True)

        def discretize():
            g = e.gmm_train(x, 12, rows, 0.1, 1000)
            e.gmm_predict(g, x, want_post=True)
            it = g.iters
            g.close()
            return it
        ms, it = timed(discretize, args.reps)
        print(f"n=2^{p} discretize (up to 1000)         {ms:9.3f} ms  iterations {it}", flush=True)
        g = e.gmm_train(x, 12, rows, 0.1, 5)
        ms, seg = timed(lambda: e.partition(g, x, 5, 4), args.reps)
        print(f"n=2^{p} predict + vote (d 5, t 4)       {ms:9.3f} ms  segments {seg.size}", flush=True)
        if not args.no_numpy:
            import partition_ref as ref
            t0 = time.perf_counter()
            z = ref.standardize(x)
            m = ref.gmm_train(z, rows, 0.1, 5)
            t1 = time.perf_counter()
            segs = ref.partition(x, m["weights"], m["means"], m["covs"], 5, 4)
            t2 = time.perf_counter()
            print(f"n=2^{p} numpy one core: train {1e3 * (t1 - t0):9.1f} ms, predict + vote {1e3 * (t2 - t1):9.1f} ms"
                  f"  segments {len(segs)}", flush=True)
        g.close()
    e.close()


if __name__ == "__main__":
    main()
