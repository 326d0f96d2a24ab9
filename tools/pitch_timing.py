#!/usr/bin/env python3
"""Sound-descriptor timings (LAB.md): ssym_sound_descriptors (max_power + pitch_confidence) on the two
committed recordings whole, on the partitioner's segments of sample.wav as one ragged batch, and on a 10-minute
synthetic tone, each next to the numpy restatement of tests/pitch_ref.py on one core.

    python tools/pitch_timing.py [--reps 5] [--no-numpy]

Every call ends in its one host synchronisation, so a host clock around the call is the call's time (the upload of the
samples included); each line is the median of --reps calls after one warm-up call.  The restatement of the long tone
runs on its first minute and is scaled by 10 (its windows are independent).
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

from soundsym_amd import Engine, Partitioner  # noqa: E402
from soundsym_amd.io import read_wav  # noqa: E402

AUDIO = os.path.join(ROOT, "tests", "golden", "audio")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def batch(parts):
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate(parts), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    e = Engine(metric="refcos", dtype="f64")
    cases = []
    for name in ("sample.wav", "Section_7_1.wav"):
        x, _ = read_wav(os.path.join(AUDIO, name))
        cases.append((name + " whole", *batch([x]), 1.0))
    x, _ = read_wav(os.path.join(AUDIO, "sample.wav"))
    p = Partitioner.from_path(os.path.join(AUDIO, "sample.wav"), engine=e).threshold(3).depth(4)
    p.train(seed=0)
    parts, pos = [], 0
    for sp in p.partition():
        parts.append(x[pos:pos + sp])
        pos = min(pos + sp, x.size)
    cases.append((f"sample.wav segments ({len(parts)})", *batch(parts), 1.0))
    n = 600 * 44100
    t = np.arange(n) / 44100.0
    tone = 0.5 * np.sin(2 * np.pi * 220.0 * t) * (1.0 + 0.3 * np.sin(2 * np.pi * 0.5 * t))
    cases.append(("10-minute tone", *batch([tone]), 10.0))
    for label, x, off, scale in cases:
        freq, _, _, woff = e.pitch_track(x, off)
        ms, (mp, pc) = timed(lambda: e.sound_descriptors(x, off), args.reps)
        line = f"{label:32s} {x.size:9d} samples {int(woff[-1]):6d} windows  gpu {ms:9.3f} ms"
        if not args.no_numpy:
            import pitch_ref as ref
            xs, offs = x, off
            if scale != 1.0:
                xs, offs = batch([x[:n // 10]])
            t0 = time.perf_counter()
            want = ref.descriptors(xs, offs)
            ms_np = 1e3 * (time.perf_counter() - t0) * scale
            if scale == 1.0:
                assert np.array_equal(mp, want[0]) and np.allclose(pc, want[1], rtol=1e-11, atol=0)
            line += f"  numpy one core {ms_np:10.1f} ms" + ("  (first minute x 10)" if scale != 1.0 else "")
        print(line, flush=True)
    e.close()


if __name__ == "__main__":
    main()
