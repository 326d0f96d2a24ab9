#!/usr/bin/env python3
"""Batched MFCC and sequence-distance timings (LAB.md):

  - SoundSequence.from_timestamps on Section_7_1.wav + vowel.txt (55 sounds): the batched path (one ssym_mfcc_batch)
    against the per-sound loop it replaced (one ssym_mfcc per label, i.e. Sound.from_samples(.., None) each);
  - SoundSequence.distances() on a clone_from_dictionary sequence built from sample.wav's partitioner segments (its
    length-fitted sounds re-analysed in one batch, then one ssym_sequence_distances), next to the same per-sound loop
    of ssym_mfcc calls.

    python tools/sequence_timing.py [--reps 9]

Every call ends in its own host synchronisation, so a host clock around it is the call's time (uploads, host table
build and copies back included); each line is the median of --reps calls after one warm-up call.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine, Partitioner, Sound, SoundDictionary, SoundSequence  # noqa: E402
from soundsym_amd.io import audacity_labels_to_timestamps, read_wav  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
AUDIO = os.path.join(GOLD, "audio")


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
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    e = Engine(metric="refcos", dtype="f64")

    y, rate = read_wav(os.path.join(AUDIO, "Section_7_1.wav"))
    section = Sound(y, rate, None)
    ts = audacity_labels_to_timestamps(os.path.join(GOLD, "vowel.txt"))

    def per_sound():
        out = []
        for start, end, label in ts:
            a, b = int(np.floor(start * rate + 0.5)), int(np.floor(end * rate + 0.5))
            out.append(Sound.from_samples(y[a:b + 1].copy(), rate, None, label, engine=e))
        return out
    ms_b, seq = timed(lambda: SoundSequence.from_timestamps(section, ts, engine=e), args.reps)
    ms_l, loop = timed(per_sound, args.reps)
    assert all(np.array_equal(a.mfccs(), b.mfccs()) for a, b in zip(seq.sounds(), loop))
    frames = sum(s.num_frames() for s in seq.sounds())
    print(f"from_timestamps  {len(ts):4d} sounds {frames:6d} frames  batched {ms_b:8.3f} ms  per-sound loop "
          f"{ms_l:8.3f} ms  ({ms_l / ms_b:.1f}x)", flush=True)
    ms_d, _ = timed(lambda: seq.distances(engine=e), args.reps)
    print(f"distances        {len(ts):4d} sounds (all carry features)  {ms_d:8.3f} ms", flush=True)

    p = Partitioner.from_path(os.path.join(AUDIO, "sample.wav"), engine=e)
    p.train(seed=0)
    d = SoundDictionary.from_segments(p.sound, p.partition(), engine=e)
    cloned = seq.clone_from_dictionary(d)
    fitted = [s for s in cloned.sounds() if not s.has_mfccs()]

    def per_sound_fitted():
        return [e.mfcc(s.samples(), s.sample_rate(), 12) for s in fitted]
    ms_c, dist = timed(lambda: cloned.distances(engine=e), args.reps)
    ms_f, _ = timed(per_sound_fitted, args.reps)
    print(f"clone distances  {len(cloned.sounds()):4d} sounds ({len(fitted)} fitted, {len(d.sounds)} in the dictionary)"
          f"  distances() {ms_c:8.3f} ms  per-sound ssym_mfcc of the fitted alone {ms_f:8.3f} ms  "
          f"(finite {int(np.isfinite(dist).sum())} of {dist.size})", flush=True)
    e.close()


if __name__ == "__main__":
    main()
