#!/usr/bin/env python3
"""examples/align.py -- which frame of the match goes with which frame of the target.

    python examples/align.py -s TARGET.wav -d DICT.wav [--depth 5] [--threshold 4] [--seed 0]

Both recordings are cut by a Partitioner trained on the dictionary recording; every target segment is matched against
the dictionary's segments under DTW and aligned with its match (SoundDictionary.align: one ssym_match_queries and one
ssym_dtw_align).  Per target segment: the matched segment, the DTW cost, the number of cells L of the warping path
and the share of its steps that are diagonal (1.0: the match fits the target's timing as it is).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soundsym_amd import Engine, Partitioner, Sound, SoundDictionary  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", required=True, help="target recording")
    ap.add_argument("-d", required=True, help="dictionary recording")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--threshold", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0, help="draws the mixture's starting frames")
    args = ap.parse_args(argv)

    engine = Engine(metric="dtw", dtype="f64")
    partitioner = Partitioner.from_path(args.d, engine=engine).threshold(args.threshold).depth(args.depth)
    partitioner.train(seed=args.seed)
    dictionary = SoundDictionary.from_segments(partitioner.sound, partitioner.partition(), engine=engine)
    dictionary.sounds = [s for s in dictionary.sounds if s.num_frames() > 0]
    target = Sound.from_path(args.s, engine=engine)
    cut = SoundDictionary.from_segments(target, partitioner.partition_other(target), engine=engine)
    targets = [s for s in cut.sounds if s.num_frames() > 0]

    alignments = dictionary.align(targets)
    print(f"{len(dictionary.sounds)} dictionary segments, {len(targets)} target segments")
    for t, (sound, a) in enumerate(zip(targets, alignments)):
        match = dictionary.sounds[a.source_index]
        print(f"{t:5d}: {sound.num_frames():4d} frames -> segment {a.source_index:5d} ({match.num_frames():4d} frames)  "
              f"cost {a.cost:10.4f}  L {len(a):4d}  diagonal {a.diagonal_share():.2f}")
    return alignments


if __name__ == "__main__":
    main()
