#!/usr/bin/env python3
"""examples/warp.py -- a reconstruction whose matches follow the target's timing.

    python examples/warp.py -s TARGET.wav -d DICT.wav -o OUT.wav [--plain PLAIN.wav] [--depth 5] [--threshold 4] [--seed 0]

Both recordings are cut by a Partitioner trained on the dictionary recording, as examples/reconstruction.py --partition
cuts them.  Every target segment is matched against the dictionary's segments under DTW, aligned with its match, and the
match is resynthesised along the alignment (SoundSequence.reconstruct_warped_from_dictionary: ssym_match_queries,
ssym_dtw_align and ssym_reconstruct_warped, the alignment staying on the GPU).  --plain writes the length-fitted
reconstruction (reconstruct_from_dictionary: matches cut off or padded with silence) beside it, to compare by ear.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from soundsym_amd import Engine, Partitioner, Sound, SoundDictionary, SoundSequence  # noqa: E402
from soundsym_amd.io import write_wav32  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", required=True, help="target recording")
    ap.add_argument("-d", required=True, help="dictionary recording")
    ap.add_argument("-o", required=True, help="output path of the warped reconstruction")
    ap.add_argument("--plain", help="also write the length-fitted reconstruction here")
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
    sequence = SoundSequence.new([s for s in cut.sounds if s.num_frames() > 0])

    samples, pcm = sequence.reconstruct_warped_from_dictionary(dictionary, want_pcm32=True)
    write_wav32(args.o, sample_rate=target.sample_rate(), pcm=pcm)
    print(f"{len(dictionary.sounds)} dictionary segments, {len(sequence.sounds())} target segments, "
          f"{samples.size} samples -> {args.o}")
    if args.plain:
        plain, plain_pcm = sequence.reconstruct_from_dictionary(dictionary, want_pcm32=True)
        write_wav32(args.plain, sample_rate=target.sample_rate(), pcm=plain_pcm)
        silent = int(np.count_nonzero((plain == 0.0) & (samples != 0.0)))
        print(f"length-fitted -> {args.plain}; {silent} of its samples are padding where the warped match still sounds")
    return samples


if __name__ == "__main__":
    main()
