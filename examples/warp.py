#!/usr/bin/env python3
"""examples/warp.py -- a reconstruction whose matches follow the target's timing.

    python examples/warp.py -s TARGET.wav -d DICT.wav -o OUT.wav [--plain PLAIN.wav] [--search 0] [--depth 5] [--threshold 4]
                            [--follow [--max-gain 8]]
                            [--seed 0] [--paced]

Both recordings are cut by a Partitioner trained on the dictionary recording, as examples/reconstruction.py --partition
cuts them.  Every target segment is matched against the dictionary's segments under DTW, aligned with its match, and the
match is resynthesised along the alignment (SoundSequence.reconstruct_warped_from_dictionary: ssym_match_queries,
ssym_dtw_align and ssym_reconstruct_warped, the alignment staying on the GPU).  --plain writes the length-fitted
reconstruction (reconstruct_from_dictionary: matches cut off or padded with silence) beside it, to compare by ear.
--search N (at most 512 samples) resynthesises with the waveform-similarity search instead (ssym_reconstruct_wsola): every
source frame may move up to N samples to where it continues the frame before it in phase; the share of frames that did
move is printed.
--paced matches, aligns and warps under the paced step pattern (match_step="paced", step="paced": ssym_match_queries_step
and ssym_dtw_align_step with SSYM_STEP_PACED): every target frame takes one source frame, the match is the segment with the
least such cost, and no target falls back to the length fit because the symmetric search chose a segment the pattern cannot
align.  Beside the output it prints how many targets the symmetric search would have handed such a pair.
--follow sends the output through the envelope follower (ssym_follow_envelope): hop by hop it takes the loudness of the
target, no gain above --max-gain (default 8); without the flag the output file is what it was.
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
    ap.add_argument("--search", type=int, default=0, help="WSOLA search width in samples (0: plain overlap-add)")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--threshold", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0, help="draws the mixture's starting frames")
    ap.add_argument("--paced", action="store_true", help="match, align and warp under the paced step pattern")
    ap.add_argument("--follow", action="store_true", help="the output takes the target's loudness (envelope following)")
    ap.add_argument("--max-gain", type=float, default=8.0, help="with --follow: the greatest gain")
    args = ap.parse_args(argv)
    follow = dict(dynamics="target", max_gain=args.max_gain) if args.follow else {}

    engine = Engine(metric="dtw", dtype="f64")
    partitioner = Partitioner.from_path(args.d, engine=engine).threshold(args.threshold).depth(args.depth)
    partitioner.train(seed=args.seed)
    dictionary = SoundDictionary.from_segments(partitioner.sound, partitioner.partition(), engine=engine)
    dictionary.sounds = [s for s in dictionary.sounds if s.num_frames() > 0]
    target = Sound.from_path(args.s, engine=engine)
    cut = SoundDictionary.from_segments(target, partitioner.partition_other(target), engine=engine)
    sequence = SoundSequence.new([s for s in cut.sounds if s.num_frames() > 0])

    step = {"step": "paced", "match_step": "paced"} if args.paced else {}
    if args.paced:
        paced_idx, paced_cost = dictionary.match_indices(sequence.sounds(), step="paced", per_frame=True)
        lost = sum(len(a) == 0 for a in dictionary.align(sequence.sounds(), step="paced"))
        print(f"paced: {int(np.isfinite(paced_cost).sum())} of {len(paced_cost)} targets matched, mean cost per frame "
              f"{float(np.mean(paced_cost[np.isfinite(paced_cost)])) if np.isfinite(paced_cost).any() else float('nan'):.4f}; "
              f"the symmetric search would have handed {lost} of them a pair with no paced path")
    if args.search:
        samples, pcm, pos, m_off = dictionary.warp(sequence.sounds(), want_pcm32=True, search=args.search, want_pos=True, **step,
                                                   **follow)
        aligned = dictionary.align(sequence.sounds(), **step)
        moved = frames = 0
        for t, al in enumerate(aligned):
            nominal = np.asarray(al.frame_map, dtype=np.uint64) * np.uint64(256)
            moved += int(np.count_nonzero(pos[int(m_off[t]):int(m_off[t]) + nominal.size] != nominal))
            frames += nominal.size
        print(f"search {args.search}: {moved} of {frames} frames ({100.0 * moved / max(frames, 1):.1f} %) moved off their nominal place")
    else:
        samples, pcm = sequence.reconstruct_warped_from_dictionary(dictionary, want_pcm32=True, **step, **follow)
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
