#!/usr/bin/env python3
"""examples/spot.py -- a reconstruction from recordings that were never cut.

    python examples/spot.py -s TARGET.wav -d DICT.wav|DIR -o OUT.wav [--paced] [--search 0] [--depth 5] [--threshold 4] [--seed 0]
                            [--follow [--max-gain 8]]

The target is cut by a Partitioner as examples/warp.py cuts it (trained on the first dictionary recording); the dictionary
recordings stay whole.  Every target segment is located inside the recordings by subsequence DTW
(SoundDictionary.spot: one ssym_spot_queries call), and each span is warped onto its target's timing where it lies, from
the dictionary and the samples that are resident already (SoundDictionary.warp with spans=: ssym_dtw_align_spans and
ssym_reconstruct_warped_spans, or ssym_reconstruct_wsola_spans with --search N) -- nothing is cut and nothing is uploaded a
second time.  The recording, span and cost of every target segment are printed; the cost is a sum along the path, not
normalised by any length.

--paced: the whole flow under the paced step pattern (step="paced": ssym_spot_queries_step, SSYM_STEP_PACED) -- every
target frame takes one source frame, at most one source frame in a row is skipped or repeated.  The span of a segment then
has about half to twice its frames, the alignment of the span has the cost the spot reported, and cost / frames is a
mean per-frame distance: it is printed per segment, and its mean over the segments at the end.
--follow sends the output through the envelope follower (ssym_follow_envelope): hop by hop it takes the loudness of the
target, no gain above --max-gain (default 8); without the flag the output file is what it was.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from soundsym_amd import Engine, Partitioner, Sound, SoundDictionary  # noqa: E402
from soundsym_amd.io import write_wav32  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", required=True, help="target recording")
    ap.add_argument("-d", required=True, help="dictionary recording, or a directory of recordings")
    ap.add_argument("-o", required=True, help="output path of the reconstruction")
    ap.add_argument("--paced", action="store_true", help="spot, align and warp under the paced step pattern")
    ap.add_argument("--search", type=int, default=0, help="WSOLA search width in samples (0: plain overlap-add)")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--threshold", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0, help="draws the mixture's starting frames")
    ap.add_argument("--follow", action="store_true", help="the output takes the target's loudness (envelope following)")
    ap.add_argument("--max-gain", type=float, default=8.0, help="with --follow: the greatest gain")
    args = ap.parse_args(argv)
    follow = dict(dynamics="target", max_gain=args.max_gain) if args.follow else {}

    engine = Engine(metric="dtw", dtype="f64")
    if os.path.isdir(args.d):
        dictionary = SoundDictionary.from_path(args.d, engine=engine)
    else:
        dictionary = SoundDictionary(engine)
        dictionary.sounds.append(Sound.from_path(args.d, engine=engine))
    dictionary.sounds = [s for s in dictionary.sounds if s.num_frames() > 0]
    partitioner = Partitioner(dictionary.sounds[0], engine=engine).threshold(args.threshold).depth(args.depth)
    partitioner.train(seed=args.seed)
    target = Sound.from_path(args.s, engine=engine)
    pieces = SoundDictionary.from_segments(target, partitioner.partition_other(target), engine=engine)
    targets = [s for s in pieces.sounds if s.num_frames() > 0]

    step = {"step": "paced"} if args.paced else {}
    spots = dictionary.spot(targets, **step)
    for t, sp in enumerate(spots):
        if not sp:
            print(f"segment {t:4d} ({targets[t].num_frames():3d} frames): no spot")
            continue
        name = dictionary.sounds[sp.source_index].name or str(sp.source_index)
        per_frame = f", per frame {sp.cost_per_frame:.6g}" if args.paced else ""
        print(f"segment {t:4d} ({targets[t].num_frames():3d} frames): {name} frames {sp.start_frame}...{sp.end_frame} "
              f"({sp.num_frames()} frames), cost {sp.cost:.6g}{per_frame}")
    samples, pcm = dictionary.warp(targets, spans=spots, want_pcm32=True, search=args.search, **step, **follow)
    if args.paced:
        means = [sp.cost_per_frame for sp in spots if sp]
        print(f"mean cost_per_frame over {len(means)} spotted segments: {np.mean(means) if means else float('nan'):.6g}")
    write_wav32(args.o, sample_rate=target.sample_rate(), pcm=pcm)
    print(f"{len(dictionary.sounds)} recordings, {len(targets)} target segments, {samples.size} samples -> {args.o}")
    return samples


if __name__ == "__main__":
    main()
