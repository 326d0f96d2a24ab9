#!/usr/bin/env python3
"""examples/cover.py -- a reconstruction whose target is cut by the dictionary itself.

    python examples/cover.py -s TARGET.wav -d DICT.wav|DIR -o OUT.wav [--penalty 0] [--search 256] [--depth 5] [--threshold 4]
                             [--follow [--max-gain 8]]
                             [--seed 0] [--gap-cost X] [--gap-fill silence|target]

The dictionary is a folder of sounds (SoundDictionary.from_path) or one recording cut by a Partitioner trained on it, as
examples/reconstruction.py --partition cuts it.  The target is NOT cut beforehand: SoundDictionary.reconstruct_covered tiles
it with dictionary sounds, cut points and sounds chosen together on the GPU so that the paced alignment costs of the pieces
sum to the least total (ssym_dtw_cover), then warps every piece from its sound along its paced alignment (the existing
align and warp calls).  --penalty X adds X per piece and trades total fit for fewer, longer pieces.  --search N (at most 512
samples) resynthesises with the waveform-similarity search.  One line per piece: source, frames, cost per frame.  Sounds of
more than 128 frames are left out of the dictionary: a cover takes none longer.  --gap-cost X lets frames stay uncovered at X
each (ssym_dtw_cover_gaps): a stretch that no sound fits better than X per frame -- breath, a door, a frame that is not
finite -- is left out and comes back as silence, or as the target's own samples with --gap-fill target; one line per gap.
--follow sends the output through the envelope follower (ssym_follow_envelope): hop by hop it takes the loudness of the
target, no gain above --max-gain (default 8); without the flag the output file is what it was.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soundsym_amd import Engine, Partitioner, Sound, SoundDictionary  # noqa: E402
from soundsym_amd.io import write_wav32  # noqa: E402

MAX_FRAMES = 128


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", required=True, help="target recording")
    ap.add_argument("-d", required=True, help="dictionary: a recording, or a folder of sounds")
    ap.add_argument("-o", required=True, help="output path of the reconstruction")
    ap.add_argument("--penalty", type=float, default=0.0, help="added per piece: fewer, longer pieces")
    ap.add_argument("--search", type=int, default=256, help="WSOLA search width in samples (0: plain overlap-add)")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--threshold", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0, help="draws the mixture's starting frames")
    ap.add_argument("--gap-cost", type=float, default=None, help="price per frame left uncovered (default: no gaps)")
    ap.add_argument("--gap-fill", choices=("silence", "target"), default="silence", help="what a gap sounds like")
    ap.add_argument("--follow", action="store_true", help="the output takes the target's loudness (envelope following)")
    ap.add_argument("--max-gain", type=float, default=8.0, help="with --follow: the greatest gain")
    args = ap.parse_args(argv)
    follow = dict(dynamics="target", max_gain=args.max_gain) if args.follow else {}

    engine = Engine(metric="dtw", dtype="f64")
    if os.path.isdir(args.d):
        dictionary = SoundDictionary.from_path(args.d, engine=engine)
    else:
        partitioner = Partitioner.from_path(args.d, engine=engine).threshold(args.threshold).depth(args.depth)
        partitioner.train(seed=args.seed)
        dictionary = SoundDictionary.from_segments(partitioner.sound, partitioner.partition(), engine=engine)
    dictionary.sounds = [s for s in dictionary.sounds if 0 < s.num_frames() <= MAX_FRAMES]
    target = Sound.from_path(args.s, engine=engine)

    cover, samples, pcm = dictionary.reconstruct_covered(target, args.penalty, search=args.search, want_pcm32=True,
                                                         gap_cost=args.gap_cost, gap_fill=args.gap_fill, **follow)
    for p in cover.pieces:
        if p.is_gap:
            print(f"{'(gap)':>16}  frames {p.start_frame:6d} ... {p.end_frame:6d}  ({p.num_frames():3d} left uncovered)      "
                  f"{p.cost_per_frame:.4f} per frame")
            continue
        name = dictionary.sounds[p.source_index].name or "#%d" % p.source_index
        print(f"{name:>16}  frames {p.start_frame:6d} ... {p.end_frame:6d}  ({p.num_frames():3d} of the sound's "
              f"{dictionary.sounds[p.source_index].num_frames():3d})  {p.cost_per_frame:.4f} per frame")
    if cover:
        print(f"{len(cover.sounding)} pieces over {cover.num_frames} frames from {len(dictionary.sounds)} dictionary sounds, "
              f"{cover.total_per_frame:.4f} per frame")
        if args.gap_cost is not None:
            print(f"{len(cover.gaps)} gaps leave {cover.num_frames - cover.covered_frames} frames uncovered")
    else:
        print("no cover (a frame that is not finite, or a stretch no dictionary sound can pace): the length-fitted match instead")
    write_wav32(args.o, sample_rate=target.sample_rate(), pcm=pcm)
    print(f"{samples.size} samples -> {args.o}")
    return cover, samples


if __name__ == "__main__":
    main()
