#!/usr/bin/env python3
"""examples/live_cover.py -- a recording covered by a dictionary while it is still arriving.

    python examples/live_cover.py -s TARGET.wav -d DICT.wav|DIR [-o OUT.wav] [--block 4096] [--penalty 0] [--search 256]
                                  [--depth 5] [--threshold 4] [--seed 0] [--gap-cost X] [--gap-fill silence|target]

The dictionary is built as examples/cover.py builds it.  The target is fed --block samples at a time (Sound.push_samples,
as a recording arrives), and SoundDictionary.cover_live follows it on the GPU: after every block, the pieces that no longer
recording could change are printed -- source, frames, cost per frame -- by the block that commits them, and the flush at the
end prints the rest.  What is printed is, piece for piece, what examples/cover.py prints for the whole recording.  -o writes
the reconstruction from the finished cover: the target cut at the pieces (SoundSequence.from_cover) and every piece warped
from its sound along its paced alignment (SoundDictionary.warp).  Sounds of more than 128 frames are left out of the
dictionary: a cover takes none longer.  --gap-cost X lets frames stay uncovered at X each (ssym_coverer_create_gaps), as in
examples/cover.py: a frame that is not finite then costs one gap frame and the cover goes on; gaps are printed by the block
that commits them, and -o fills them with silence or, with --gap-fill target, with the recording's own samples.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soundsym_amd import Engine, Partitioner, Sound, SoundDictionary, SoundSequence  # noqa: E402
from soundsym_amd.io import write_wav32  # noqa: E402

MAX_FRAMES = 128


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", required=True, help="target recording")
    ap.add_argument("-d", required=True, help="dictionary: a recording, or a folder of sounds")
    ap.add_argument("-o", help="output path of the reconstruction")
    ap.add_argument("--block", type=int, default=4096, help="samples per push")
    ap.add_argument("--penalty", type=float, default=0.0, help="added per piece: fewer, longer pieces")
    ap.add_argument("--search", type=int, default=256, help="WSOLA search width in samples (0: plain overlap-add)")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--threshold", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0, help="draws the mixture's starting frames")
    ap.add_argument("--gap-cost", type=float, default=None, help="price per frame left uncovered (default: no gaps)")
    ap.add_argument("--gap-fill", choices=("silence", "target"), default="silence", help="what a gap sounds like")
    args = ap.parse_args(argv)
    if args.block < 1:
        ap.error("--block must be at least 1")

    engine = Engine(metric="dtw", dtype="f64")
    if os.path.isdir(args.d):
        dictionary = SoundDictionary.from_path(args.d, engine=engine)
    else:
        partitioner = Partitioner.from_path(args.d, engine=engine).threshold(args.threshold).depth(args.depth)
        partitioner.train(seed=args.seed)
        dictionary = SoundDictionary.from_segments(partitioner.sound, partitioner.partition(), engine=engine)
    dictionary.sounds = [s for s in dictionary.sounds if 0 < s.num_frames() <= MAX_FRAMES]
    whole = Sound.from_path(args.s, engine=engine)
    samples = whole.samples()

    def show(pieces, at):
        for _, p in pieces:
            if p.is_gap:
                print(f"[{at:9d} samples] {'(gap)':>16}  frames {p.start_frame:6d} ... {p.end_frame:6d}  "
                      f"{p.cost_per_frame:.4f} per frame")
                continue
            name = dictionary.sounds[p.source_index].name or "#%d" % p.source_index
            print(f"[{at:9d} samples] {name:>16}  frames {p.start_frame:6d} ... {p.end_frame:6d}  "
                  f"{p.cost_per_frame:.4f} per frame")

    first = min(args.block, samples.size)
    target = Sound.from_samples(samples[:first], whole.sample_rate(), engine=engine)
    target.push_samples(samples[:0], engine)                          # resident: the stream the cover follows
    live = dictionary.cover_live([target], args.penalty, args.gap_cost)
    show(live.poll(), first)
    for at in range(first, samples.size, args.block):
        target.push_samples(samples[at:at + args.block], engine)
        show(live.poll(), min(at + args.block, samples.size))
    show(live.flush(), samples.size)
    consumed, covered, committed, total = live.pending()
    cover = live.covers()[0]
    live.close()
    if covered[0] == consumed[0] and cover:
        print(f"{len(cover.sounding)} pieces over {cover.num_frames} frames from {len(dictionary.sounds)} dictionary sounds, "
              f"{cover.total_per_frame:.4f} per frame")
        if args.gap_cost is not None:
            print(f"{len(cover.gaps)} gaps leave {cover.num_frames - cover.covered_frames} frames uncovered")
    else:
        print(f"the cover ends after {int(covered[0])} of {int(consumed[0])} frames (a frame that is not finite, or a stretch no "
              "dictionary sound can pace)")
    out = None
    if args.o and cover and covered[0] == consumed[0]:
        if cover.gaps:
            # the finished sound's cover is the live one: reconstruct_covered warps its pieces and fills its gaps
            _, out, pcm = dictionary.reconstruct_covered(target, args.penalty, args.search, True, args.gap_cost, args.gap_fill)
        else:
            pieces = SoundSequence.from_cover(target, cover).sounds()
            out, pcm = dictionary.warp(pieces, cover.indices(), True, args.search, step="paced")
        write_wav32(args.o, sample_rate=target.sample_rate(), pcm=pcm)
        print(f"{out.size} samples -> {args.o}")
    return cover, out


if __name__ == "__main__":
    main()
