#!/usr/bin/env python3
"""examples/mosaic.py -- concatenative resynthesis from uncut recordings: neither side is cut beforehand.

    python examples/mosaic.py -s TARGET.wav -d REC.wav|DIR -o OUT.wav [--penalty 1.0] [--gap-cost X] [--gap-fill silence|target]
                              [--search 256] [--follow [--max-gain 8]]

The dictionary is one recording or a folder of recordings, each taken whole, of any length.  SoundDictionary.
reconstruct_mosaic tiles the target with free spans of the recordings -- cuts, recordings, spans and paced paths chosen
together on the GPU for the least total (ssym_dtw_mosaic) -- and resynthesises every piece from its span along its frame map
in one call of the window reconstruction.  --penalty X is charged once per piece and trades total fit for fewer, longer
pieces; at 0 the optimum is frame-wise and stretched spans come back in fragments, so the default is 1.  --gap-cost X lets
frames stay uncovered at X each: they come back as silence, or as the target's own samples with --gap-fill target.
--search N (at most 512 samples) resynthesises with the waveform-similarity search.  One line per piece:
[t0-t1] <- recording r [s0-s1] cost/frame.
--follow sends the output through the envelope follower (ssym_follow_envelope): hop by hop it takes the loudness of the
target, no gain above --max-gain (default 8); without the flag the output file is what it was.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soundsym_amd import Engine, Sound, SoundDictionary  # noqa: E402
from soundsym_amd.io import write_wav32  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", required=True, help="target recording")
    ap.add_argument("-d", required=True, help="dictionary: a recording, or a folder of recordings")
    ap.add_argument("-o", required=True, help="output path of the resynthesis")
    ap.add_argument("--penalty", type=float, default=1.0, help="charged once per piece: fewer, longer pieces")
    ap.add_argument("--gap-cost", type=float, default=None, help="price per frame left uncovered (default: no gaps)")
    ap.add_argument("--gap-fill", choices=("silence", "target"), default="silence", help="what a gap sounds like")
    ap.add_argument("--search", type=int, default=256, help="WSOLA search width in samples (0: plain overlap-add)")
    ap.add_argument("--follow", action="store_true", help="the output takes the target's loudness (envelope following)")
    ap.add_argument("--max-gain", type=float, default=8.0, help="with --follow: the greatest gain")
    args = ap.parse_args(argv)
    follow = dict(dynamics="target", max_gain=args.max_gain) if args.follow else {}

    engine = Engine(metric="dtw", dtype="f64")
    if os.path.isdir(args.d):
        dictionary = SoundDictionary.from_path(args.d, engine=engine)
    else:
        dictionary = SoundDictionary(engine=engine)
        dictionary.sounds = [Sound.from_path(args.d, engine=engine)]
    dictionary.sounds = [s for s in dictionary.sounds if s.num_frames() > 0]
    target = Sound.from_path(args.s, engine=engine)

    mosaic, samples, pcm = dictionary.reconstruct_mosaic(target, args.penalty, args.gap_cost, args.gap_fill, args.search,
                                                         want_pcm32=True, **follow)
    for p in mosaic.pieces:
        if p.is_gap:
            print(f"[{p.start_frame:6d}-{p.end_frame:6d}] <- (gap, {p.num_frames()} frames left uncovered)  "
                  f"{p.cost_per_frame:.4f}/frame")
            continue
        name = dictionary.sounds[p.source_index].name or "#%d" % p.source_index
        print(f"[{p.start_frame:6d}-{p.end_frame:6d}] <- recording {name} [{p.source_first:6d}-{p.source_last:6d}]  "
              f"{p.cost_per_frame:.4f}/frame")
    if mosaic:
        print(f"{len(mosaic.sounding)} pieces and {len(mosaic.gaps)} gaps over {mosaic.num_frames} frames from "
              f"{len(dictionary.sounds)} recordings, {mosaic.total_per_frame:.4f} per frame")
    else:
        print("no mosaic (no frames, or a frame that is not finite and no --gap-cost): silence")
    write_wav32(args.o, sample_rate=target.sample_rate(), pcm=pcm)
    print(f"{samples.size} samples -> {args.o}")
    return mosaic, samples


if __name__ == "__main__":
    main()
