#!/usr/bin/env python3
"""examples/live_mosaic.py -- a recording tiled by free spans of uncut recordings while it is still arriving.

    python examples/live_mosaic.py -s TARGET.wav -d REC.wav|DIR [-o OUT.wav] [--block 4096] [--penalty 1.0] [--gap-cost X]
                                   [--gap-fill silence|target] [--search 256] [--live-audio] [--follow [--max-gain 8]]

The dictionary is built as examples/mosaic.py builds it: one recording or a folder of recordings, each taken whole.  The
target is fed --block samples at a time (Sound.push_samples, as a recording arrives), and SoundDictionary.mosaic_live follows
it on the GPU.  The mosaicker commits target frames a frame or two behind the input; a piece is printed -- target frames,
recording, its span, cost per frame -- by the block that closes it (the next start has been committed), and the flush at the
end prints the rest.  What is printed is, piece for piece, what examples/mosaic.py prints for the whole recording.  -o writes
the resynthesis of the finished mosaic (SoundDictionary.reconstruct_mosaic(mosaic=...)): nothing is computed twice.
--gap-cost X lets frames stay uncovered at X each: a frame that is not finite then costs one gap frame and the mosaic goes on.
--live-audio resynthesises while the target arrives (mosaic_live(audio=True), LiveMosaic.audio()): every block also prints
the samples it released and the hops still held back (at most 4 without a search, at most 12 with one), and -o writes what
was gathered push by push -- the same WAV as without the flag, sample for sample.
--follow gives the resynthesis the target's loudness, hop by hop (dynamics="target", at most --max-gain): without --live-audio
through reconstruct_mosaic, with it through the LiveMosaic's Follower, which holds two or three hops more -- again the same
WAV either way.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from soundsym_amd import HOP, Engine, Sound, SoundDictionary  # noqa: E402
from soundsym_amd.io import write_wav32  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", required=True, help="target recording")
    ap.add_argument("-d", required=True, help="dictionary: a recording, or a folder of recordings")
    ap.add_argument("-o", help="output path of the resynthesis")
    ap.add_argument("--block", type=int, default=4096, help="samples per push")
    ap.add_argument("--penalty", type=float, default=1.0, help="charged once per piece: fewer, longer pieces")
    ap.add_argument("--gap-cost", type=float, default=None, help="price per frame left uncovered (default: no gaps)")
    ap.add_argument("--gap-fill", choices=("silence", "target"), default="silence", help="what a gap sounds like")
    ap.add_argument("--search", type=int, default=256, help="WSOLA search width in samples (0: plain overlap-add)")
    ap.add_argument("--live-audio", action="store_true", help="resynthesise while the target arrives (LiveMosaic.audio)")
    ap.add_argument("--follow", action="store_true",
                    help="the resynthesis takes the target's loudness, hop by hop (dynamics=\"target\"; live with --live-audio)")
    ap.add_argument("--max-gain", type=float, default=8.0, help="the greatest gain of --follow, finite and at least 1")
    args = ap.parse_args(argv)
    if args.block < 1:
        ap.error("--block must be at least 1")

    engine = Engine(metric="dtw", dtype="f64")
    if os.path.isdir(args.d):
        dictionary = SoundDictionary.from_path(args.d, engine=engine)
    else:
        dictionary = SoundDictionary(engine=engine)
        dictionary.sounds = [Sound.from_path(args.d, engine=engine)]
    dictionary.sounds = [s for s in dictionary.sounds if s.num_frames() > 0]
    whole = Sound.from_path(args.s, engine=engine)
    samples = whole.samples()

    def show(pieces, at):
        for _, p in pieces:
            if p.is_gap:
                print(f"[{at:9d} samples] [{p.start_frame:6d}-{p.end_frame:6d}] <- (gap, {p.num_frames()} frames left uncovered)  "
                      f"{p.cost_per_frame:.4f}/frame")
                continue
            name = dictionary.sounds[p.source_index].name or "#%d" % p.source_index
            print(f"[{at:9d} samples] [{p.start_frame:6d}-{p.end_frame:6d}] <- recording {name} "
                  f"[{p.source_first:6d}-{p.source_last:6d}]  {p.cost_per_frame:.4f}/frame")

    first = min(args.block, samples.size)
    target = Sound.from_samples(samples[:first], whole.sample_rate(), engine=engine)
    target.push_samples(samples[:0], engine)                          # resident: the stream the mosaic follows
    if args.live_audio:
        live = dictionary.mosaic_live([target], args.penalty, args.gap_cost, audio=True, search=args.search, gap_fill=args.gap_fill,
                                      dynamics="target" if args.follow else None, max_gain=args.max_gain)
    else:
        live = dictionary.mosaic_live([target], args.penalty, args.gap_cost)
    heard = []                                                        # --live-audio: (samples, pcm) as they are released

    def listen(at):
        if not args.live_audio:
            return
        heard.append(live.audio(want_pcm32=True)[0])
        released = sum(h[0].size for h in heard)
        frames = int(live.pending()[2][0])
        print(f"[{at:9d} samples] {heard[-1][0].size:7d} samples released, {max(frames - released // HOP, 0):2d} hops held"
              + (" (two or three of them by the follower)" if args.follow else ""))

    show(live.poll(), first)
    listen(first)
    for at in range(first, samples.size, args.block):
        target.push_samples(samples[at:at + args.block], engine)
        show(live.poll(), min(at + args.block, samples.size))
        listen(min(at + args.block, samples.size))
    show(live.flush(), samples.size)
    listen(samples.size)
    consumed, covered, committed, total = live.pending()
    mosaic = live.mosaics()[0]
    live.close()
    if covered[0] == consumed[0] and mosaic:
        print(f"{len(mosaic.sounding)} pieces and {len(mosaic.gaps)} gaps over {mosaic.num_frames} frames from "
              f"{len(dictionary.sounds)} recordings, {mosaic.total_per_frame:.4f} per frame")
    else:
        print(f"the mosaic ends after {int(covered[0])} of {int(consumed[0])} frames (a frame that is not finite and no --gap-cost)")
    out = None
    if args.live_audio and mosaic and covered[0] == consumed[0]:
        out, pcm = (np.concatenate([h[k] for h in heard]) for k in (0, 1))      # what was heard, push by push
        if args.o:
            write_wav32(args.o, sample_rate=target.sample_rate(), pcm=pcm)
            print(f"{out.size} samples -> {args.o}")
    elif args.o and mosaic and covered[0] == consumed[0]:
        _, out, pcm = dictionary.reconstruct_mosaic(target, args.penalty, args.gap_cost, args.gap_fill, args.search,
                                                    want_pcm32=True, mosaic=mosaic, dynamics="target" if args.follow else None,
                                                    max_gain=args.max_gain)
        write_wav32(args.o, sample_rate=target.sample_rate(), pcm=pcm)
        print(f"{out.size} samples -> {args.o}")
    return mosaic, out


if __name__ == "__main__":
    main()
