#!/usr/bin/env python3
"""examples/occurrences.py -- every place a sound occurs inside recordings that were never cut.

    python examples/occurrences.py -s TARGET.wav -d REC.wav|DIR [-k 8] [--max-cost X] [-o OUT.wav]
                                   [--paced [--max-cost-per-frame X]]

The target stays whole and so do the recordings.  SoundDictionary.spot_all (one ssym_dtw_spot_all call) gives up to -k
pairwise disjoint occurrences per recording, merged by ascending cost; recording, start and end time and cost of every one
are printed.  The cost is a sum along the warping path, not normalised by any length: without --max-cost the list goes on,
after the real occurrences, with spans the target merely fits least badly, and a look at the printed costs shows where
to put the threshold.  With --paced the paced step pattern is used (ssym_dtw_spot_all_step): an occurrence is between
about half and twice the target's length, the mean cost per target frame is printed beside the sum, and
--max-cost-per-frame puts the threshold on that mean, which does not depend on the target's length.  With -o the
occurrences are cut out (SoundDictionary.cut) and written one after the other.
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
    ap.add_argument("-s", required=True, help="the sound to look for")
    ap.add_argument("-d", required=True, help="a recording, or a directory of recordings")
    ap.add_argument("-k", type=int, default=8, help="occurrences per recording at most (1 ... 64)")
    ap.add_argument("--max-cost", type=float, default=None, help="an occurrence costs at most this")
    ap.add_argument("--paced", action="store_true", help="the paced step pattern: slope-bounded spans, costs per frame")
    ap.add_argument("--max-cost-per-frame", type=float, default=None,
                    help="with --paced: an occurrence costs at most this per target frame")
    ap.add_argument("-o", default=None, help="output path: the occurrences cut out and concatenated")
    args = ap.parse_args(argv)
    if args.max_cost_per_frame is not None and not args.paced:
        ap.error("--max-cost-per-frame needs --paced")

    engine = Engine(metric="dtw", dtype="f64")
    if os.path.isdir(args.d):
        dictionary = SoundDictionary.from_path(args.d, engine=engine)
    else:
        dictionary = SoundDictionary(engine)
        dictionary.sounds.append(Sound.from_path(args.d, engine=engine))
    dictionary.sounds = [s for s in dictionary.sounds if s.num_frames() > 0]
    target = Sound.from_path(args.s, engine=engine)

    if args.paced:
        spots = dictionary.spot_all([target], max_spots=args.k, max_cost=args.max_cost, step="paced",
                                    max_cost_per_frame=args.max_cost_per_frame)[0]
    else:
        spots = dictionary.spot_all([target], max_spots=args.k, max_cost=args.max_cost)[0]
    for m, sp in enumerate(spots):
        rec = dictionary.sounds[sp.source_index]
        a, b = sp.sample_span(rec.samples().size)
        print(f"occurrence {m:3d}: {rec.name or sp.source_index} {a / rec.sample_rate():9.3f} s ... "
              f"{b / rec.sample_rate():9.3f} s (frames {sp.start_frame}...{sp.end_frame}), cost {sp.cost:.6g}"
              + (f", per frame {sp.cost_per_frame:.6g}" if sp.cost_per_frame is not None else ""))
    print(f"{len(dictionary.sounds)} recordings, target of {target.num_frames()} frames ({target.num_frames() * HOP} "
          f"samples): {len(spots)} occurrences")
    if args.o:
        pieces = [s.samples() for s in dictionary.cut(spots).sounds]
        samples = np.concatenate(pieces) if pieces else np.zeros(0)
        write_wav32(args.o, samples, sample_rate=target.sample_rate())
        print(f"{samples.size} samples -> {args.o}")
    return spots


if __name__ == "__main__":
    main()
