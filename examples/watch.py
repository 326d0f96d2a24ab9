#!/usr/bin/env python3
"""examples/watch.py -- watch for known sounds in a recording that arrives block by block.

    python examples/watch.py -s RECORDING.wav -d TARGETS.wav|DIR [--block 4096] [--max-cost X]
                             [--paced [--max-cost-per-frame X]]

The recording is fed --block samples at a time, as a microphone would deliver it (Sound.push_samples: only the new
samples are uploaded and analysed).  A Watch (streaming DTW spotting: ssym_spotter_*) consumes the new frames of every
block on the GPU -- the work of a block does not grow with what came before -- and reports an occurrence of a target as
soon as the frames that follow it no longer overlap it: the block, the target, the span in seconds and the cost are printed
as each event is emitted.  The rule is causal: a span once reported is never revised, unlike examples/occurrences.py, which
sees the whole recording.  The cost is a sum along the warping path, not normalised by any length; without --max-cost
every stretch of the recording is reported as the occurrence it resembles most, and the printed costs show where to put the
threshold.  With --paced the paced step pattern is used (ssym_spotter_create_step): a reported span has between about half
and twice the target's frames, the cost per target frame is printed beside the sum, and --max-cost-per-frame puts the
threshold on that mean -- one value for targets of every length.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soundsym_amd import BIN, Engine, Sound, SoundDictionary, watch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", required=True, help="the recording that is fed block by block")
    ap.add_argument("-d", required=True, help="a target sound, or a directory of them")
    ap.add_argument("--block", type=int, default=4096, help="samples per block")
    ap.add_argument("--max-cost", type=float, default=None, help="an occurrence costs at most this")
    ap.add_argument("--paced", action="store_true", help="the paced step pattern: slope-bounded spans, costs per frame")
    ap.add_argument("--max-cost-per-frame", type=float, default=None,
                    help="with --paced: an occurrence costs at most this per target frame")
    args = ap.parse_args(argv)
    if args.max_cost_per_frame is not None and not args.paced:
        ap.error("--max-cost-per-frame needs --paced")

    engine = Engine(metric="dtw", dtype="f64")
    whole = Sound.from_path(args.s, engine=engine)
    if os.path.isdir(args.d):
        targets = [t for t in SoundDictionary.from_path(args.d, engine=engine).sounds if t.num_frames() > 0]
    else:
        targets = [Sound.from_path(args.d, engine=engine)]
    samples, rate = whole.samples(), whole.sample_rate()

    head = min(BIN, samples.size)                       # the first window, analysed as a sound of its own
    live = Sound.from_samples(samples[:head], rate, engine=engine)
    live.push_samples(samples[head:head], engine)       # makes the sound resident: the stream a Watch follows
    if args.paced:
        w = watch([live], targets, max_cost=args.max_cost, engine=engine, step="paced",
                  max_cost_per_frame=args.max_cost_per_frame)
    else:
        w = watch([live], targets, max_cost=args.max_cost, engine=engine)
    found = []

    def report(block, events):
        for _, t, sp in events:
            a, b = sp.sample_span(live.samples().size)
            print(f"block {block:5d}: {targets[t].name or t} {a / rate:9.3f} s ... {b / rate:9.3f} s "
                  f"(frames {sp.start_frame}...{sp.end_frame}), cost {sp.cost:.6g}"
                  + (f", per frame {sp.cost_per_frame:.6g}" if sp.cost_per_frame is not None else ""))
        found.extend(events)

    block = 0
    report(block, w.poll())
    for at in range(head, samples.size, args.block):
        block += 1
        live.push_samples(samples[at:at + args.block], engine)
        report(block, w.poll())
    report(block, w.flush())
    print(f"{block} blocks of {args.block} samples, {live.num_frames()} frames, {len(targets)} targets: {len(found)} events")
    w.close()
    return found


if __name__ == "__main__":
    main()
