#!/usr/bin/env python3
"""examples/stream.py -- the "online" side of examples/reconstruction.rs: feed a recording to a Sound block by block.

    python examples/stream.py -s IN.wav [-b 4096] [--seed 0]

Every block goes through Sound.push_samples (src/sound.rs:145-164): the samples and the MFCC frames stay on the GPU,
only the new samples are uploaded and only the frames they complete are analysed.  At the end the
recording is partitioned straight from the device-resident frames, and the segment lengths are checked against those
of the same file loaded whole.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from soundsym_amd import Partitioner, Sound  # noqa: E402
from soundsym_amd.io import read_wav  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Streams a sound file into a Sound and partitions the resident frames.")
    ap.add_argument("-s", "--sound", required=True, help="path to input sound file")
    ap.add_argument("-b", "--block", type=int, default=4096, help="samples per push")
    ap.add_argument("--seed", type=int, default=0, help="draws the mixture's starting frames")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.block < 1:
        raise SystemExit("--block must be at least 1")
    samples, rate = read_wav(args.sound)
    samples = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
    live = Sound.from_samples(np.zeros(0), float(rate), None)
    for at in range(0, samples.size, args.block):
        live.push_samples(samples[at:at + args.block])
        print(f"pushed {min(at + args.block, samples.size):9d} samples: {live.num_frames():6d} frames")
    whole = Sound.from_path(args.sound)
    assert np.array_equal(live.mfccs(), whole.mfccs()), "streamed frames differ from the whole-file analysis"
    partitioner = Partitioner.new(whole)
    partitioner.train(seed=args.seed)
    want = partitioner.partition()
    stream, lane = live.stream()
    frames = partitioner.engine.partition(partitioner.model, stream.frames_device(lane), partitioner.depth(),
                                          partitioner.threshold())
    got = [int(f) * 256 for f in frames]
    print(f"splits from the resident frames: {got}")
    if got != want:
        print("the resident frames give other segments than the file loaded whole", file=sys.stderr)
        return 1
    print(f"found {len(got)} partitions, equal to the file loaded whole")
    return 0


if __name__ == "__main__":
    sys.exit(main())
