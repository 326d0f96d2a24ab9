#!/usr/bin/env python3
"""examples/partition.py -- examples/partition.rs: partition a recording and optionally write every segment.

    python examples/partition.py -s IN.wav [-o OUT_DIR] [-d 4] [-t 3] [--seed 0]

A Partitioner trained on the recording cuts it into segments (GMM letters + voting experts on the GPU);
the segment lengths are printed and, with -o, written by io.write_splits as {idx:05}_{split}.wav (src/lib.rs:155-178).
The reference reads a fixed data/inventing.wav (partition.rs:53); here the input is -s.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soundsym_amd import Partitioner  # noqa: E402
from soundsym_amd.io import write_splits  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Partitions a sound file into phoneme-like segments.")
    ap.add_argument("-s", "--sound", required=True, help="path to input sound file")
    ap.add_argument("-o", "--output", help="output directory for the segments")
    ap.add_argument("-d", "--depth", type=int, default=4, help="depth of analysis trie")
    ap.add_argument("-t", "--threshold", type=int, default=3, help="threshold for segmentation")
    ap.add_argument("--seed", type=int, default=0, help="draws the mixture's starting frames")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    t0 = time.perf_counter()
    partitioner = Partitioner.from_path(args.sound).threshold(args.threshold).depth(args.depth)
    partitioner.train(seed=args.seed)
    splits = partitioner.partition()
    print(f"time to partition: {time.perf_counter() - t0:.3f} s")
    print(f"splits: {splits}")
    print(f"found {len(splits)} partitions")
    if args.output:
        os.makedirs(args.output, exist_ok=True)
        write_splits(partitioner.sound, splits, args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
