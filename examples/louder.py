#!/usr/bin/env python3
"""examples/louder.py -- examples/louder.rs: arrange the phonemes of a recording in order of increasing loudness.

    python examples/louder.py -s IN.wav -o OUT.wav [-d 4] [-t 3] [--seed 0]

A Partitioner trained on the recording cuts it into segments (GMM letters + voting experts on the GPU),
every segment's max_power (the largest RMS over 128-sample windows hopped by 64, src/sound.rs:244-256) comes from one
ssym_sound_descriptors call over all segments, and the segments are written back to back in ascending order (a stable
sort, like sort_by) with the input's sample rate and bit depth.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ordering  # noqa: E402


def parse_args(argv=None):
    return _ordering.parser("Arranges the phonemes in a sound file in order of increasing loudness.").parse_args(argv)


def main(argv=None):
    _ordering.run(parse_args(argv), "max_power")
    return 0


if __name__ == "__main__":
    sys.exit(main())
