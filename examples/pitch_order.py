#!/usr/bin/env python3
"""examples/pitch_order.py -- examples/pitch_confidence.rs: arrange the phonemes of a recording in order of increasing
pitch confidence.

    python examples/pitch_order.py -s IN.wav -o OUT.wav [-d 4] [-t 3] [--seed 0]

As examples/louder.py, sorted by pitch_confidence instead (src/sound.rs:258-269 with the reference's literal
arguments: rate 44100, 100-500 Hz, voicing threshold 0.2; this package's own pitch definition, DESIGN.md 5.9, parity
unpinned).  The reference also writes every segment to ./test_sound/out_sound.wav while it preloads the confidences
(pitch_confidence.rs:57-68), each write replacing the last; that debugging output is left out here.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ordering  # noqa: E402


def parse_args(argv=None):
    return _ordering.parser("Arranges the phonemes in a sound file in order of increasing pitch confidence.") \
        .parse_args(argv)


def main(argv=None):
    _ordering.run(parse_args(argv), "pitch_confidence")
    return 0


if __name__ == "__main__":
    sys.exit(main())
