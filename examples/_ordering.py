"""The flow shared by examples/louder.py and examples/pitch_order.py (examples/louder.rs, pitch_confidence.rs):
partition a recording, cut it into sounds, sort them by one descriptor and write them back to back."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soundsym_amd import Partitioner, Sound, analyze_sounds  # noqa: E402
from soundsym_amd.io import read_wav_spec, write_wav_pcm  # noqa: E402


def parser(description: str) -> argparse.ArgumentParser:
    """The reference's options (louder.rs:22-25): -s and -o required, -d depth 4 and -t threshold 3 by default
    (:35-38); --seed draws the mixture's starting frames (the reference draws them at random)."""
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("-s", "--sound", required=True, help="path to input sound file")
    ap.add_argument("-o", "--output", required=True, help="path to output sound file")
    ap.add_argument("-d", "--depth", type=int, default=4, help="depth of analysis trie")
    ap.add_argument("-t", "--threshold", type=int, default=3, help="threshold for segmentation")
    ap.add_argument("--seed", type=int, default=0, help="draws the mixture's starting frames")
    return ap


def cut(samples: np.ndarray, splits, rate: float):
    """`samples.by_ref().take(split)` per split (louder.rs:51-54): the last sounds may come up short, samples past the
    last split are dropped."""
    out, pos = [], 0
    for split in splits:
        out.append(Sound(samples[pos:pos + int(split)], rate, None))
        pos = min(pos + int(split), samples.size)
    return out


def run(args, key: str):
    """key: "max_power" or "pitch_confidence".  Returns (order, descriptor values in input order, splits)."""
    partitioner = Partitioner.from_path(args.sound).threshold(args.threshold).depth(args.depth)
    partitioner.train(seed=args.seed)
    splits = partitioner.partition()
    samples, rate, bits = read_wav_spec(args.sound)
    sounds = cut(samples, splits, rate)
    max_power, pitch_conf = analyze_sounds(sounds, partitioner.engine)     # one device call for every segment
    values = max_power if key == "max_power" else pitch_conf
    order = sorted(range(len(sounds)), key=lambda i: values[i])            # stable and ascending, like sort_by
    for i in order:
        print(f"sound: {i} ({sounds[i].samples().size} samples) {key} {values[i]:.6f}")
    out = np.concatenate([sounds[i].samples() for i in order] or [np.zeros(0)])
    write_wav_pcm(args.output, out, rate, bits)
    return order, values, splits
