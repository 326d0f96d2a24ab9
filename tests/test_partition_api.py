"""The partitioner's Python surface without a device (src/lib.rs:67-178)."""
import os
import struct

import numpy as np
import pytest

from soundsym_amd import Partitioner, Sound
from soundsym_amd import io as sio


def _sound(frames=40, rate=8000.0):
    rng = np.random.default_rng(5)
    return Sound(rng.uniform(-0.5, 0.5, frames * 256), rate, rng.normal(size=frames * 12), "s")


def test_builders_keep_their_values():
    p = Partitioner(_sound())
    assert p.depth() == 5 and p.threshold() == 4               # src/lib.rs:78-79
    q = p.depth(3).threshold(2)
    assert q is p and p.depth() == 3 and p.threshold() == 2
    other = _sound(10)
    p.sound = other                                             # examples/reconstruction.rs:72 reassigns it
    assert p.sound is other


def test_partition_before_train_raises():
    p = Partitioner(_sound())
    with pytest.raises(RuntimeError, match="Must first train model"):
        p.partition()
    with pytest.raises(RuntimeError, match="Must first train model"):
        p.partition_other(_sound(12))


def _read_pcm32(path):
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    fmt = struct.unpack("<HHIIHH", data[20:36])
    assert fmt[0] == 1 and fmt[1] == 1 and fmt[5] == 32
    size = struct.unpack("<I", data[40:44])[0]
    return fmt[2], np.frombuffer(data[44:44 + size], dtype="<i4")


def test_write_splits_names_and_pcm(tmp_path):
    s = _sound(8)
    splits = [512, 256, 768, 1024]                              # the last one runs past the end of the sound
    paths = sio.write_splits(s, splits, str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == ["00000_512.wav", "00001_256.wav", "00002_768.wav", "00003_1024.wav"]
    assert [os.path.basename(p) for p in paths] == names
    pos = 0
    for name, split in zip(names, splits):
        rate, pcm = _read_pcm32(os.path.join(tmp_path, name))
        want = sio.pcm32(s.samples()[pos:pos + split])
        assert rate == 8000 and np.array_equal(pcm, want)
        pos = min(pos + split, s.samples().size)
    assert _read_pcm32(os.path.join(tmp_path, names[-1]))[1].size == 8 * 256 - 1536
