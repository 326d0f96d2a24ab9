"""The sound descriptors' Python surface without a device: Sound.pitch_confidence / preload_pitch_confidence,
analyze_sounds, io.read_wav_spec / write_wav_pcm, the limits, and the example programs' options
(src/sound.rs:170-179, examples/louder.rs, examples/pitch_confidence.rs, examples/partition.rs)."""
import ctypes
import importlib.util
import os
import struct

import numpy as np
import pytest

from soundsym_amd import Sound, analyze_sounds
from soundsym_amd import io as sio
from soundsym_amd.engine import pitch_lags

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
AUDIO = os.path.join(HERE, "golden", "audio")


class _StubEngine:
    """Records the batches it is handed and answers with recognisable values."""

    def __init__(self):
        self.calls = []

    def sound_descriptors(self, samples, offsets, rate, f_min, f_max, voicing, voiced_only):
        self.calls.append((np.array(samples), np.array(offsets), rate, f_min, f_max, voicing, voiced_only))
        n = len(offsets) - 1
        return np.arange(n) + 0.5, np.arange(n) + 0.25


def _sound(n, rate=16000.0, seed=0):
    return Sound(np.random.default_rng(seed).uniform(-0.5, 0.5, n), rate, np.zeros(12))


def test_analyze_sounds_is_one_batch_with_the_reference_literals():
    e = _StubEngine()
    sounds = [_sound(3000, seed=1), _sound(0), _sound(2048, seed=2)]
    mp, pc = analyze_sounds(sounds, e)
    assert len(e.calls) == 1
    samples, offsets, rate, f_min, f_max, voicing, voiced_only = e.calls[0]
    assert list(offsets) == [0, 3000, 3000, 5048]
    assert np.array_equal(samples, np.concatenate([s.samples() for s in sounds]))
    assert (rate, f_min, f_max, voicing, voiced_only) == (44100.0, 100.0, 500.0, 0.2, False)   # src/sound.rs:265
    assert list(mp) == [0.5, 1.5, 2.5] and list(pc) == [0.25, 1.25, 2.25]
    assert analyze_sounds([], e)[0].size == 0 and len(e.calls) == 1


def test_pitch_confidence_is_computed_unless_preloaded():
    e = _StubEngine()
    s = _sound(4096)
    assert s.pitch_confidence(e) == 0.25 and s.pitch_confidence(e) == 0.25
    assert len(e.calls) == 2                                 # not cached (src/sound.rs:170-175)
    s.preload_pitch_confidence(e)
    assert len(e.calls) == 3
    assert s.pitch_confidence(e) == 0.25 and len(e.calls) == 3   # preloaded (:177-179)
    assert s.max_power() == sio.max_power(s.samples())            # unchanged: the host helper


@pytest.mark.parametrize("kw", [dict(f_min=0.0), dict(f_min=600.0), dict(f_max=44100.0), dict(f_min=50.0),
                                dict(rate=0.0), dict(rate=float("inf")), dict(voicing=float("nan"))])
def test_invalid_limits_raise_before_any_device_call(kw):
    e = _StubEngine()
    with pytest.raises(ValueError):
        analyze_sounds([_sound(4096)], e, **kw)
    assert e.calls == []
    args = dict(rate=44100.0, f_min=100.0, f_max=500.0, voicing=0.2)
    args.update(kw)
    with pytest.raises(ValueError):
        pitch_lags(**args)


def test_pitch_lags():
    assert pitch_lags(44100.0, 100.0, 500.0) == (89, 441)
    assert pitch_lags(44100.0, 44100.0 / 682, 44100.0 / 2) == (2, 682)


@pytest.mark.parametrize("name,bits", [("sample.wav", 24), ("Section_7_1.wav", 16)])
def test_wav_spec_round_trip(tmp_path, name, bits):
    x, rate, b = sio.read_wav_spec(os.path.join(AUDIO, name))
    assert b == bits and rate == 44100.0
    y, rate2 = sio.read_wav(os.path.join(AUDIO, name))
    assert np.array_equal(x, y) and rate2 == rate
    out = str(tmp_path / "out.wav")
    sio.write_wav_pcm(out, x, rate, b)
    z, rate3, b3 = sio.read_wav_spec(out)
    assert (rate3, b3) == (rate, b) and np.array_equal(z, x)


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_write_wav_pcm_truncates_and_clips(tmp_path, bits):
    scale = (2 ** 31 - 1) >> (32 - bits)
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, np.nan, 0.999 / scale, -1.999 / scale])
    path = str(tmp_path / "t.wav")
    sio.write_wav_pcm(path, x, 8000, bits)
    data = open(path, "rb").read()
    fmt = struct.unpack("<HHIIHH", data[20:36])
    assert fmt == (1, 1, 8000, 8000 * bits // 8, bits // 8, bits)
    y, _, _ = sio.read_wav_spec(path)
    ints = np.rint(y * scale).astype(np.int64)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    want = [0, int(0.5 * scale), -int(0.5 * scale), scale, -scale, hi, lo, 0, 0, -1]
    assert list(ints) == want


def _example(name):
    spec = importlib.util.spec_from_file_location("ex_" + name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["louder", "pitch_order", "partition"])
def test_example_options(name):
    mod = _example(name)
    a = mod.parse_args(["-s", "in.wav", "-o", "out"])
    assert (a.sound, a.output, a.depth, a.threshold) == ("in.wav", "out", 4, 3)     # louder.rs:35-38
    a = mod.parse_args(["-s", "in.wav", "-o", "o.wav", "-d", "6", "-t", "2"])
    assert (a.depth, a.threshold) == (6, 2)
    with pytest.raises(SystemExit):
        mod.parse_args(["-o", "out"])                        # -s is required (reqopt)
    if name != "partition":
        with pytest.raises(SystemExit):
            mod.parse_args(["-s", "in.wav"])                 # so is -o


def test_cut_takes_splits_in_order_and_drops_the_rest():
    mod = _example("louder")
    import _ordering
    x = np.arange(10.0)
    parts = _ordering.cut(x, [4, 3, 5], 8000.0)
    assert [list(p.samples()) for p in parts] == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]]
    parts = _ordering.cut(x, [2, 3], 8000.0)
    assert sum(p.samples().size for p in parts) == 5
    assert mod is not None


def test_native_window_counts_and_null_context(native_lib):
    out = ctypes.c_uint64()
    for n, w in [(0, 0), (2047, 0), (2048, 1), (3071, 1), (3072, 2), (3073, 2)]:
        assert native_lib.ssym_pitch_num_windows(n, ctypes.byref(out)) == 0 and out.value == w
    assert native_lib.ssym_pitch_num_windows(5, None) == -1
    off = (ctypes.c_uint64 * 2)(0, 0)
    rc = native_lib.ssym_sound_descriptors(None, None, off, 1, 44100.0, 100.0, 500.0, 0.2, 0, None, None)
    assert rc == -1                                          # SSYM_E_INVALID
    rc = native_lib.ssym_pitch_track(None, None, off, 1, 44100.0, 100.0, 500.0, 0.2, 0, None, None, None)
    assert rc == -1
