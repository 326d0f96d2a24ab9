"""Streaming sounds, the part that needs no GPU: the push plan against a brute-force restatement,
Sound.mfcc_arrays, the errors raised before any device work, and the ssym_stream_* names in every binding."""
import os
import re

import numpy as np
import pytest

import soundsym_amd._native as nat
from soundsym_amd import Sound, push_sounds, stream_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_SYMBOLS = {"ssym_stream_create", "ssym_stream_destroy", "ssym_stream_push", "ssym_stream_seed",
                  "ssym_stream_counts", "ssym_stream_read", "ssym_stream_frames_device", "ssym_stream_samples_device",
                  "ssym_stream_descriptors", "ssym_stream_reset"}


def _starts(n, size, hop):
    """the starts of the full windows of a sound of n samples, listed one by one"""
    return [s for s in range(0, max(n - size + 1, 0), hop)]


def test_stream_plan_against_listed_windows():
    frames = {n: _starts(n, 1024, 256) for n in range(0, 2600 + 1400 + 1)}
    power = {n: _starts(n, 128, 64) for n in range(0, 2600 + 1400 + 1)}
    for n_old in range(0, 2601):
        fo, po = frames[n_old], power[n_old]
        for n_add in range(0, 1401):
            f0, fn, w0, wn = stream_plan(n_old, n_add)
            fw, pw = frames[n_old + n_add], power[n_old + n_add]
            # the old windows, then the new ones, are the whole sound's: none missing, none doubled
            assert f0 == len(fo) and f0 + fn == len(fw) and w0 == len(po) and w0 + wn == len(pw)
            if fn:      # the first new frame starts on both grids, and its window is inside the new sound
                assert fw[f0] == 256 * f0 and fw[f0] % 64 == 0 and fw[-1] + 1024 <= n_old + n_add
            if wn:
                assert pw[w0] == 64 * w0 and pw[-1] + 128 <= n_old + n_add
    # (starts are multiples of the hop from 0, so equal counts mean equal lists; spot-check that claim itself)
    assert frames[2600] == [0, 256, 512, 768, 1024, 1280, 1536] and power[300] == [0, 64, 128]


def test_stream_plan_reference_cases_and_errors():
    assert stream_plan(2048, 3072)[:2] == (5, 12) and stream_plan(0, 5120)[:2] == (0, 17)    # 17 frames, not the stale 5
    assert stream_plan(0, 0) == (0, 0, 0, 0) and stream_plan(1023, 1) == (0, 1, 14, 1)
    with pytest.raises(ValueError):
        stream_plan(-1, 4)
    with pytest.raises(ValueError):
        stream_plan(4, -1)


def test_mfcc_arrays():
    m = np.arange(36, dtype=np.float64)
    s = Sound(np.zeros(2000), 44100.0, m)
    a = s.mfcc_arrays()
    assert a.shape == (3, 12) and np.array_equal(a, m.reshape(3, 12)) and np.array_equal(a[1], m[12:24])
    assert Sound(np.zeros(10), 8000.0, np.zeros(0), ncoeffs=5).mfcc_arrays().shape == (0, 5)
    assert Sound(np.zeros(10), 8000.0, np.arange(10.0), ncoeffs=5).mfcc_arrays().shape == (2, 5)
    with pytest.raises(ValueError):
        Sound(np.zeros(10), 8000.0, None).mfcc_arrays()


def test_push_errors_before_any_device_work():
    with pytest.raises(ValueError, match="carries no features"):
        Sound(np.zeros(4096), 44100.0, None).push_samples(np.zeros(256))
    # more frames than the samples allow (2047 samples hold 4 full windows)
    with pytest.raises(ValueError, match="more frames"):
        Sound(np.zeros(2047), 44100.0, np.zeros(5 * 12)).push_samples(np.zeros(256))
    a, b = Sound(np.zeros(2048), 44100.0, np.zeros(12)), Sound(np.zeros(2048), 22050.0, np.zeros(12))
    with pytest.raises(ValueError, match="share"):
        push_sounds([a, b], [np.zeros(4), np.zeros(4)])
    c = Sound(np.zeros(2048), 44100.0, np.zeros(13), ncoeffs=13)
    with pytest.raises(ValueError, match="share"):
        push_sounds([a, c], [np.zeros(4), np.zeros(4)])
    with pytest.raises(ValueError):
        push_sounds([a], [np.zeros(4), np.zeros(4)])
    with pytest.raises(ValueError):
        push_sounds([a, a], [np.zeros(4), np.zeros(4)])
    push_sounds([], [])


def test_stream_symbols_are_bound_everywhere():
    header = open(os.path.join(ROOT, "include", "soundsym_amd.h")).read()
    declared = set(re.findall(r"SSYM_API\s+[\w\s\*]+?\b(ssym_stream_\w+)\s*\(", header))
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    assert STREAM_SYMBOLS <= declared
    assert STREAM_SYMBOLS <= set(nat.ABI_SYMBOLS)
    assert STREAM_SYMBOLS <= set(re.findall(r"pub fn (ssym_stream_\w+)", rust))
    assert "stream.hip" in open(os.path.join(ROOT, "soundsym_amd", "csrc", "Makefile")).read()


def test_library_exports_the_stream_symbols(native_lib):
    for name in STREAM_SYMBOLS:
        assert hasattr(native_lib, name), name
    assert native_lib.ssym_abi_version() == 3
