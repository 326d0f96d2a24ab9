"""Hand-checked properties of the numpy restatement of DESIGN.md 5.9 (tests/pitch_ref.py), the yardstick that
tests/test_gpu_pitch.py holds the device to."""
import numpy as np
import pytest

import pitch_ref as ref
from soundsym_amd import io as sio

RATE = 44100.0


def _sine(f, n=8192, amp=0.5):
    return amp * np.sin(2.0 * np.pi * f * np.arange(n) / RATE)


@pytest.mark.parametrize("f", [100.5, 150.0, 220.0, 333.0, 490.0])
def test_sines_are_recovered(f):
    t = ref.track(_sine(f))
    assert len(t["freq"]) == 7
    assert np.all(np.abs(t["freq"] - f) < 1e-3)
    assert np.all((t["strength"] >= 0.99) & (t["strength"] <= 1.03))
    assert np.all(t["tau"] == np.round(RATE / f))          # the voiced candidate wins: u is 0.2 in a full-scale tone
    assert np.all(t["unvoiced"] == pytest.approx(0.2))


def test_harmonic_tone_is_not_an_octave_off():
    n = np.arange(8192)
    x = sum(np.sin(2.0 * np.pi * 150.0 * k * n / RATE) / k for k in range(1, 8))
    t = ref.track(x)
    assert np.all(np.abs(t["freq"] - 150.0) < 1e-2)


def test_white_noise_is_weakly_voiced():
    x = np.random.default_rng(0).normal(size=16384)
    t = ref.track(x)
    assert np.all(t["strength"] < 0.3)


@pytest.mark.parametrize("n,w", [(0, 0), (2047, 0), (2048, 1), (3071, 1), (3072, 2), (3073, 2), (4096, 3)])
def test_window_counts(n, w):
    assert ref.num_windows(n) == w


def test_short_sound_has_confidence_zero():
    mp, pc, pv, tracks = ref.descriptors(_sine(220.0, 2047), [0, 2047])
    assert pc[0] == 0.0 and pv[0] == 0.0 and len(tracks[0]["freq"]) == 0
    assert mp[0] > 0.0


def test_unvoiced_candidate():
    x = _sine(220.0, 2048 * 5)
    x[4096:6144] = 0.0                                      # window 4 is silent, the sound is not
    t = ref.track(x)
    assert t["unvoiced"][4] == 2.2 and not np.any(t["freq"][4:5])
    assert t["score"][4] == 2.2 and t["tau"][4] == -1
    z = ref.track(np.zeros(4096))                           # G = 0: u = v (Rust's max of 0 and NaN)
    assert np.all(z["unvoiced"] == 0.2) and np.all(z["freq"] == 0.0)
    mp, pc, pv, _ = ref.descriptors(np.zeros(4096), [0, 4096], voicing=0.35)
    assert pc[0] == 0.35 and pv[0] == 0.0 and mp[0] == 0.0


def test_nan_window_is_skipped_by_the_fold():
    x = _sine(220.0, 2048 * 3)
    x[100] = np.nan                                         # only in window 0
    t = ref.track(x)
    assert np.isnan(t["freq"][0]) and np.isnan(t["strength"][0]) and np.isnan(t["unvoiced"][0])
    assert np.all(np.isfinite(t["score"][1:]))
    _, pc, _, _ = ref.descriptors(x, [0, x.size])
    assert pc[0] == np.max(t["score"][1:])


def test_max_power_matches_the_host_helper():
    rng = np.random.default_rng(3)
    for n in (127, 128, 129, 191, 192, 5000, 44100):
        x = rng.normal(size=n) * rng.uniform(0.01, 2.0)
        want = sio.max_power(x)
        got = ref.max_power(x)
        assert abs(got - want) <= 1e-15 * max(want, 1e-300) or got == want == 0.0


def test_limits():
    assert ref.lag_range(44100.0, 100.0, 500.0) == (89, 441)
    for args in [(44100.0, 0.0, 500.0), (44100.0, 500.0, 100.0), (44100.0, 100.0, 44100.0), (44100.0, 60.0, 500.0),
                 (0.0, 100.0, 500.0), (float("nan"), 100.0, 500.0)]:
        with pytest.raises(ValueError):
            ref.lag_range(*args)
