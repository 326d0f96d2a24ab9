"""tests/warp_ref.py, the restatement the GPU is held to, against what follows from the definition of warped
reconstruction itself: no device needed."""
import math

import numpy as np

import warp_ref as ref
from soundsym_amd.api import BIN, HOP, length_fit

ULP = 2.0 ** -52


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _random_maps(rng, frames, s_frames):
    kind = int(rng.integers(0, 3))
    if kind == 0:                                             # monotone, as ssym_dtw_align gives them
        return np.sort(rng.integers(0, max(s_frames, 1), size=frames)).astype(np.uint32)
    if kind == 1:                                             # any order
        return rng.integers(0, max(s_frames, 1) + 3, size=frames).astype(np.uint32)
    m = rng.integers(0, max(s_frames, 1), size=frames).astype(np.uint32)
    m[rng.integers(0, frames, size=max(1, frames // 4))] = rng.choice(
        np.array([0xFFFFFFFF, 0x80000000, 0x01000000, s_frames + 5], dtype=np.uint32), size=max(1, frames // 4))
    return m


def test_the_window_is_the_mfcc_table():
    assert len(ref.WINDOW) == BIN == 1024 and HOP == 256 and ref.HOP == HOP and ref.BIN == BIN
    assert ref.WINDOW[0] == 0.0 and ref.WINDOW[512] == 1.0
    for m in (1, 255, 256, 700, 1023):
        assert ref.WINDOW[m] == 0.5 - 0.5 * math.cos(2.0 * math.pi * m / 1024.0)
    src = open(__file__.replace("tests/test_warp_ref.py", "soundsym_amd/csrc/mfcc_frame.hpp")).read()
    assert "0.5 - 0.5 * std::cos(2.0 * PI * (double)i / (double)kBin)" in src


def test_vectorised_and_scalar_restatements_agree_bit_for_bit():
    rng = np.random.default_rng(0x3A9)
    for case in range(40):
        frames = int(rng.integers(1, 12))
        n = int(rng.integers(0, frames * HOP + BIN + 300))
        s_len = int(rng.integers(0, 3000)) if case % 7 else 0
        x = rng.standard_normal(s_len)
        fmap = _random_maps(rng, frames, s_len // HOP)
        a, b = ref.warp_one(x, n, fmap), ref.warp_one_scalar(x, n, fmap)
        assert np.array_equal(_bits(a), _bits(b)), case
        assert np.array_equal(_bits(ref.warp_one(x, n, fmap, valid=False)), _bits(length_fit(x, n)))


def test_identity_map_returns_the_sound():
    rng = np.random.default_rng(0x1D)
    for frames in (1, 4, 5, 23):
        n = frames * HOP
        x = rng.standard_normal(n)
        out = ref.warp_one(x, n, np.arange(frames, dtype=np.uint32))
        # every tap of sample k reads x[k]: num = sum fl(w x), den = sum w -- one rounding per product, three per sum of
        # four, one for the division.  Sample 0 has one tap, of weight w[0] = 0: den = 0, the sample is +0.0
        err = np.abs(out[1:] - x[1:])
        print("identity map, %d frames: max |out - x| / |x| = %.3g ulp" % (frames, (err / np.abs(x[1:])).max() / ULP))
        assert (err <= 4.0 * ULP * np.abs(x[1:])).all()
        assert _bits(out[:1])[0] == 0


def test_a_constant_signal_stays_constant_under_any_map():
    rng = np.random.default_rng(0xC0)
    worst = 0.0
    for c in (1.0, -0.25, 0.1, -0.7312, 1e-3, 3.0e5, math.pi):
        for _ in range(6):
            frames = int(rng.integers(1, 30))
            s_len = int(rng.integers(1, 6000))
            n = int(rng.integers(1, frames * HOP + BIN + 200))
            fmap = _random_maps(rng, frames, s_len // HOP)
            out = ref.warp_one(np.full(s_len, c), n, fmap)
            # where a tap is valid: samples whose denominator is positive
            probe = ref.warp_one(np.ones(s_len), n, fmap)
            has = probe != 0.0
            assert np.array_equal(has, out != 0.0)
            if has.any():
                worst = max(worst, (np.abs(out[has] - c) / (ULP * abs(c))).max())
            assert (np.abs(out[has] - c) <= 2.0 * ULP * abs(c)).all(), c
    print("constant signals: worst error %.3g ulp" % worst)


def test_samples_without_a_valid_tap_are_plus_zero():
    x = -np.ones(700)                                                     # a negative signal: -0.0 would show
    # two frames mapped far beyond the source, one onto its start: only the frame-2 stretch has valid taps
    fmap = np.array([0xFFFFFFFF, 9, 0], dtype=np.uint32)
    out = ref.warp_one(x, 3000, fmap)
    k = np.arange(3000)
    valid = (k >= 2 * HOP) & (k < 2 * HOP + BIN) & (k - 2 * HOP < 700) & (k != 2 * HOP)      # w[0] = 0 at k = 512
    assert (out[valid] == -1.0).all()
    assert (_bits(out[~valid]) == 0).all()                                # +0.0, not -0.0
    assert (_bits(ref.warp_one(np.zeros(0), 2000, np.arange(5))) == 0).all()      # an empty source
    assert ref.warp_one(x, 0, fmap).size == 0


def test_no_map_is_the_length_fit():
    rng = np.random.default_rng(0xF0)
    for s_len, n in ((0, 5), (10, 0), (1000, 300), (300, 1000), (777, 777)):
        x = rng.standard_normal(s_len)
        x[:2] = [-0.0, 5e-324][:min(2, s_len)]
        assert np.array_equal(_bits(ref.warp_one(x, n, [])), _bits(length_fit(x, n)))
        assert np.array_equal(_bits(ref.warp_one(x, n, [3, 4], valid=False)), _bits(length_fit(x, n)))
    sounds = [rng.standard_normal(500), rng.standard_normal(900)]
    off = np.array([0, 600, 600, 1500])
    out = ref.warp(sounds, [1, 0, 0], off, np.array([7, 7, 7, 7], np.uint32), [0, 2, 2, 4], [0, 0, 2], pair_len=[1, 1, 0])
    want = np.concatenate([length_fit(sounds[1], 600), length_fit(sounds[0], 900)])
    assert np.array_equal(_bits(out), _bits(want))


def test_two_frames_worked_by_hand():
    # a source of 3 frames' worth of samples: 1.0 in its first hop, 0.0 in the second, 2.0 from there on
    x = np.concatenate([np.full(256, 1.0), np.zeros(256), np.full(1024, 2.0)])
    # target frame 0 plays source frame 1, target frame 1 plays source frame 0
    out = ref.warp_one(x, 1500, np.array([1, 0], dtype=np.uint32))
    w = ref.WINDOW
    # k = 100: one tap, frame 0 (m = 100) -> x[256 + 100] = 0.0
    assert _bits(out[100:101])[0] == 0
    # k = 300: frame 0 (m = 300) reads x[556] = 2.0, frame 1 (m = 44) reads x[44] = 1.0, in that order
    assert out[300] == (w[300] * 2.0 + w[44] * 1.0) / (w[300] + w[44])
    # k = 600: frame 0 (m = 600) reads x[856] = 2.0, frame 1 (m = 344) reads x[344] = 0.0
    assert out[600] == (w[600] * 2.0 + w[344] * 0.0) / (w[600] + w[344])
    # k = 1100: frame 0 has ended (m = 1100 >= 1024); frame 1 alone, m = 844, x[844] = 2.0: w * 2 / w is exact
    assert out[1100] == 2.0
    # k = 1279: the last sample any frame reaches (frame 1, m = 1023); from 1280 on nothing
    assert out[1279] == 2.0 and (_bits(out[1280:]) == 0).all()
    # k = 256: frame 0 with m = 256 (x[512] = 2.0) and frame 1 with m = 0, whose weight is exactly 0
    assert out[256] == (w[256] * 2.0 + 0.0 * 1.0) / (w[256] + 0.0) == 2.0
    assert np.array_equal(_bits(out), _bits(ref.warp_one_scalar(x, 1500, [1, 0])))


def test_pcm32_is_write_files_conversion():
    x = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, -2.0, float("nan"), 1e-12, -0.9999999999])
    got = ref.pcm32(x)
    assert got.dtype == np.int32
    assert got.tolist() == [0, 0, 2147483647, -2147483647, 1073741823, 2147483647, -2147483648, 0, 0, -2147483646]
