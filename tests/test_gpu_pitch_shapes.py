"""ssym_sound_descriptors and ssym_pitch_track at every lag range and grid size they accept, against tests/pitch_ref.py.

tests/test_gpu_pitch.py checks three lag ranges, all with an odd count nR = hi - lo + 3 of r(tau) values, about 1 000
windows and fewer than 200 peak chunks per call.  Here, with test_gpu_pitch._check's rules (max_power bit-equal, rtol
1e-11, the same candidate wherever the restatement's two best are more than 1e-9 apart):

  * lag ranges with hi == lo, hi = lo + 1, hi - lo around 256 (the voiced loop's second pass over 256 threads) and
    around 508 (the two-lag loop's, q <= (nR + 1) / 2), lo = 2 and hi = 682 (kMaxTau), each with both parities of nR,
    and at rates other than 44 100 Hz.  f_max = rate / (lo - 1/2) and f_min = rate / (hi + 1/2) put both quotients
    half-way between integers, so ceil and floor cannot round to a neighbour;
  * more than 2 * num_cus * 8 windows in one call (every pitch workgroup takes two or three windows), with NaN windows
    placed so that workgroups take a bad window and then a good one, and a good one and then a bad one;
  * more than 2 * num_cus * 8 peak chunks, from thousands of sounds shorter than one window and sounds of 8192 k +- 1
    samples (power windows that straddle a chunk end);
  * subnormal, huge and all-NaN samples, and voicing thresholds at and below -1 and far above 1.

tests/test_descriptor_boundaries.py checks these case lists against the constants of csrc/pitch.hip.
"""
import numpy as np
import pytest

import pitch_ref as ref
from soundsym_amd import engine as engine_mod
from test_gpu_pitch import _batch, _check, _synthetic

pytestmark = pytest.mark.gpu
CAP_FACTOR = 8                      # pitch.hip: grid = min(items, num_cus * 8)
W, H, CHUNK = 2048, 1024, 8192

# (rate, tau_lo, tau_hi)
LAG_CASES = [(44100.0, 100, 100), (44100.0, 100, 101),
             (44100.0, 89, 343), (44100.0, 89, 344), (44100.0, 89, 345), (44100.0, 89, 346),
             (44100.0, 40, 546), (44100.0, 40, 547), (44100.0, 40, 548), (44100.0, 40, 549), (44100.0, 40, 550),
             (44100.0, 2, 40), (44100.0, 2, 41), (44100.0, 300, 682), (44100.0, 301, 682),
             (8000.0, 2, 682), (8000.0, 2, 681), (96000.0, 2, 2), (96000.0, 2, 3), (16000.0, 681, 682),
             (22050.0, 682, 682)]
VOICINGS = [-2.0, -1.0, -0.5, 1e3]
NARROW = (44100.0, 200, 215)        # 16 lags: the restatement's cost grows with windows x lags
SHORT_LENGTHS = [1, 127, 128, 129, 191, 192, 1000, 2047]
CHUNK_EDGE_LENGTHS = [CHUNK * k + d for k in (1, 2, 3) for d in (-1, 0, 1)]


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def limits(rate, lo, hi):
    """(f_min, f_max) whose lag range is (lo, hi): both quotients half-way between integers."""
    return rate / (hi + 0.5), rate / (lo - 0.5)


@pytest.fixture(scope="module")
def eng():
    from soundsym_amd import Engine
    e = Engine(metric="refcos", dtype="f64")
    yield e
    e.close()


def _periodic(n, period, seed, noise=0.1):
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * np.arange(n) / period + rng.uniform(0, 6.28)
    return 0.6 * np.sin(ph) + 0.3 * np.sin(2 * ph + 1.0) + noise * rng.normal(size=n)


def _kw(rate, lo, hi, **extra):
    f_min, f_max = limits(rate, lo, hi)
    return dict(rate=rate, f_min=f_min, f_max=f_max, **extra)


# ---- lag ranges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,lo,hi", LAG_CASES)
def test_lag_ranges(eng, rate, lo, hi):
    kw = _kw(rate, lo, hi)
    assert ref.lag_range(rate, kw["f_min"], kw["f_max"]) == (lo, hi)
    assert engine_mod.pitch_lags(rate, kw["f_min"], kw["f_max"]) == (lo, hi)
    n = W + 4 * H                                         # 5 windows per sound
    periods = [max(lo, 2), hi, max(0.5 * (lo + hi) + 0.37, 2.0)]
    parts = [_periodic(n, p, 7 * lo + hi + i) for i, p in enumerate(periods)]
    parts.append(np.random.default_rng(lo + hi).normal(size=n))
    parts.append(np.zeros(0))
    x, off = _batch(parts)
    _, _, pv = _check(eng, x, off, **kw)
    _, pcv = eng.sound_descriptors(x, off, voiced_only=True, **kw)
    assert np.allclose(pcv, pv, rtol=1e-11, atol=0)
    _, _, _, tracks = ref.descriptors(x, off, **kw)
    assert any(np.any(t["tau"] >= 0) for t in tracks), "no window chose a voiced candidate"


# ---- voicing thresholds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voicing", VOICINGS)
def test_voicing_thresholds(eng, voicing):
    x, off = _synthetic()
    with np.errstate(all="ignore"):
        mp, pc, pv = _check(eng, x, off, voicing=voicing)
    mpv, pcv = eng.sound_descriptors(x, off, voicing=voicing, voiced_only=True)
    assert np.array_equal(mpv, mp) and np.allclose(pcv, pv, rtol=1e-11, atol=0)
    if voicing == -1.0:                                   # sigma / (1 + v) = inf: u = v + 2 wherever G > 0
        assert pc[8] == 0.0                               # the all-zero sound: u = v = -1, the fold keeps 0
    if voicing == 1e3:
        assert np.all(pc[:10] >= 1e3)


# ---- windows past the grid --------------------------------------------------------------------------------------------
def window_case(cus):
    """(lengths, global indices of the windows poisoned by a NaN) for more than 2 * cap windows, cap = cus * 8:
    a short sound, a 3-window sound, then one long sound; a NaN at sample 1024 t + 1500 of a sound poisons its windows
    t and t + 1."""
    cap = cus * CAP_FACTOR
    total = 2 * cap + 37
    w = [1, 3, total - 4]
    lengths = [W + 500, W + (w[1] - 1) * H + 1000, W + (w[2] - 1) * H]
    first = [0, 1, 4]
    poison = [17, cap + 40, 100, cap + 100, 2 * cap + 31]       # local t in the long sound, t + 1 also bad
    bad = sorted({first[2] + t + d for t in poison for d in (0, 1)} | {first[1] + 1, first[1] + 2})
    return lengths, poison, bad


def test_windows_past_the_grid(eng):
    cus = num_cus()
    cap = cus * CAP_FACTOR
    lengths, poison, bad = window_case(cus)
    rate, lo, hi = NARROW
    parts = []
    for i, n in enumerate(lengths):
        t = np.arange(n) / rate
        f = rate / (lo + 1.5) + (rate / (hi - 1.5) - rate / (lo + 1.5)) * t / t[-1]      # a slow sweep within the range
        ph = 2 * np.pi * np.cumsum(f) / rate
        parts.append(0.5 * np.sin(ph) + 0.2 * np.sin(3 * ph) + 0.05 * np.random.default_rng(i).normal(size=n))
    for t in poison:
        parts[2][H * t + 1500] = np.nan
    parts[1][H + 1500] = np.nan                           # windows 1 and 2 of the 3-window sound: its last two
    x, off = _batch(parts)
    kw = _kw(rate, lo, hi)
    assert ref.lag_range(rate, kw["f_min"], kw["f_max"]) == (lo, hi)
    _check(eng, x, off, **kw)
    freq, _, _, woff = eng.pitch_track(x, off, **kw)
    assert woff[-1] > 2 * cap
    isbad = np.isnan(freq)
    assert sorted(np.nonzero(isbad)[0].tolist()) == bad
    assert any(isbad[g] and not isbad[g + cap] for g in range(woff[-1] - cap))      # bad, then good
    assert any(not isbad[g] and isbad[g + cap] for g in range(woff[-1] - cap))      # good, then bad


# ---- peak chunks past the grid ----------------------------------------------------------------------------------------
def chunk_case(cus):
    """Lengths: 2 * cap + 50 sounds shorter than one window (one chunk each, no pitch window), then sounds of
    8192 k - 1, 8192 k, 8192 k + 1 samples."""
    cap = cus * CAP_FACTOR
    short = [SHORT_LENGTHS[i % len(SHORT_LENGTHS)] for i in range(2 * cap + 50)]
    return short + CHUNK_EDGE_LENGTHS


def n_chunks(lengths):
    return sum(-(-n // CHUNK) for n in lengths)


def test_chunks_past_the_grid(eng):
    cus = num_cus()
    lengths = chunk_case(cus)
    rng = np.random.default_rng(41)
    parts = [rng.uniform(0.01, 2.0) * _periodic(n, rng.uniform(90.0, 440.0), i) for i, n in enumerate(lengths)]
    x, off = _batch(parts)
    assert n_chunks(lengths) > 2 * cus * CAP_FACTOR
    mp, _, _ = _check(eng, x, off)
    assert np.all(mp[np.array(lengths) >= 128] > 0.0) and np.all(mp[np.array(lengths) < 128] == 0.0)


# ---- input values -----------------------------------------------------------------------------------------------------
def test_extreme_and_non_finite_samples(eng):
    base = _periodic(3 * CHUNK + 77, 180.0, 5)
    parts = [1e-310 * base, 1e200 * base, np.full(6000, np.nan), base[:9000], 1e-310 * base[:1000]]
    x, off = _batch(parts)
    assert 0 < abs(x[1]) < np.finfo(np.float64).tiny                        # subnormal samples
    for kw in ({}, _kw(8000.0, 2, 682), _kw(44100.0, 100, 100)):
        with np.errstate(all="ignore"):
            mp, pc, _ = _check(eng, x, off, **kw)
        assert mp[0] == 0.0 and mp[1] == np.inf and mp[2] == 0.0       # x * x underflows / overflows; NaN skipped
        assert pc[2] == 0.0                                              # every window NaN: the fold keeps 0
