"""ssym_mfcc and ssym_mfcc_batch at every shape they accept, against the C oracle and against each other.

tests/test_gpu_mfcc.py checks 12, 13 and 20 coefficients on the default band and at most 169 frames per call.  This file
covers what lies between and beyond (tests/test_descriptor_boundaries.py checks that the case lists below straddle the
kernel's constants): 1 to 64 coefficients (4 to 130 = kMaxFilters filters), bands whose lowest filters are narrower than
one bin (no non-zero weight: their energy is the 1e-30 floor), bands up to and past rate / 2, six sample rates, frame
counts around the grid cap (num_cus * 16 workgroups, so a workgroup takes a second frame), a ragged batch of thousands of
sounds, extreme and non-finite samples, and the rejected inverted band.

Tolerance.  FFT, spectrum, filter sums and DCT have the same operands and operation order on both sides; only ln() is
each side's libm.  With each ln within a few ulps, |dL_m| <= k ulp(L_m) <= k 2^-52 |L_m|, and the DCT carries that
into c_j as at most k 2^-52 S_j, S_j = sum_m |d_jm| |L_m| (k = 4: two ulps for either library).  The bound is
max(TOL (1 + |want|), 4 * 2^-52 * S_j).  The first term is the suite's tolerance and is the larger one wherever
|c_j| is not small against S_j.  The second takes over only where the DCT cancels: for nf = 130 filters all on the floor,
L_m = ln(1e-30) = -69.08, S_j is about 5.7e3, the bound about 5e-12, and the coefficients themselves are
rounding residue near 0.  S_j is computed from a numpy restatement of the log energies.  Its FFT is not the device's,
but its relative error is far below the factor this bound leaves.
"""
import math

import numpy as np
import pytest

import soundsym_amd._native as nat
from soundsym_amd import Engine, Sound, SsymError
from test_gpu_sequence import _mean_fold, _same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-12
EPS = 2.0 ** -52
BIN, HOP, SPEC = 1024, 256, 513
GRID_FACTOR = 16                                   # mfcc.hip: grid = min(frames, num_cus * 16)

NCS = [1, 2, 7, 8, 12, 20, 31, 32, 33, 40, 63, 64]
RATES = [8000.0, 16000.0, 22050.0, 44100.0, 48000.0, 96000.0]
# (label, rate, n_coeffs, f_lo, f_hi, filters with no weight: "none", "some" or "all")
BANDS = [("default", 44100.0, 12, 100.0, 8000.0, "none"),
         ("f_lo=0", 44100.0, 20, 0.0, 8000.0, "none"),
         ("f_lo=0,nyquist_64", 22050.0, 64, 0.0, 11025.0, "none"),
         ("nyquist", 48000.0, 33, 100.0, 24000.0, "none"),
         ("above_nyquist", 16000.0, 13, 100.0, 12000.0, "none"),
         ("above_nyquist_64", 8000.0, 64, 100.0, 1e6, "none"),
         ("narrow_64", 44100.0, 64, 100.0, 1200.0, "some"),
         ("sub_bin", 44100.0, 12, 1000.0, 1020.0, "all"),
         ("sub_bin_64", 96000.0, 64, 3010.0, 3060.0, "all"),
         ("just_below_nyquist", 8000.0, 7, 3990.0, 4000.0, "some")]
# lengths of the large batch: around one window, one window + one hop, and many empty sounds
BATCH_LENGTHS = [0, 0, 0, 1023, 1024, 1025, 1279, 1280, 1281, 255, 256, 2048]
BATCH_SOUNDS = 9000
BATCH_NC = 64


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def grid_frames(cus):
    """Frame counts of one call around the grid cap: a workgroup with no second frame, exactly one frame each, one
    workgroup with two, every workgroup with two or three."""
    cap = cus * GRID_FACTOR
    return [cap - 1, cap, cap + 1, 2 * cap + 3]


def batch_lengths(seed=5):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.choice(BATCH_LENGTHS, BATCH_SOUNDS)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="refcos", dtype="f64")
    yield e
    e.close()


def _signal(n, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    f = rng.uniform(80.0, 0.45 * rate)
    return (0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * f * t + 1.0)
            + 0.05 * rng.normal(size=n))


def _batch(parts):
    parts = [np.asarray(p, dtype=np.float64).reshape(-1) for p in parts]
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return (np.concatenate(parts) if parts else np.zeros(0)), off


# ---- a numpy restatement of the host tables (mfcc.hip build_tables): weights, their bin ranges, the DCT ------------
def _mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def _hz(m):
    return 700.0 * (math.exp(m / 1127.0) - 1.0)


def filterbank(rate, nc, f_lo, f_hi):
    """(weights [nf][513], lo [nf], hi [nf]) as build_tables forms them (math.log / exp are the host's libm, so the
    ranges are the same integers); lo = hi = 0 for a filter without a non-zero weight."""
    nf = 2 * nc + 2
    top = min(f_hi, 0.5 * rate)
    m0, m1 = _mel(f_lo), _mel(top)
    f = np.arange(SPEC, dtype=np.float64) * rate / float(BIN)
    W = np.zeros((nf, SPEC))
    lo, hi = np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
    for m in range(nf):
        h0 = _hz(m0 + (m1 - m0) * m / (nf + 1))
        h1 = _hz(m0 + (m1 - m0) * (m + 1) / (nf + 1))
        h2 = _hz(m0 + (m1 - m0) * (m + 2) / (nf + 1))
        up = (f > h0) & (f <= h1)
        down = ~up & (f > h1) & (f < h2)
        with np.errstate(divide="ignore", invalid="ignore"):
            W[m] = np.where(up, (f - h0) / (h1 - h0), np.where(down, (h2 - f) / (h2 - h1), 0.0))
        nz = np.nonzero(W[m])[0]
        if nz.size:
            lo[m], hi[m] = nz[0], nz[-1] + 1
    return W, lo, hi


def dct_matrix(nc):
    nf = 2 * nc + 2
    j = np.arange(1, nc + 1, dtype=np.float64)[:, None]
    m = np.arange(nf, dtype=np.float64)[None, :]
    return np.cos(np.pi * j * (m + 0.5) / nf)


def log_energies(x, rate, nc, f_lo, f_hi, pad_tail=False):
    """L [frames][nf] = ln(max(E, 1e-30)) by numpy's FFT (for the error bound only)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    T = Engine.mfcc_num_frames(x.size, pad_tail)
    xp = np.concatenate([x, np.zeros(BIN)])
    frames = np.lib.stride_tricks.sliding_window_view(xp, BIN)[::HOP][:T]
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(BIN) / BIN)
    with np.errstate(all="ignore"):
        P = np.abs(np.fft.rfft(frames * win, axis=1)) ** 2
        E = P @ filterbank(rate, nc, f_lo, f_hi)[0].T
        return np.log(np.fmax(E, 1e-30))


def assert_close(got, want, L, nc):
    """|got - want| <= max(TOL (1 + |want|), 4 * 2^-52 * S), S[t][j] = sum_m |d_jm| |L[t][m]| (module docstring);
    non-finite values in the same places, with the same bits where they are infinite."""
    got, want = np.asarray(got).reshape(-1, nc), np.asarray(want).reshape(-1, nc)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN in other places than the oracle's"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    ok = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        S = np.abs(L) @ np.abs(dct_matrix(nc)).T
    bound = np.maximum(TOL * (1.0 + np.abs(want)), np.where(np.isfinite(S), 4.0 * EPS * S, 0.0))
    err = np.abs(got - want)
    assert np.all(err[ok] <= bound[ok]), float(np.max(np.where(ok, err - bound, -np.inf)))


def _check_single(eng, oracle, x, rate, nc, f_lo=100.0, f_hi=8000.0, pad=False):
    got = eng.mfcc(x, rate, nc, f_lo, f_hi, pad_tail=pad)
    want = oracle.mfcc(x, rate, nc, f_lo, f_hi, pad_tail=pad)
    assert got.shape == want.shape == (Engine.mfcc_num_frames(x.size, pad), nc)
    if want.size:
        assert_close(got, want, log_energies(x, rate, nc, f_lo, f_hi, pad), nc)
    return got


def _check_batch_vs_single(eng, parts, rate, nc, f_lo=100.0, f_hi=8000.0, pad=False):
    x, off = _batch(parts)
    feats, fo, mean = eng.mfcc_batch(x, off, rate, nc, f_lo, f_hi, pad_tail=pad, want_mean=True)
    for i, p in enumerate(parts):
        single = eng.mfcc(p, rate, nc, f_lo, f_hi, pad_tail=pad)
        assert np.array_equal(feats[int(fo[i]):int(fo[i + 1])], single), f"sound {i} ({p.size} samples)"
        assert _same_bits(mean[i], _mean_fold(single, nc))
    return feats, fo


# ---- A. coefficients ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("nc", NCS)
def test_every_coefficient_count(eng, oracle, nc, pad):
    rate = 44100.0
    parts = [_signal(n, rate, 10 * nc + k) for k, n in enumerate([5000, 0, 1023, 1300, 255, 3000])]
    for p in parts:
        _check_single(eng, oracle, p, rate, nc, pad=pad)
    _check_batch_vs_single(eng, parts, rate, nc, pad=pad)


# ---- A. bands and rates ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,rate,nc,f_lo,f_hi,empty", BANDS, ids=[b[0] for b in BANDS])
def test_bands(eng, oracle, label, rate, nc, f_lo, f_hi, empty):
    _, lo, hi = filterbank(rate, nc, f_lo, f_hi)
    none = hi == 0
    assert {"none": not none.any(), "some": none.any() and not none.all(), "all": none.all()}[empty]
    assert np.all((lo < hi) | ((lo == 0) & (hi == 0)))
    parts = [_signal(n, rate, 7 + k) for k, n in enumerate([6000, 1024, 2500])]
    for p in parts:
        got = _check_single(eng, oracle, p, rate, nc, f_lo, f_hi)
        if empty == "all":
            # every log energy is ln(1e-30): the frames are the DCT of a constant, the same for every window
            assert np.all(got == got[0]) and np.all(np.abs(got) < 1e-10)
    _check_batch_vs_single(eng, parts, rate, nc, f_lo, f_hi, pad=True)


@pytest.mark.parametrize("rate", RATES)
def test_rates(eng, oracle, rate):
    x = _signal(12000, rate, int(rate))
    for nc, f_lo, f_hi in ((12, 100.0, 8000.0), (64, 0.0, 0.5 * rate), (20, 50.0, 2.0 * rate)):
        _check_single(eng, oracle, x, rate, nc, f_lo, f_hi, pad=True)


# ---- A. grid: frame counts around num_cus * 16 ------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4))
def test_grid_single_call(eng, oracle, which):
    T = grid_frames(num_cus())[which]
    rate = 44100.0
    x = _signal(BIN + HOP * (T - 1), rate, T)
    _check_single(eng, oracle, x, rate, 12)
    _check_single(eng, oracle, x[:HOP * T], rate, 12, pad=True)        # the same frame count, tail padded


@pytest.mark.parametrize("which", range(4))
def test_grid_batch(eng, oracle, which):
    T = grid_frames(num_cus())[which]
    rate = 16000.0
    rng = np.random.default_rng(T)
    counts = []
    while sum(counts) < T:
        counts.append(int(min(rng.integers(1, 400), T - sum(counts))))
    counts.insert(len(counts) // 2, 0)
    parts = [_signal(HOP * c + int(rng.integers(0, HOP)), rate, 1000 + i) for i, c in enumerate(counts)]
    assert sum(Engine.mfcc_num_frames(p.size, True) for p in parts) == T
    # the batch first (its output buffer must not hold an earlier call's frames), then every sound alone
    feats, fo = _check_batch_vs_single(eng, parts, rate, 13, pad=True)
    assert feats.shape == (T, 13)
    want = np.concatenate([oracle.mfcc(p, rate, 13, pad_tail=True) for p in parts])
    L = np.concatenate([log_energies(p, rate, 13, 100.0, 8000.0, True) for p in parts])
    assert_close(feats, want, L, 13)


# ---- A. the large ragged batch --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_batch(eng):
    rate = 44100.0
    lens = batch_lengths()
    rng = np.random.default_rng(9)
    parts = [rng.uniform(0.05, 1.0) * _signal(n, rate, i) for i, n in enumerate(lens)]
    x, off = _batch(parts)
    feats, fo, mean = eng.mfcc_batch(x, off, rate, BATCH_NC, pad_tail=True, want_mean=True)
    return rate, lens, parts, x, off, feats, fo, mean


def test_large_batch_against_oracle_and_single_calls(eng, oracle, big_batch):
    rate, lens, parts, x, off, feats, fo, mean = big_batch
    counts = [Engine.mfcc_num_frames(n, True) for n in lens]
    assert fo.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    cus = num_cus()
    assert int(fo[-1]) > 2 * cus * GRID_FACTOR and BATCH_SOUNDS * BATCH_NC > cus * 8 * 256
    want = np.concatenate([oracle.mfcc(p, rate, BATCH_NC, pad_tail=True) for p in parts])
    L = np.concatenate([log_energies(p, rate, BATCH_NC, 100.0, 8000.0, True) for p in parts])
    assert_close(feats, want, L, BATCH_NC)
    # every length class, and the sounds on either side of an empty one (among the first 400), each alone
    picks = {j for i in range(1, 400) if lens[i] == 0 for j in (i - 1, i + 1)}
    picks |= {lens.index(n) for n in set(lens)} | {len(lens) - 1}
    for i in sorted(picks):
        assert np.array_equal(feats[int(fo[i]):int(fo[i + 1])], eng.mfcc(parts[i], rate, BATCH_NC, pad_tail=True))
    # the means: Sound.mean_mfccs()'s fold, NaN for a sound without frames
    for i in range(len(parts)):
        assert _same_bits(mean[i], _mean_fold(feats[int(fo[i]):int(fo[i + 1])], BATCH_NC)), i
        assert np.all(np.isnan(mean[i])) == (counts[i] == 0)
    for i in sorted(picks)[:20]:
        if counts[i]:
            s = Sound(parts[i], rate, feats[int(fo[i]):int(fo[i + 1])].reshape(-1), None, BATCH_NC)
            assert _same_bits(mean[i], s.mean_mfccs())


def test_large_batch_offsets_device_output_and_one_sound(eng, big_batch):
    import torch
    rate, lens, parts, x, off, feats, fo, mean = big_batch
    # offsets that do not start at 0: the sounds [k, n) of the same samples
    k = 1237
    sub_feats, sub_fo, sub_mean = eng.mfcc_batch(x, off[k:], rate, BATCH_NC, pad_tail=True, want_mean=True)
    assert int(off[k]) > 0 and np.array_equal(sub_fo, fo[k:] - fo[k])
    assert np.array_equal(sub_feats, feats[int(fo[k]):]) and _same_bits(sub_mean, mean[k:])
    # SSYM_OUT_DEVICE at the full size
    out = torch.full((int(fo[-1]) * BATCH_NC,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t, tfo, tmean = eng.mfcc_batch(x, off, rate, BATCH_NC, pad_tail=True, want_mean=True, out=out)
    assert t is out and np.array_equal(tfo, fo) and _same_bits(tmean, mean)
    assert np.array_equal(out.cpu().numpy().reshape(-1, BATCH_NC), feats)
    # n_sounds = 1
    i = lens.index(2048)
    one, ofo, omean = eng.mfcc_batch(parts[i], [0, lens[i]], rate, BATCH_NC, pad_tail=True, want_mean=True)
    assert ofo.tolist() == [0, 8] and np.array_equal(one, feats[int(fo[i]):int(fo[i + 1])])
    assert _same_bits(omean[0], mean[i])


# ---- A. input values ------------------------------------------------------------------------------------------------
def test_extreme_amplitudes(eng, oracle):
    rate = 44100.0
    base = _signal(6000, rate, 31)
    for amp in (1e-160, 1e150):
        x = amp * base
        for nc in (12, 64):
            got = _check_single(eng, oracle, x, rate, nc)
            assert np.all(np.isfinite(got))
            if amp < 1:        # every energy under the floor: the frames of silence
                floor = eng.mfcc(np.zeros(BIN), rate, nc)
                assert np.array_equal(got, np.repeat(floor, got.shape[0], axis=0))
        _check_batch_vs_single(eng, [x, base, x[:3000]], rate, 64)


def test_non_finite_samples(eng, oracle):
    """Pinned: a window holding a NaN has NaN energies, which the floor max(E, 1e-30) turns into
    1e-30 on both sides -- its coefficients are finite and equal to those of a silent window.  A window holding an
    infinity gives what the same operations give on the oracle: NaN or infinite coefficients in the same places, the
    same infinities, the finite ones within the bound."""
    rate = 44100.0
    x = _signal(BIN + HOP * 39, rate, 41)                  # 40 frames
    nan_at, inf_at = HOP * 5 + 700, HOP * 30 + 10
    x[nan_at] = np.nan
    x[inf_at] = np.inf
    holds = lambda s: {t for t in range(40) if HOP * t <= s < HOP * t + BIN}      # noqa: E731
    assert holds(nan_at) == {4, 5, 6, 7} and holds(inf_at) == {27, 28, 29, 30}
    got = _check_single(eng, oracle, x, rate, 12)
    for nc in (1, 64):
        _check_single(eng, oracle, x, rate, nc, pad=True)
    floor = eng.mfcc(np.zeros(BIN), rate, 12)[0]
    for t in holds(nan_at):
        assert np.array_equal(got[t], floor)
    for t in set(range(40)) - holds(nan_at) - holds(inf_at):
        assert np.all(np.isfinite(got[t])) and not np.array_equal(got[t], floor)
    _check_batch_vs_single(eng, [x, _signal(3000, rate, 1), x[:HOP * 6 + BIN]], rate, 12)


# ---- A. the inverted band ---------------------------------------------------------------------------------------------
def test_inverted_band_is_rejected(eng, oracle):
    L = nat.lib()
    x = _signal(4096, 8000.0, 3)
    out = np.full(13 * 12, 7.0)
    mean = np.full(2 * 12, 7.0)
    fo = np.full(3, 7, dtype=np.uint64)
    off = np.array([0, 2048, 4096], dtype=np.uint64)
    for rate, f_lo, f_hi in ((8000.0, 5000.0, 8000.0), (8000.0, 4000.0, 8000.0), (16000.0, 8000.0, 8001.0)):
        rc = L.ssym_mfcc(eng.ctx, x.ctypes.data, x.size, rate, 12, f_lo, f_hi, 0, out.ctypes.data, mean.ctypes.data)
        assert rc == nat.SSYM_E_INVALID
        assert b"f_lo" in L.ssym_last_error(eng.ctx)
        rc = L.ssym_mfcc_batch(eng.ctx, x.ctypes.data, off.ctypes.data, 2, rate, 12, f_lo, f_hi, 0, fo.ctypes.data,
                               out.ctypes.data, mean.ctypes.data)
        assert rc == nat.SSYM_E_INVALID
        with pytest.raises(SsymError) as ei:
            eng.mfcc(x, rate, 12, f_lo, f_hi)
        assert ei.value.code == nat.SSYM_E_INVALID
    assert np.all(out == 7.0) and np.all(mean == 7.0) and np.all(fo == 7)
    # the context is still usable, and a band that starts just below rate / 2 is accepted
    _check_single(eng, oracle, x, 8000.0, 12, 100.0, 8000.0)
    _check_single(eng, oracle, x, 8000.0, 12, 3999.0, 8000.0)
