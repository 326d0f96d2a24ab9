"""Sound descriptors on the GPU (ssym_sound_descriptors / ssym_pitch_track) against the numpy restatement of
DESIGN.md 5.9 (tests/pitch_ref.py).

Parity with the REFERENCE is unpinned for the pitch side (vox_box is not vendored); what is checked is GPU ==
restatement.  max_power must be bit-equal to the sequential fold.  Frequencies, strengths and unvoiced strengths agree to
rtol 1e-11, and the chosen candidate (voiced or not, and its lag) is identical in every window whose two best
candidates the restatement puts more than 1e-9 apart.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pitch_ref as ref
import soundsym_amd._native as nat
from soundsym_amd import Engine, Partitioner, SsymError
from soundsym_amd.io import read_wav, read_wav_spec

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
AUDIO = os.path.join(HERE, "golden", "audio")
SECTION = os.path.join(AUDIO, "Section_7_1.wav")
RATE = 44100.0


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="refcos", dtype="f64")
    yield e
    e.close()


def _batch(parts):
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate(parts) if parts else np.zeros(0), off


def _synthetic():
    n = np.arange(3 * 8192)
    rng = np.random.default_rng(11)
    parts = [0.5 * np.sin(2 * np.pi * f * n[:8192] / RATE) for f in (100.5, 150.0, 220.0, 333.0, 490.0)]
    parts.append(sum(np.sin(2 * np.pi * 150.0 * k * n[:8192] / RATE) / k for k in range(1, 8)))
    parts.append(rng.normal(size=16384))
    loud = 0.8 * np.sin(2 * np.pi * 180.0 * n[:10240] / RATE)
    loud[4096:6144] = 0.0                                   # a silent window inside a loud sound: u = 2.2
    parts.append(loud)
    parts.append(np.zeros(5000))                            # G = 0: u = v
    bad = 0.3 * np.sin(2 * np.pi * 260.0 * n[:6144] / RATE)
    bad[50] = np.nan                                        # window 0 reports NaN, the fold skips it
    bad[3000] = np.inf                                      # ... and windows 1 and 2
    parts.append(bad)
    parts.append(np.zeros(0))
    parts.append(0.1 * np.sin(2 * np.pi * 300.0 * n[:2047] / RATE))
    return _batch(parts)


def _ragged(seed=7):
    """Empty sounds, the window-count edges, random lengths; 2^20 samples in all, the last window ending on the last
    sample."""
    rng = np.random.default_rng(seed)
    lens = [0, 2047, 0, 2048, 3071, 3072, 3073, 127, 128, 129, 1]
    lens += [int(v) for v in rng.integers(1000, 30000, 24)]
    s = sum(lens)
    lens.append((1024 - s % 1024) % 1024 + 1024)            # the sum becomes a multiple of 1024
    lens.append((1 << 20) - sum(lens))
    assert lens[-1] >= 2048 and (lens[-1] - 2048) % 1024 == 0 and sum(lens) == 1 << 20
    parts = []
    for L in lens:
        t = np.arange(L) / RATE
        f = rng.uniform(80.0, 600.0)
        x = rng.uniform(0.05, 1.0) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28))
        x = x + rng.uniform(0.0, 0.3) * rng.normal(size=L)
        if L > 4096 and rng.uniform() < 0.3:
            x[L // 3:L // 3 + 2500] = 0.0
        parts.append(x)
    return _batch(parts)


def _segments():
    p = Partitioner.from_path(SECTION).threshold(3).depth(4)
    p.train(seed=0)
    splits = p.partition()
    x, _ = read_wav(SECTION)
    parts, pos = [], 0
    for sp in splits:
        parts.append(x[pos:pos + sp])
        pos = min(pos + sp, x.size)
    return _batch(parts)


def _whole(name):
    x, _ = read_wav(os.path.join(AUDIO, name))
    return _batch([x])


CASES = {"synthetic": _synthetic, "ragged": _ragged, "sample": lambda: _whole("sample.wav"),
         "section": lambda: _whole("Section_7_1.wav"), "segments": _segments}


def _check(eng, x, off, **kw):
    mp, pc = eng.sound_descriptors(x, off, **kw)
    freq, st, u, woff = eng.pitch_track(x, off, **kw)
    mp_r, pc_r, pv_r, tracks = ref.descriptors(x, off, **kw)
    assert list(np.diff(woff)) == [len(t["freq"]) for t in tracks]
    assert np.array_equal(mp, mp_r), "max_power is not bit-equal to the sequential fold"
    assert np.allclose(pc, pc_r, rtol=1e-11, atol=0)
    cat = {k: np.concatenate([t[k] for t in tracks]) for k in tracks[0]} if tracks else {}
    if woff[-1] == 0:
        return mp, pc, pv_r
    nan = np.isnan(cat["unvoiced"])
    assert np.array_equal(np.isnan(u), nan) and np.array_equal(np.isnan(freq), nan) and np.array_equal(np.isnan(st), nan)
    ok = ~nan
    assert np.allclose(u[ok], cat["unvoiced"][ok], rtol=1e-11, atol=0)
    clear = ok & (cat["gap"] > 1e-9)
    assert np.allclose(freq[clear], cat["freq"][clear], rtol=1e-11, atol=0)
    assert np.allclose(st[clear], cat["strength"][clear], rtol=1e-11, atol=0)
    voiced = (freq > 0) & (st >= u)
    tau = np.where(voiced, np.rint(kw.get("rate", RATE) / np.where(freq > 0, freq, 1.0)), -1).astype(np.int64)
    assert np.array_equal(tau[clear], cat["tau"][clear]), "the chosen candidate differs"
    return mp, pc, pv_r


@pytest.mark.parametrize("name", list(CASES))
def test_descriptors_match_restatement(eng, name):
    x, off = CASES[name]()
    mp, pc, pv_r = _check(eng, x, off)
    # SSYM_PITCH_VOICED changes the confidence only
    mpv, pcv = eng.sound_descriptors(x, off, voiced_only=True)
    assert np.array_equal(mpv, mp)
    assert np.allclose(pcv, pv_r, rtol=1e-11, atol=0)
    t0, t1 = eng.pitch_track(x, off), eng.pitch_track(x, off, voiced_only=True)
    for a, b in zip(t0, t1):
        assert np.array_equal(a, b, equal_nan=True)
    # a second call gives the same bits
    mp2, pc2 = eng.sound_descriptors(x, off)
    assert mp2.tobytes() == mp.tobytes() and pc2.tobytes() == pc.tobytes()
    if name == "synthetic":
        assert pc[8] == 0.2 and pcv[8] == 0.0               # the all-zero sound
        assert pc[11] == 0.0 and pc[10] == 0.0              # shorter than a window; empty
        assert np.isfinite(pc[9])                           # the NaN / inf windows are skipped


def test_other_arguments(eng):
    x, off = _synthetic()
    _check(eng, x, off, rate=16000.0, f_min=60.0, f_max=400.0, voicing=0.45)
    _check(eng, x, off, rate=44100.0, f_min=44100.0 / 682, f_max=44100.0 / 2, voicing=0.0)


def test_offsets_need_not_start_at_zero(eng):
    x, off = _ragged(3)
    sub = off[5:12]
    mp, pc = eng.sound_descriptors(x, sub)
    mp_all, pc_all = eng.sound_descriptors(x, off)
    assert np.array_equal(mp, mp_all[5:11]) and np.array_equal(pc, pc_all[5:11])


def test_empty_calls(eng):
    mp, pc = eng.sound_descriptors(np.zeros(0), np.zeros(1, dtype=np.uint64))
    assert mp.size == 0 and pc.size == 0
    mp, pc = eng.sound_descriptors(np.zeros(0), np.zeros(4, dtype=np.uint64))
    assert list(mp) == [0.0] * 3 and list(pc) == [0.0] * 3


def test_invalid_limits_leave_the_context_usable(eng):
    L = nat.lib()
    x, off = _batch([np.sin(np.arange(5000) * 0.05)])
    mp, pc = np.zeros(1), np.zeros(1)
    bad = [(44100.0, 0.0, 500.0, 0.2), (44100.0, 500.0, 100.0, 0.2), (44100.0, 100.0, 44100.0, 0.2),
           (44100.0, 60.0, 500.0, 0.2), (0.0, 100.0, 500.0, 0.2), (float("nan"), 100.0, 500.0, 0.2),
           (44100.0, 100.0, 500.0, float("inf"))]
    for rate, lo, hi, v in bad:
        rc = L.ssym_sound_descriptors(eng.ctx, x.ctypes.data, off.ctypes.data, 1, rate, lo, hi, v, 0,
                                      mp.ctypes.data, pc.ctypes.data)
        assert rc == nat.SSYM_E_INVALID
        with pytest.raises(SsymError, match="ssym_sound_descriptors"):
            nat.check(rc, eng.ctx)
        rc = L.ssym_pitch_track(eng.ctx, x.ctypes.data, off.ctypes.data, 1, rate, lo, hi, v, 0, None, None, None)
        assert rc == nat.SSYM_E_INVALID
    assert mp[0] == 0.0 and pc[0] == 0.0                    # nothing written
    back = (ctypes.c_uint64 * 2)(10, 5)
    assert L.ssym_sound_descriptors(eng.ctx, x.ctypes.data, back, 1, 44100.0, 100.0, 500.0, 0.2, 0, None,
                                    None) == nat.SSYM_E_INVALID
    got = eng.sound_descriptors(x, off)
    want = ref.descriptors(x, off)
    assert np.array_equal(got[0], want[0]) and np.allclose(got[1], want[1], rtol=1e-11, atol=0)


@pytest.mark.parametrize("example,key", [("louder.py", "max_power"), ("pitch_order.py", "pitch_confidence")])
def test_example_orders_the_segments(eng, tmp_path, example, key):
    out = str(tmp_path / "out.wav")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", example), "-s", SECTION, "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    x, off = _segments()
    n = off.size - 1
    mp, pc = eng.sound_descriptors(x, off)
    values = mp if key == "max_power" else pc
    order = sorted(range(n), key=lambda i: values[i])
    y, rate, bits = read_wav_spec(out)
    _, rate_in, bits_in = read_wav_spec(SECTION)
    assert (rate, bits) == (rate_in, bits_in)
    segs = [x[int(off[i]):int(off[i + 1])] for i in range(n)]
    assert np.array_equal(y, np.concatenate([segs[i] for i in order]))
    assert sorted(s.tobytes() for s in segs) == sorted(segs[i].tobytes() for i in order)
    assert all(values[order[k]] <= values[order[k + 1]] for k in range(n - 1))
    assert r.stdout.count("sound: ") == n
