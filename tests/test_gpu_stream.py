"""Streaming sounds on the GPU (ssym_stream).

The rule: after any sequence of pushes a lane holds, BIT FOR BIT, what ssym_mfcc (frames), ssym_mfcc_batch (mean) and
ssym_sound_descriptors (max_power) return for the concatenated samples.  Every comparison against those is
np.array_equal; the oracle (1e-12 * (1 + |oracle|), the tolerance of tests/test_gpu_mfcc.py) and tests/pitch_ref.py's
max_power (exact) are consulted once per case.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import pitch_ref
import soundsym_amd._native as nat
from soundsym_amd import Engine, Sound, push_sounds
from soundsym_amd.api import init_rows
from soundsym_amd.io import read_wav

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIO = os.path.join(ROOT, "tests", "golden", "audio")
TOL = 1e-12
CHUNKS = (1, 255, 256, 257, 767, 768, 1023, 1024, 1025, 4096)


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="refcos", dtype="f64")
    yield e
    e.close()


def _signal(n, rate=44100.0, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    return 0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 3000.0 * t + 1.0) + 0.05 * rng.normal(size=n)


def _whole(eng, x, rate=44100.0, nc=12, f_lo=100.0, f_hi=8000.0):
    """(frames, max_power, mean) of the sound analysed whole, by the three calls the stream must equal"""
    frames = eng.mfcc(x, rate, nc, f_lo, f_hi)
    power = eng.sound_descriptors(x, [0, x.size])[0][0]
    mean = eng.mfcc_batch(x, [0, x.size], rate, nc, f_lo, f_hi, want_mean=True)[2][0]
    return frames, power, mean


def _check_lane(eng, st, lane, x, rate=44100.0, nc=12, f_lo=100.0, f_hi=8000.0):
    frames, power, mean = _whole(eng, x, rate, nc, f_lo, f_hi)
    ns, nf = st.counts()
    assert int(ns[lane]) == x.size and int(nf[lane]) == Engine.mfcc_num_frames(x.size) == frames.shape[0]
    got = st.read(lane)
    mp, mn = st.descriptors()
    assert np.array_equal(got, frames, equal_nan=True)
    assert np.array_equal(mp[lane], power, equal_nan=True)
    assert np.array_equal(mn[lane], mean, equal_nan=True)
    return got, mp[lane], mn[lane]


def _check_oracle(oracle, x, got, power, rate=44100.0, nc=12):
    want = oracle.mfcc(x, rate, nc)
    assert got.shape == want.shape and np.all(np.abs(got - want) <= TOL * (1.0 + np.abs(want)))
    assert power == pitch_ref.max_power(x)


# ---- equality with whole-sound analysis ----------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 1, 600, 1023, 3000])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_pushes_equal_whole_sound(eng, oracle, start, chunk):
    pushes = 40 if chunk == 1 else 7
    x = _signal(start + pushes * chunk + 1024, seed=start * 31 + chunk)
    st = eng.stream(1, 44100.0)
    at = start
    if start >= 1024:          # a sound that already has frames
        st.seed(0, x[:start], eng.mfcc(x[:start], 44100.0))
    elif start:
        assert int(st.push(x[:start])[0]) == 0
    _check_lane(eng, st, 0, x[:at])
    for _ in range(pushes):
        before = Engine.mfcc_num_frames(at)
        new = st.push(x[at:at + chunk])
        at += chunk
        assert int(new[0]) == Engine.mfcc_num_frames(at) - before
        got, power, _ = _check_lane(eng, st, 0, x[:at])
    _check_oracle(oracle, x[:at], got, power)
    st.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_chunks_equal_whole_sound(eng, oracle, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 3000, size=25)
    x = _signal(int(sizes.sum()), seed=seed) if seed != 2 else np.sin(0.05 * np.arange(int(sizes.sum())))   # a pure tone
    st = eng.stream(1, 44100.0)
    at = 0
    for k in sizes:
        st.push(x[at:at + int(k)])
        at += int(k)
        got, power, _ = _check_lane(eng, st, 0, x[:at])
    _check_oracle(oracle, x, got, power)
    st.close()


def test_the_references_two_cases(eng):
    """test_push_samples and test_empty_sound (src/sound.rs:617-631): 5120 samples, 17 frames with HOP = 256 (their
    `5` holds for HOP = 1024)."""
    s = Sound.from_samples(np.zeros(2048), 44100.0, None, engine=eng)
    s.push_samples(np.zeros(3072), engine=eng)
    assert s.samples().size == 5120 and s.num_frames() == 17 and s.mfcc_arrays().shape == (17, 12)
    t = Sound.from_samples(np.zeros(0), 44100.0, None, engine=eng)
    assert t.num_frames() == 0
    t.push_samples(np.zeros(5120), engine=eng)
    assert t.samples().size == 5120 and t.num_frames() == 17
    assert np.array_equal(s.mfccs(), t.mfccs()) and np.array_equal(s.mfccs(), eng.mfcc(np.zeros(5120), 44100.0).reshape(-1))


# ---- lanes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lanes", [1, 2, 7, 64])
def test_lanes_equal_one_lane_streams(eng, n_lanes):
    rng = np.random.default_rng(n_lanes)
    st = eng.stream(n_lanes, 44100.0)
    singles = [eng.stream(1, 44100.0) for _ in range(n_lanes)]
    held = [np.zeros(0) for _ in range(n_lanes)]
    for rnd in range(5):
        sizes = rng.integers(0, 2500, size=n_lanes)
        sizes[rng.random(n_lanes) < 0.3] = 0                     # some chunks are empty
        sizes[rng.random(n_lanes) < 0.2] = 100                   # ... and some complete no frame
        if n_lanes >= 2:
            sizes[0] = 90 // 5 if rnd < 5 else 0                 # lane 0 never reaches 128 samples
            sizes[1] = 150                                       # lane 1 never reaches 1024
        parts = [_signal(int(k), seed=1000 * rnd + l) for l, k in enumerate(sizes)]
        off = np.concatenate([[0], np.cumsum(sizes)])
        new = st.push(np.concatenate(parts), off)
        for l in range(n_lanes):
            assert int(new[l]) == int(singles[l].push(parts[l])[0])
            held[l] = np.concatenate([held[l], parts[l]])
        ns, nf = st.counts()
        mp, mn = st.descriptors()
        for l in range(n_lanes):
            sp, sm = singles[l].descriptors()
            assert int(ns[l]) == held[l].size and int(nf[l]) == Engine.mfcc_num_frames(held[l].size)
            assert np.array_equal(st.read(l), singles[l].read(0))
            assert np.array_equal(mp[l], sp[0]) and np.array_equal(mn[l], sm[0], equal_nan=True)
    if n_lanes >= 2:
        assert held[0].size < 128 and mp[0] == 0.0 and int(nf[0]) == 0
        assert held[1].size < 1024 and int(nf[1]) == 0 and np.all(np.isnan(mn[1])) and mp[1] > 0.0
    for l in (0, n_lanes // 2, n_lanes - 1):
        _check_lane(eng, st, l, held[l])
    for s in singles + [st]:
        s.close()


# ---- seeding -------------------------------------------------------------------------------------------------------------
def test_seeding(eng):
    x = _signal(9000, seed=5)
    a, b = x[:5000], x[5000:]
    fa = eng.mfcc(a, 44100.0)
    st = eng.stream(4, 44100.0)
    off = lambda lane, n: [0] * (lane + 1) + [n] * (4 - lane)            # a chunk for one lane only
    st.push(a, off(0, a.size))                    # lane 0: pushed everything
    st.seed(1, a, fa)                             # lane 1: seeded with the features
    st.seed(2, a)                                 # lane 2: seeded without
    st.seed(3, a, fa[:7])                         # lane 3: fewer frames than the samples allow (16)
    ns, nf = st.counts()
    assert list(nf) == [16, 16, 16, 7] and list(ns) == [5000] * 4
    mp, mn = st.descriptors()
    assert mp[0] == mp[1] == mp[2] == mp[3] and np.array_equal(mn[0], mn[1]) and np.array_equal(mn[0], mn[2])
    assert np.array_equal(st.read(1), st.read(0)) and np.array_equal(st.read(2), st.read(0))
    new = st.push(np.concatenate([b] * 4), [0, 4000, 8000, 12000, 16000])
    assert list(new) == [16, 16, 16, 25]          # the 9 missing frames are analysed by this push
    for lane in range(4):
        _check_lane(eng, st, lane, x)
    # a lane that holds something, too many frames, a lane out of range: SSYM_E_INVALID, nothing changes
    before = (st.counts(), st.descriptors())
    for call in (lambda: st.seed(0, a, fa), lambda: st.seed(0, a)):
        with pytest.raises(nat.SsymError) as ei:
            call()
        assert ei.value.code == nat.SSYM_E_INVALID
    st.reset(2)
    with pytest.raises(nat.SsymError) as ei:
        st.seed(2, a[:4863], fa)            # 4863 samples hold 15 frames, fa has 16
    assert ei.value.code == nat.SSYM_E_INVALID
    assert list(st.counts()[1]) == [32, 32, 0, 32] and np.array_equal(st.descriptors()[0][[0, 1, 3]], before[1][0][[0, 1, 3]])
    st.seed(2, x, None)
    _check_lane(eng, st, 2, x)
    st.close()


# ---- growth --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [0, 300])
def test_growth_keeps_what_was_pushed(eng, capacity):
    x = _signal(70000, seed=9)
    st = eng.stream(2, 44100.0, capacity=capacity)
    at, early = 0, None
    for k in (700, 700, 1500, 3000, 6000, 12000, 24000, 22100):      # the capacity doubles several times over
        st.push(np.concatenate([x[at:at + k], x[at:at + k // 2]]), [0, k, k + k // 2])
        at += k
        if at == 2900:
            early = st.read(0).copy()
    assert at == 70000 and early.shape[0] == 8
    got, _, _ = _check_lane(eng, st, 0, x)
    assert np.array_equal(got[:8], early) and np.array_equal(st.read(0, 0, 8), early)
    st.close()


# ---- the grid-stride cap ------------------------------------------------------------------------------------------------
def _grid_cap():
    text = open(os.path.join(ROOT, "soundsym_amd", "csrc", "stream.hip")).read()
    factors = [int(v) for v in re.findall(r"num_cus \* (\d+)", text)]
    assert len(factors) == 1
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * factors[0]


@pytest.mark.parametrize("extra", [0, 333])
def test_more_work_than_the_grid(eng, extra):
    cap = _grid_cap()
    frames = cap + extra                        # exactly the cap, and past it (the power chunks come on top)
    n = 1024 + 256 * (frames - 1)
    x = _signal(n + 100, seed=extra)
    st = eng.stream(1, 44100.0)
    assert int(st.push(x[:n])[0]) == frames
    _check_lane(eng, st, 0, x[:n])
    st.push(x[n:])
    _check_lane(eng, st, 0, x)
    st.close()


# ---- coefficient counts and rates --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000.0, 44100.0])
@pytest.mark.parametrize("nc", [1, 12, 13, 40, 64])
def test_coefficient_counts_and_rates(eng, oracle, nc, rate):
    x = _signal(6000, rate, seed=nc)
    f_hi = 3800.0 if rate == 8000.0 else 8000.0
    st = eng.stream(2, rate, nc, 100.0, f_hi)
    at = 0
    for k in (1500, 1030, 0, 3470):
        st.push(np.concatenate([x[at:at + k], x[at:at + k]]), [0, k, 2 * k])
        at += k
        got, _, _ = _check_lane(eng, st, 1, x[:at], rate, nc, 100.0, f_hi)
    want = oracle.mfcc(x, rate, nc, f_lo=100.0, f_hi=f_hi)
    assert np.all(np.abs(got - want) <= TOL * (1.0 + np.abs(want)))
    st.close()


# ---- the device path -----------------------------------------------------------------------------------------------------
def test_resident_frames_feed_the_other_calls(eng):
    y, rate = read_wav(os.path.join(AUDIO, "Section_7_1.wav"))
    y = np.ascontiguousarray(y, dtype=np.float64)[:120000]
    st = eng.stream(1, float(rate))
    for at in range(0, y.size, 4096):
        st.push(y[at:at + 4096])
    host = st.read(0)
    dev = st.frames_device(0)
    n = host.shape[0]
    assert dev.shape == (n, 12) and dev.data_ptr() and st.samples_device(0).shape == (y.size, 1)
    gmm = eng.gmm_train(host, 12, init_rows(n, 8, 0), 0.1, 5)
    assert np.array_equal(eng.partition(gmm, dev), eng.partition(gmm, host))
    lh, ph = eng.gmm_predict(gmm, host, want_post=True)
    ld, pd = eng.gmm_predict(gmm, dev, want_post=True)
    assert np.array_equal(ld, lh) and np.array_equal(pd, ph)
    off = np.array([0, 5, 5, 40, n // 2, n], dtype=np.uint64)
    dh, mh = eng.sequence_distances(host, off, 12, want_mean=True)
    dd, md = eng.sequence_distances(dev, off, 12, want_mean=True)
    assert np.array_equal(dd, dh, equal_nan=True) and np.array_equal(md, mh, equal_nan=True)
    d = eng.dictionary(_signal(40 * 12 * 10, seed=3).reshape(-1), np.arange(0, 41 * 10, 10, dtype=np.uint64), 12)
    qoff = np.array([0, 5, 40, n // 2, n], dtype=np.uint64)
    qh, qd = eng.queries(host, qoff, 12), eng.queries(dev, qoff, 12)
    ih, vh = eng.match(d, qh)
    idv, vd = eng.match(d, qd)
    assert np.array_equal(idv, ih) and np.array_equal(vd, vh, equal_nan=True)
    for h in (qh, qd, d, gmm, st):
        h.close()


# ---- recordings ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Section_7_1.wav", "sample.wav"])
def test_recordings_in_blocks(eng, name):
    path = os.path.join(AUDIO, name)
    whole = Sound.from_path(path, engine=eng)
    y = whole.samples()
    s = Sound.from_samples(np.zeros(0), whole.sample_rate(), None, engine=eng)
    for at in range(0, y.size, 4096):
        s.push_samples(y[at:at + 4096], engine=eng)
    assert np.array_equal(s.samples(), y) and s.num_frames() == whole.num_frames()
    assert np.array_equal(s.mfccs(), whole.mfccs())
    assert s.max_power() == whole.max_power() and np.array_equal(s.mean_mfccs(), whole.mean_mfccs())
    st, lane = s.stream()
    mp, mn = st.descriptors()
    assert mp[lane] == eng.sound_descriptors(y, [0, y.size])[0][0]
    assert np.array_equal(mn[lane], eng.mfcc_batch(y, [0, y.size], whole.sample_rate(), want_mean=True)[2][0])


# ---- the Python interface -------------------------------------------------------------------------------------------------
def test_push_samples_and_push_sounds(eng):
    x = _signal(30000, seed=11)
    s = Sound.from_samples(x[:9000], 44100.0, None, engine=eng)
    s.preload_pitch_confidence(eng)
    conf = s.pitch_confidence()
    early = s.samples()
    s.push_samples(x[9000:9100], engine=eng)
    s.push_samples(x[9100:20000], engine=eng)
    assert s.pitch_confidence() == conf                                  # not refreshed by a push (src/sound.rs:170-179)
    assert early.size == 9000 and np.array_equal(early, x[:9000])
    assert np.array_equal(s.samples(), x[:20000]) and np.array_equal(s.mfcc_arrays(), eng.mfcc(x[:20000], 44100.0))
    # a sound whose features lag behind its samples: the push analyses the rest (the reference's tail)
    lag = Sound(x[:9000], 44100.0, eng.mfcc(x[:9000], 44100.0)[:10])
    lag.push_samples(x[9000:9001], engine=eng)
    assert np.array_equal(lag.mfcc_arrays(), eng.mfcc(x[:9001], 44100.0))
    # push_sounds: one device call for many sounds equals one push_samples each
    cuts = [(0, 3000), (3000, 3100), (5000, 12000), (100, 1300)]
    many = [Sound.from_samples(x[a:b], 44100.0, None, engine=eng) for a, b in cuts]
    each = [Sound.from_samples(x[a:b], 44100.0, None, engine=eng) for a, b in cuts]
    for rnd in range(3):
        chunks = [x[b + 900 * rnd:b + 900 * rnd + k] for (a, b), k in zip(cuts, (900, 0, 700, 100))]
        push_sounds(many, chunks, eng)
        for t, c in zip(each, chunks):
            t.push_samples(c, engine=eng)
        for m, t in zip(many, each):
            assert np.array_equal(m.samples(), t.samples()) and np.array_equal(m.mfccs(), t.mfccs())
            assert np.array_equal(m.mfccs(), eng.mfcc(m.samples(), 44100.0).reshape(-1))
    assert many[0].stream()[0] is many[3].stream()[0] and many[3].stream()[1] == 3


def test_reset_and_repeatability(eng):
    x = _signal(12000, seed=21)

    def run(st):
        for at in range(0, x.size, 1700):
            a, b = x[at:at + 1700], x[at:at + 500]
            st.push(np.concatenate([a, b]), [0, a.size, a.size + b.size])
        return st.read(0).copy(), st.read(1).copy(), st.descriptors()
    st = eng.stream(2, 44100.0)
    first = run(st)
    st.reset(0)
    ns, nf = st.counts()
    assert int(ns[0]) == int(nf[0]) == 0 and int(nf[1]) == first[1].shape[0]
    mp, mn = st.descriptors()
    assert mp[0] == 0.0 and np.all(np.isnan(mn[0])) and mp[1] == first[2][0][1] and np.array_equal(mn[1], first[2][1][1])
    st.reset(1)
    again = run(st)                                   # a reset lane behaves as a fresh one
    fresh = eng.stream(2, 44100.0)
    other = run(fresh)                                # ... and a second run gives the same bits
    for a, b, c in zip(first, again, other):
        if isinstance(a, tuple):
            assert all(np.array_equal(u, v) and np.array_equal(u, w) for u, v, w in zip(a, b, c))
        else:
            assert np.array_equal(a, b) and np.array_equal(a, c)
    st.close()
    fresh.close()


# ---- bad arguments ---------------------------------------------------------------------------------------------------------
def test_bad_arguments(eng):
    L, ctx = nat.lib(), eng.ctx
    out = ctypes.c_void_p()
    bad_create = [(0, 44100.0, 12, 100.0, 8000.0), (1, 44100.0, 0, 100.0, 8000.0), (1, 44100.0, 65, 100.0, 8000.0),
                  (1, 0.0, 12, 100.0, 8000.0), (1, -1.0, 12, 100.0, 8000.0), (1, float("inf"), 12, 100.0, 8000.0),
                  (1, float("nan"), 12, 100.0, 8000.0), (1, 44100.0, 12, -1.0, 8000.0), (1, 44100.0, 12, 500.0, 400.0),
                  (1, 8000.0, 12, 4000.0, 8000.0)]
    for lanes, rate, nc, lo, hi in bad_create:
        assert L.ssym_stream_create(ctx, lanes, rate, nc, lo, hi, 0, ctypes.byref(out)) == nat.SSYM_E_INVALID
        assert not out.value and L.ssym_last_error(ctx)
    assert L.ssym_stream_create(ctx, 1, 44100.0, 12, 100.0, 8000.0, 0, None) == nat.SSYM_E_INVALID
    assert L.ssym_stream_create(None, 1, 44100.0, 12, 100.0, 8000.0, 0, ctypes.byref(out)) == nat.SSYM_E_INVALID

    st = eng.stream(3, 44100.0)
    x = _signal(5000, seed=2)
    st.push(np.concatenate([x, x[:2000]]), [0, 5000, 5000, 7000])
    state = lambda: (st.counts(), st.descriptors(), st.read(0))
    before = state()
    u64 = lambda *v: np.array(v, dtype=np.uint64)
    buf = np.zeros(64 * 12)
    cases = [
        L.ssym_stream_push(ctx, st.ptr, x.ctypes.data, None, 0, None, None),                       # NULL offsets
        L.ssym_stream_push(ctx, st.ptr, None, u64(0, 10, 20, 30).ctypes.data, 0, None, None),      # NULL samples
        L.ssym_stream_push(ctx, st.ptr, x.ctypes.data, u64(0, 10, 5, 30).ctypes.data, 0, None, None),   # decreasing
        L.ssym_stream_push(ctx, None, x.ctypes.data, u64(0, 1, 2, 3).ctypes.data, 0, None, None),   # NULL stream
        L.ssym_stream_push(None, st.ptr, x.ctypes.data, u64(0, 1, 2, 3).ctypes.data, 0, None, None),
        L.ssym_stream_seed(ctx, st.ptr, 3, x.ctypes.data, 100, None, 0),                            # lane out of range
        L.ssym_stream_seed(ctx, st.ptr, 1, None, 100, None, 0),                                     # NULL samples
        L.ssym_stream_seed(ctx, st.ptr, 0, x.ctypes.data, 100, None, 0),                            # lane not empty
        L.ssym_stream_read(ctx, st.ptr, 3, 0, 1, 0, buf.ctypes.data),
        L.ssym_stream_read(ctx, st.ptr, 0, 0, 17, 0, buf.ctypes.data),                              # lane 0 holds 16
        L.ssym_stream_read(ctx, st.ptr, 0, 16, 1, 0, buf.ctypes.data),
        L.ssym_stream_read(ctx, st.ptr, 0, 17, 0, 0, buf.ctypes.data),
        L.ssym_stream_read(ctx, st.ptr, 0, 0, 4, 0, None),
        L.ssym_stream_read(ctx, st.ptr, 1, 0, 1, 0, buf.ctypes.data),                               # lane 1 holds none
        L.ssym_stream_reset(ctx, st.ptr, 3),
        L.ssym_stream_reset(ctx, None, 0),
        L.ssym_stream_descriptors(ctx, None, buf.ctypes.data, None),
        L.ssym_stream_counts(None, buf.ctypes.data, None),
        L.ssym_stream_frames_device(st.ptr, 3, ctypes.byref(out), ctypes.byref(ctypes.c_uint64())),
        L.ssym_stream_frames_device(st.ptr, 0, None, ctypes.byref(ctypes.c_uint64())),
        L.ssym_stream_samples_device(st.ptr, 0, ctypes.byref(out), None),
    ]
    assert cases == [nat.SSYM_E_INVALID] * len(cases)
    other = Engine(metric="refcos", dtype="f64")              # a stream belongs to its context
    assert L.ssym_stream_push(other.ctx, st.ptr, x.ctypes.data, u64(0, 1, 2, 3).ctypes.data, 0, None, None) == nat.SSYM_E_INVALID
    other.close()
    with pytest.raises(ValueError):
        st.push(x, [0, 10, 20])
    with pytest.raises(ValueError):
        st.read(5)
    after = state()
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before[1], after[1]))
    assert np.array_equal(before[2], after[2])
    assert np.array_equal(st.read(0, 16, 0), np.zeros((0, 12)))            # an empty read at the end is fine
    st.close()


# ---- non-finite samples ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_samples(eng, bad):
    clean = _signal(8000, seed=4)
    x = clean.copy()
    x[3333] = bad
    st = eng.stream(1, 44100.0)
    at = 0
    for k in (3000, 1000, 4000):          # the middle chunk carries the value
        st.push(x[at:at + k])
        at += k
        got, power, _ = _check_lane(eng, st, 0, x[:at])
    # frames 10..13 read sample 3333; what they hold is whatever Engine.mfcc gives (checked above), the others are clean
    ref = eng.mfcc(clean, 44100.0)
    touched = [t for t in range(ref.shape[0]) if 256 * t <= 3333 < 256 * t + 1024]
    assert touched == [10, 11, 12, 13]
    rest = [t for t in range(ref.shape[0]) if t not in touched]
    assert np.array_equal(got[rest], ref[rest]) and not np.array_equal(got[touched], ref[touched], equal_nan=True)
    assert np.isfinite(power) == (bad != bad)      # a NaN window is skipped by the maximum, an infinite one wins it
    st.close()
