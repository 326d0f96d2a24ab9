"""Batched MFCC analysis and SoundSequence distances on the GPU (ssym_mfcc_batch / ssym_sequence_distances, DESIGN.md
5.10).

The batch must give every sound's frames bit for bit as ssym_mfcc does for that sound alone (and stay within the MFCC
tolerance of the oracle).  The distances are held to a host restatement written out here: the means by the sequential
fold of Sound.mean_mfccs(), the oracle's cosine_sim (the reference's, src/sound.rs:22-33), the reference's clamp
(:63-67, a similarity below -1 also maps to 1) and math.acos(x) * FRAC_1_PI.  Similarities are bit-equal, distances
within 1e-15, NaN in the same places.
"""
import ctypes
import math
import os

import numpy as np
import pytest

import soundsym_amd._native as nat
from soundsym_amd import (Engine, Partitioner, Sound, SoundDictionary, SoundSequence, SsymError, analyze_mfccs,
                          cosine_sim_angular)
from soundsym_amd.io import audacity_labels_to_timestamps, read_wav, write_wav32

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
SECTION = os.path.join(GOLD, "audio", "Section_7_1.wav")
SAMPLE = os.path.join(GOLD, "audio", "sample.wav")
FRAC_1_PI = 0.3183098861837907
TOL = 1e-12
LENGTHS = [0, 1, 255, 1023, 1024, 1025, 5000, 44100]


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="refcos", dtype="f64")
    yield e
    e.close()


def _batch(parts):
    parts = [np.asarray(p, dtype=np.float64).reshape(-1) for p in parts]
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return (np.concatenate(parts) if parts else np.zeros(0)), off


def _signal(n, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    return 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t) + 0.05 * rng.normal(size=n)


def _mean_fold(frames, dim):
    """Sound.mean_mfccs(): acc = acc + row from +0.0 in frame order, then / T (NaN without frames)."""
    m = np.asarray(frames, dtype=np.float64).reshape(-1, dim)
    acc = np.zeros(dim)
    for row in m:
        acc = acc + row
    return acc / m.shape[0] if m.shape[0] else acc * np.nan


def _restate(means, oracle):
    sims, dists = [], []
    for a, b in zip(means[:-1], means[1:]):
        s = oracle.cosine_sim(a, b)
        c = 1.0 if s > 1.0 else (1.0 if s < -1.0 else s)
        sims.append(c)
        dists.append(math.acos(c) * FRAC_1_PI)
    return np.array(sims), np.array(dists)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    k = ~np.isnan(a)
    return np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))


def _check_distances(dist, sim, means, oracle):
    want_sim, want_dist = _restate(means, oracle)
    assert _same_bits(sim, want_sim)
    assert np.array_equal(np.isnan(dist), np.isnan(want_dist))
    k = ~np.isnan(want_dist)
    assert np.all(np.abs(dist[k] - want_dist[k]) <= 1e-15)


# 1. + 3. batch == single calls, == oracle within tolerance; means bit-identical to Sound.mean_mfccs() ----------------
@pytest.mark.parametrize("rate,nc", [(44100.0, 12), (16000.0, 13), (8000.0, 20)])
@pytest.mark.parametrize("pad_tail", [False, True])
def test_batch_equals_single_calls(eng, oracle, rate, nc, pad_tail):
    lengths = list(LENGTHS)
    np.random.default_rng(int(rate) + nc).shuffle(lengths)
    parts = [_signal(n, rate, i) for i, n in enumerate(lengths)]
    x, off = _batch(parts)
    feats, fo, mean = eng.mfcc_batch(x, off, rate, nc, pad_tail=pad_tail, want_mean=True)
    counts = [Engine.mfcc_num_frames(n, pad_tail) for n in lengths]
    assert fo.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert feats.shape == (sum(counts), nc)
    for i, p in enumerate(parts):
        got = feats[int(fo[i]):int(fo[i + 1])]
        single = eng.mfcc(p, rate, nc, pad_tail=pad_tail)
        assert np.array_equal(got, single), f"sound {i} ({lengths[i]} samples)"
        if got.shape[0]:
            want = oracle.mfcc(p, rate, nc, pad_tail=pad_tail)
            assert np.all(np.abs(got - want) <= TOL * (1.0 + np.abs(want)))
        s = Sound(p, rate, single.reshape(-1), None, nc)
        assert _same_bits(mean[i], s.mean_mfccs())
        assert np.all(np.isnan(mean[i])) == (counts[i] == 0)
    # the api form: flat arrays, each Sound.from_samples(.., None).mfccs() bit for bit (full windows)
    if not pad_tail:
        flat = analyze_mfccs(parts, rate, nc, engine=eng)
        for p, f in zip(parts, flat):
            assert np.array_equal(f, Sound.from_samples(p, rate, None, ncoeffs=nc, engine=eng).mfccs())


# 2. a window reads zeros past its own sound's end, never the next sound ----------------------------------------------
def test_pad_tail_isolation(eng):
    rate = 44100.0
    loud = [1e3 * _signal(3000 + 77 * i, rate, 100 + i) for i in range(4)]
    short = [_signal(n, rate, 200 + n) for n in (300, 700, 1500)]
    parts = [loud[0], short[0], loud[1], short[1], loud[2], short[2], loud[3]]
    x, off = _batch(parts)
    for pad_tail in (True, False):
        feats, fo = eng.mfcc_batch(x, off, rate, 12, pad_tail=pad_tail)
        for i, p in enumerate(parts):
            assert np.array_equal(feats[int(fo[i]):int(fo[i + 1])], eng.mfcc(p, rate, 12, pad_tail=pad_tail))
    # the short sounds do hold padded frames, whose tails would see the loud neighbours if the reads leaked
    assert [Engine.mfcc_num_frames(p.size, True) for p in short] == [1, 2, 5]


# 4. distances against the restatement, every branch of the clamp -----------------------------------------------------
def test_distances_crafted_branches(eng, oracle):
    m = np.array([0.1, 0.4, 0.2, 0.8, 0., 0., 0., 0., 0., 0., 0., 0.])       # the reference's test_angular_distance
    a = np.full(12, 0.1)                                                      # sum of squares 0.12: sim(a, -a) < -1
    x = _signal(44100, 44100.0, 5)
    real = [eng.mfcc(x[k * 8000:k * 8000 + 4000 + 512 * k], 44100.0, 12) for k in range(4)]
    blocks = [m, m, a, -a, np.zeros(12), np.zeros(0), real[0], real[1], real[2], real[3]]
    feats, off = _batch(blocks)
    off //= np.uint64(12)
    dist, mean, sim = eng.sequence_distances(feats, off, 12, want_mean=True, want_sim=True)
    means = [_mean_fold(b, 12) for b in blocks]
    assert all(_same_bits(mean[i], means[i]) for i in range(len(blocks)))
    assert oracle.cosine_sim(m, m) > 1.0 and oracle.cosine_sim(a, -a) < -1.0
    assert sim[0] == 1.0 and dist[0] == 0.0                                  # sim > 1 -> 1 -> exactly 0
    assert sim[2] == 1.0 and dist[2] == 0.0                                  # sim < -1 -> 1 (not -1) -> 0
    assert np.isnan(dist[3]) and np.isnan(dist[4]) and np.isnan(dist[5])     # a zero mean and a frameless block
    assert np.all(np.isfinite(dist[6:])) and np.all((dist[6:] >= 0.0) & (dist[6:] <= 1.0))
    _check_distances(dist, sim, means, oracle)
    assert cosine_sim_angular(m, m, engine=eng) == 0.0
    assert cosine_sim_angular(a, -a, engine=eng) == 0.0


@pytest.mark.parametrize("dim", [1, 7, 8, 13, 20, 64])
def test_distances_every_dim(eng, oracle, dim):
    # rulinalg's dot: whole blocks of eight plus the tail, at every shape of the split
    rng = np.random.default_rng(dim)
    blocks = [rng.normal(size=(int(t), dim)) * (0.02 if k % 3 else 3.0) for k, t in enumerate(rng.integers(1, 9, 12))]
    feats, off = _batch(blocks)
    off //= np.uint64(dim)
    dist, mean, sim = eng.sequence_distances(feats, off, dim, want_mean=True, want_sim=True)
    means = [_mean_fold(b, dim) for b in blocks]
    assert all(_same_bits(mean[i], means[i]) for i in range(len(blocks)))
    _check_distances(dist, sim, means, oracle)


# 5. recordings: from_timestamps in one batch; its distances -----------------------------------------------------------
def test_from_timestamps_recording(eng, oracle):
    x, rate = read_wav(SECTION)
    ts = audacity_labels_to_timestamps(os.path.join(GOLD, "vowel.txt"))
    seq = SoundSequence.from_timestamps(Sound(x, rate, None), ts, engine=eng)
    assert len(seq.sounds()) == 55
    total = 0
    for s, (_, _, label) in zip(seq.sounds(), ts):
        want = Sound.from_samples(s.samples(), rate, None, label, engine=eng)
        assert s.name == label and np.array_equal(s.mfccs(), want.mfccs())
        total += s.num_frames()
    assert total == 1537
    dist = seq.distances(engine=eng)
    assert dist.shape == (54,)
    means = [s.mean_mfccs() for s in seq.sounds()]
    _, want = _restate(means, oracle)
    assert np.array_equal(np.isnan(dist), np.isnan(want))
    k = ~np.isnan(want)
    assert np.all(np.abs(dist[k] - want[k]) <= 1e-15)


# 6. a clone_from_dictionary sequence: fitted sounds without features next to shared dictionary sounds -----------------
def test_clone_from_dictionary_distances(eng, oracle):
    src = Sound.from_path(SAMPLE, engine=eng)
    d = SoundDictionary.from_segments(src, [4096] * 40, engine=eng)       # every dictionary sound 4096 samples long
    y, rate = read_wav(SECTION)
    lengths = [4096, 3000, 4096, 6000, 5000, 4096, 4096, 2500, 9000, 4096]
    targets, pos = [], 20000
    for n in lengths:
        targets.append(Sound.from_samples(y[pos:pos + n], rate, None, engine=eng))
        pos += n + 1000
    seq = SoundSequence.new(targets).clone_from_dictionary(d)
    out = seq.sounds()
    shared = [s.has_mfccs() for s in out]
    assert shared == [n == 4096 for n in lengths] and any(shared) and not all(shared)
    feats = [s.mfccs() if s.has_mfccs() else eng.mfcc(s.samples(), s.sample_rate(), 12).reshape(-1) for s in out]
    means = [_mean_fold(f, 12) for f in feats]
    dist = seq.distances(engine=eng)
    _, want = _restate(means, oracle)
    assert np.array_equal(np.isnan(dist), np.isnan(want))
    k = ~np.isnan(want)
    assert np.all(np.abs(dist[k] - want[k]) <= 1e-15)
    assert not any(s.has_mfccs() for s, sh in zip(out, shared) if not sh)   # nothing stored on the fitted sounds
    assert np.array_equal(seq.distances(engine=eng), dist)


# 7. device path: features never leave the GPU -------------------------------------------------------------------------
def test_device_path_same_bits(eng):
    import torch
    rate = 16000.0
    parts = [_signal(n, rate, 300 + i) for i, n in enumerate([5000, 0, 1024, 20000, 700, 3333])]
    x, off = _batch(parts)
    feats, fo, mean = eng.mfcc_batch(x, off, rate, 13, want_mean=True)
    dist, hmean, sim = eng.sequence_distances(feats, fo, 13, want_mean=True, want_sim=True)
    out = torch.full((int(fo[-1]) * 13,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t, tfo, tmean = eng.mfcc_batch(x, off, rate, 13, want_mean=True, out=out)
    assert t is out and np.array_equal(tfo, fo) and _same_bits(tmean, mean)
    assert np.array_equal(out.cpu().numpy().reshape(-1, 13), feats)
    ddist, dmean, dsim = eng.sequence_distances(out, tfo, 13, want_mean=True, want_sim=True)
    assert _same_bits(ddist, dist) and _same_bits(dmean, hmean) and _same_bits(dsim, sim)
    assert _same_bits(hmean, mean)


# 8. SoundDictionary.from_path: one batch per sample rate, file order kept ---------------------------------------------
def test_from_path_two_rates(eng, tmp_path):
    y, _ = read_wav(SECTION)
    specs = [("a_first", 44100, 30000), ("b_low", 16000, 20000), ("c_short", 44100, 900), ("d_low", 16000, 7000),
             ("e_last", 44100, 12345)]
    pos = 0
    for name, rate, n in specs:
        write_wav32(str(tmp_path / f"{name}.wav"), 0.5 * y[pos:pos + n], rate)
        pos += n
    (tmp_path / "notes.txt").write_text("not a sound")
    d = SoundDictionary.from_path(str(tmp_path), engine=eng)
    assert [s.name for s in d.sounds] == [s[0] for s in specs]
    for s, (name, rate, n) in zip(d.sounds, specs):
        want = Sound.from_path(str(tmp_path / f"{name}.wav"), engine=eng)
        assert s.sample_rate() == want.sample_rate() == float(rate)
        assert np.array_equal(s.samples(), want.samples()) and np.array_equal(s.mfccs(), want.mfccs())


# 9. bad arguments: SSYM_E_INVALID, host outputs untouched --------------------------------------------------------------
def test_bad_arguments(eng):
    L = nat.lib()
    x = np.ones(4096)
    fo = np.full(4, 7, dtype=np.uint64)
    out = np.full(64 * 64, 7.0)
    mean = np.full(3 * 65, 7.0)

    def batch(off, rate=44100.0, nc=12):
        o = np.ascontiguousarray(off, dtype=np.uint64)
        return L.ssym_mfcc_batch(eng.ctx, x.ctypes.data, o.ctypes.data, o.size - 1, rate, nc, 100.0, 8000.0, 0,
                                 fo.ctypes.data, out.ctypes.data, mean.ctypes.data)
    good = [0, 2048, 2048, 4096]
    for rc in (batch([0, 2048, 1024, 4096]), batch(good, nc=0), batch(good, nc=65), batch(good, rate=0.0),
               batch(good, rate=-44100.0)):
        assert rc == nat.SSYM_E_INVALID
        assert L.ssym_last_error(eng.ctx)
    assert np.all(fo == 7) and np.all(out == 7.0) and np.all(mean == 7.0)
    feats = np.ones(5 * 12)
    sim, dist = np.full(4, 7.0), np.full(4, 7.0)

    def seqd(off, dim=12):
        o = np.ascontiguousarray(off, dtype=np.uint64)
        return L.ssym_sequence_distances(eng.ctx, feats.ctypes.data, o.ctypes.data, o.size - 1, dim, 0,
                                         mean.ctypes.data, sim.ctypes.data, dist.ctypes.data)
    for rc in (seqd([0, 2, 1, 5]), seqd([0, 1, 2, 5], dim=0), seqd([0, 1, 2, 5], dim=65)):
        assert rc == nat.SSYM_E_INVALID
    assert np.all(mean == 7.0) and np.all(sim == 7.0) and np.all(dist == 7.0)
    # through the engine: SsymError carrying the code
    for call in (lambda: eng.mfcc_batch(x, [0, 4096], 44100.0, 0), lambda: eng.mfcc_batch(x, [0, 4096], 0.0),
                 lambda: eng.mfcc_batch(x, [0, 4096], 44100.0, 65),
                 lambda: eng.sequence_distances(feats, [0, 2, 5], 0)):
        with pytest.raises(SsymError) as ei:
            call()
        assert ei.value.code == nat.SSYM_E_INVALID
    # the context still works after the failures
    assert np.array_equal(eng.mfcc_batch(x, [0, 4096], 44100.0)[0], eng.mfcc(x, 44100.0))


def test_partitioner_segments_distances(eng, oracle):
    # the reference's reconstruction flow: a dictionary of sample.wav's partitioner segments, a sequence cloned from it
    p = Partitioner.from_path(SAMPLE, engine=eng).threshold(3).depth(4)
    p.train(seed=0)
    d = SoundDictionary.from_segments(p.sound, p.partition(), engine=eng)
    y, rate = read_wav(SECTION)
    ts = audacity_labels_to_timestamps(os.path.join(GOLD, "vowel.txt"))[:20]
    seq = SoundSequence.from_timestamps(Sound(y, rate, None), ts, engine=eng).clone_from_dictionary(d)
    feats = [s.mfccs() if s.has_mfccs() else eng.mfcc(s.samples(), s.sample_rate(), 12).reshape(-1)
             for s in seq.sounds()]
    _, want = _restate([_mean_fold(f, 12) for f in feats], oracle)
    dist = seq.distances(engine=eng)
    assert np.array_equal(np.isnan(dist), np.isnan(want))
    k = ~np.isnan(want)
    assert np.all(np.abs(dist[k] - want[k]) <= 1e-15)
