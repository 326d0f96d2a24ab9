"""The partitioner on the GPU (ssym_standardize / ssym_gmm_* / ssym_vote_segments / ssym_partition) against the numpy
restatement of DESIGN.md 5.8 (tests/partition_ref.py).

Parity with the REFERENCE is unpinned (its arithmetic is in un-vendored crates); what is checked is GPU == restatement.
Tolerances: standardised data 1e-12, mixture parameters and log-likelihood rtol 1e-9, posteriors 1e-9.  Votes: the
frequency expert works on integer counts and a prescribed f64 formula, so its votes must be exact; the entropy expert's
vote may differ only in windows whose two best entropy scores the restatement puts within 1e-9 of each other.
"""
import ctypes
import os

import numpy as np
import pytest

import partition_ref as ref
import soundsym_amd._native as nat
from soundsym_amd import Engine, Partitioner, SoundDictionary, SoundSequence, SsymError
from soundsym_amd.api import HOP, init_rows
from soundsym_amd.io import read_wav

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = os.path.join(HERE, "golden", "audio", "sample.wav")


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="refcos", dtype="f64")
    yield e
    e.close()


def _mixture(seed=1, K=26, d=12, n=20000):
    rng = np.random.default_rng(seed)
    centers = rng.normal(scale=6.0, size=(K, d))
    lab = rng.integers(0, K, n)
    return centers[lab] + rng.normal(size=(n, d)) * rng.uniform(0.5, 1.5, size=(K, 1))[lab]


@pytest.fixture(scope="module")
def sample_mfcc(eng):
    x, rate = read_wav(SAMPLE)
    return eng.mfcc(x, rate, 12)


def _data(name, eng, sample_mfcc):
    return _mixture() if name == "mixture" else sample_mfcc


def _close(got, want, tol):
    return np.all(np.abs(got - want) <= tol * (1.0 + np.abs(want)))


@pytest.mark.parametrize("name", ["mixture", "sample"])
def test_standardize_matches_restatement(eng, sample_mfcc, name):
    x = _data(name, eng, sample_mfcc).copy()
    x[:, 3] = 5.0                                     # a constant column maps to 0
    got, want = eng.standardize(x, 12), ref.standardize(x)
    assert _close(got, want, 1e-12)
    assert np.all(got[:, 3] == 0.0)


@pytest.mark.parametrize("name,iters", [("mixture", 5), ("mixture", 1000), ("sample", 5), ("sample", 40)])
def test_gmm_matches_restatement(eng, sample_mfcc, name, iters):
    x = _data(name, eng, sample_mfcc)
    rows = init_rows(x.shape[0], 26, seed=3)
    g = eng.gmm_train(x, 12, rows, 0.1, iters)
    want = ref.gmm_train(ref.standardize(x), rows, 0.1, iters)
    assert g.iters == want["iters"]
    assert np.allclose(g.weights, want["weights"], rtol=1e-9, atol=1e-13)
    assert np.allclose(g.means, want["means"], rtol=1e-9, atol=1e-11)
    assert np.allclose(g.covs, want["covs"], rtol=1e-9, atol=1e-11)
    assert np.isclose(g.log_lik, want["log_lik"], rtol=1e-9, atol=0)
    g.close()


@pytest.mark.parametrize("name", ["mixture", "sample"])
def test_predict_matches_restatement(eng, sample_mfcc, name):
    x = _data(name, eng, sample_mfcc)
    g = eng.gmm_train(x, 12, init_rows(x.shape[0], 26, seed=4), 0.1, 5)
    let, post = eng.gmm_predict(g, x, want_post=True)
    want_post, _ = ref.posteriors(ref.standardize(x), g.weights, g.means, g.covs)
    assert np.all(np.abs(post - want_post) <= 1e-9)
    want = ref.letters(want_post)
    srt = np.sort(want_post, axis=1)
    gap = srt[:, -1] - srt[:, -2]
    excused = (gap > 0) & (gap < 1e-9)                # exact ties resolve to the first maximum on both sides
    assert excused.sum() < 1e-3 * len(x)
    assert np.array_equal(let[~excused], want[~excused])
    # the letters alone (no posterior matrix) are the same
    assert np.array_equal(eng.gmm_predict(g, x), let)
    g.close()


def _planted(A, n, seed, nwords=20):
    rng = np.random.default_rng(seed)
    lex = [rng.integers(0, A, rng.integers(3, 7)) for _ in range(nwords)]
    out, bounds, pos = [], [], 0
    while pos < n:
        w = lex[rng.integers(0, nwords)]
        out.extend(w.tolist())
        pos += len(w)
        bounds.append(pos)
    return np.array(out[:n], dtype=np.uint8), [b for b in bounds if b < n]


def _check_votes(eng, s, A, d, t):
    s = np.asarray(s, dtype=np.uint8)
    N = s.size
    seg, votes = eng.vote_segments(s, A, d, t, want_votes=True)
    assert seg.sum() == N and np.all(seg > 0)
    vf, vh, margins, _ = ref.vote_details(s, d)
    assert np.array_equal(votes[0], vf), "frequency-expert votes differ"
    # entropy expert: a window with a near-tie may put its vote on any of its d - 1 positions; an exact tie (margin 0)
    # resolves to the first maximum on both sides and is not excused
    slack = np.zeros(N + 1, dtype=np.int64)
    for w in np.nonzero((margins > 0) & (margins < 1e-9))[0]:
        slack[w + 1:w + d] += 1
    assert np.all(np.abs(votes[1].astype(np.int64) - vh) <= slack)
    total = votes[0].astype(np.int64) + votes[1]
    assert total.sum() == 2 * max(N - d + 1, 0)
    got_b = set(np.cumsum(seg)[:-1].tolist())
    want_b = set(ref.boundaries(vf + vh, t))
    affected = np.zeros(N + 2, dtype=bool)
    affected[:N + 1] = slack > 0
    for p in range(1, N):
        if not (affected[p - 1] or affected[p] or affected[p + 1]):
            assert (p in got_b) == (p in want_b), p
    if not slack.any():
        assert seg.tolist() == ref.segments(s, d, t)
    return seg


@pytest.mark.parametrize("A,d", [(2, 2), (2, 5), (3, 3), (5, 4), (8, 6), (26, 5), (26, 7), (13, 2)])
@pytest.mark.parametrize("N", [0, 1, "d-1", "d", 1000])
def test_votes_random(eng, A, d, N):
    N = {"d-1": d - 1, "d": d}.get(N, N)
    rng = np.random.default_rng(A * 1000 + d * 10 + N)
    s = rng.integers(0, A, N)
    for t in sorted({1, d - 1, 2 * (d - 1)}):
        seg = _check_votes(eng, s, A, d, t)
        if N < d:
            assert seg.tolist() == ([N] if N else [])


@pytest.mark.parametrize("A,d,t,floor", [(26, 5, 4, 0.99), (8, 4, 3, 0.8), (26, 7, 6, 0.95), (4, 4, 3, 0.55)])
def test_votes_planted_lexicon(eng, A, d, t, floor):
    s, bounds = _planted(A, 20000, A * 10 + d)
    seg = _check_votes(eng, s, A, d, t)
    found = set(np.cumsum(seg)[:-1].tolist())
    assert len(found & set(bounds)) / len(bounds) >= floor


@pytest.mark.parametrize("A,d,t", [(26, 5, 4), (2, 7, 12)])
def test_votes_million(eng, A, d, t):
    s = np.random.default_rng(d).integers(0, A, 10 ** 6)
    _check_votes(eng, s, A, d, t)


def test_partitioner_end_to_end(eng):
    p = Partitioner.from_path(SAMPLE, engine=eng)
    p.train(seed=0)
    splits = p.partition()
    frames = p.sound.num_frames()
    assert len(splits) > 0                                    # the reference's own assertion (src/lib.rs:220-233)
    assert all(s % HOP == 0 and s > 0 for s in splits)
    assert sum(splits) == frames * HOP
    m = p.model
    want = ref.partition(p.sound.mfccs().reshape(-1, 12), m.weights, m.means, m.covs, 5, 4)
    assert splits == [f * HOP for f in want]
    # predict + vote in one call == the two steps
    let = eng.gmm_predict(m, p.sound.mfccs().reshape(-1, 12))
    assert (eng.vote_segments(let, 26, 5, 4) * HOP).tolist() == splits
    # the reconstruction flow: dictionary from the source's segments, the partitioned target matched against it
    d = SoundDictionary.from_segments(p.sound, splits, engine=eng)
    target = Partitioner.from_path(os.path.join(HERE, "golden", "audio", "Section_7_1.wav"), engine=eng).sound
    tsplits = p.partition_other(target)
    assert sum(tsplits) == target.num_frames() * HOP
    td = SoundDictionary.from_segments(target, tsplits, engine=eng)
    out = SoundSequence.new(td.sounds).clone_from_dictionary(d)
    assert len(out.sounds()) == len(tsplits)


def test_two_runs_same_bits(eng, sample_mfcc):
    x = sample_mfcc
    rows = init_rows(x.shape[0], 26, seed=7)
    a, b = eng.gmm_train(x, 12, rows, 0.1, 20), eng.gmm_train(x, 12, rows, 0.1, 20)
    assert a.iters == b.iters and a.log_lik == b.log_lik
    for u, v in ((a.weights, b.weights), (a.means, b.means), (a.covs, b.covs)):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
    pa, pb = eng.gmm_predict(a, x, want_post=True)[1], eng.gmm_predict(a, x, want_post=True)[1]
    assert np.array_equal(pa.view(np.uint64), pb.view(np.uint64))
    s = np.random.default_rng(0).integers(0, 26, 50000)
    va, vb = eng.vote_segments(s, 26, 5, 4, True), eng.vote_segments(s, 26, 5, 4, True)
    assert np.array_equal(va[0], vb[0]) and np.array_equal(va[1], vb[1])
    a.close()
    b.close()


def test_error_paths(eng):
    L = nat.lib()
    ctx = eng.ctx
    x = np.random.default_rng(0).normal(size=(40, 12))
    rows = np.arange(26, dtype=np.uint64)
    out = ctypes.c_void_p()
    seg = np.zeros(64, dtype=np.uint64)
    m = ctypes.c_uint64()
    s = np.zeros(64, dtype=np.uint8)

    def expect(rc, text):
        assert rc == nat.SSYM_E_INVALID
        assert text in L.ssym_last_error(ctx).decode()

    expect(L.ssym_gmm_train(ctx, x.ctypes.data, 20, 12, 26, rows.ctypes.data, 0.1, 5, 0, ctypes.byref(out)),
           "n_frames < n_components")
    expect(L.ssym_gmm_train(ctx, None, 40, 12, 26, rows.ctypes.data, 0.1, 5, 0, ctypes.byref(out)), "NULL")
    expect(L.ssym_gmm_train(ctx, x.ctypes.data, 40, 65, 26, rows.ctypes.data, 0.1, 5, 0, ctypes.byref(out)),
           "dim")
    bad = rows.copy()
    bad[3] = 40
    expect(L.ssym_gmm_train(ctx, x.ctypes.data, 40, 12, 26, bad.ctypes.data, 0.1, 5, 0, ctypes.byref(out)),
           "init_rows")
    expect(L.ssym_vote_segments(ctx, s.ctypes.data, 64, 4, 1, 1, 0, None, seg.ctypes.data, ctypes.byref(m)),
           "depth")
    expect(L.ssym_vote_segments(ctx, s.ctypes.data, 64, 1, 3, 1, 0, None, seg.ctypes.data, ctypes.byref(m)),
           "alphabet")
    expect(L.ssym_vote_segments(ctx, s.ctypes.data, 64, 256, 8, 1, 0, None, seg.ctypes.data, ctypes.byref(m)),
           "2^63")
    expect(L.ssym_vote_segments(ctx, s.ctypes.data, 64, 4, 3, 1, 0, None, None, ctypes.byref(m)), "NULL")
    s[5] = 9
    expect(L.ssym_vote_segments(ctx, s.ctypes.data, 64, 4, 3, 1, 0, None, seg.ctypes.data, ctypes.byref(m)),
           ">= alphabet")
    expect(L.ssym_partition(ctx, None, x.ctypes.data, 40, 5, 4, 0, seg.ctypes.data, ctypes.byref(m)), "NULL model")
    expect(L.ssym_gmm_predict(ctx, None, x.ctypes.data, 40, 0, None, None), "NULL model")
    with pytest.raises(SsymError):
        eng.vote_segments(np.zeros(10, dtype=np.uint8), 2, 1, 1)
    # empty input: no segments, no error
    assert eng.vote_segments(np.zeros(0, dtype=np.uint8), 4, 3, 1).size == 0
    g = eng.gmm_train(x, 12, rows, 0.1, 2)
    assert eng.partition(g, np.zeros((0, 12))).size == 0
    assert eng.partition(g, x[:3]).tolist() == [3]
    assert eng.gmm_predict(g, np.zeros((0, 12))).size == 0
    g.close()
