"""The partitioner on the GPU at every model shape and input path the C ABI accepts, against the numpy restatement
(tests/partition_ref.py), with the tolerances of tests/test_gpu_partition.py.

The cases straddle the kernels' internal boundaries: the E-step's model in LDS or in global memory
(`model_fits_lds`), the E-step chunking capped by the slab budget (`chunking`), the lane splits of `colstats_kernel`,
frame counts around the 32-frame tile.  tests/test_partition_boundaries.py reads those constants from partition.hip
and checks, without a GPU, that the case lists below fall on both sides of every one of them.
"""
import ctypes
import os

import numpy as np
import pytest

import partition_ref as ref
import soundsym_amd._native as nat
from soundsym_amd import Partitioner, Sound, SsymError
from soundsym_amd.api import HOP, init_rows
from soundsym_amd.io import read_wav
from test_gpu_partition import _check_votes, _close, _mixture, eng  # noqa: F401  (eng: the module's engine fixture)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = os.path.join(HERE, "golden", "audio", "sample.wav")

# (K, d, n, max_iters) of the shape grid: standardised mixtures, eps 0.1
GMM_CASES = [
    (1, 1, 2000, 5), (2, 1, 2000, 5),
    (26, 13, 20000, 5),                               # model in LDS
    (26, 14, 20000, 5),                               # model in global memory
    (33, 12, 20000, 5), (34, 12, 20000, 5),           # the LDS edge at d = 12
    (8, 15, 5000, 3), (8, 23, 5000, 3),               # the covariance pass's lane splits (d = 16, 22 below)
    (64, 16, 20000, 4), (64, 21, 20000, 3),
    (64, 22, 20000, 3), (64, 32, 20000, 3),           # E-step blocks capped by the slab budget
    (64, 64, 20000, 3),                               # global memory and capped
    (26, 12, 26, 5), (26, 12, 31, 5), (26, 12, 32, 5), (26, 12, 33, 5), (26, 12, 65, 5),   # n around the tile
    (26, 12, 1 << 20, 1),
]
STD_DIMS = [1, 2, 3, 13, 16, 64]                      # standardiser at n = 20000
STD_NS = [1, 2, 33, 1 << 20]                          # standardiser at d = 12
VOTE_CASES = [(256, 7), (255, 7), (2, 62), (3, 39)]


def _same_stop(got_iters, want):
    """EM stops when |delta ll| < 1e-15, in effect exact equality: the iteration counts must match.  The one excused
    difference is a stop one step apart where the restatement's |delta ll| at that step is within 4 ulps of |ll|."""
    R = want["iters"]
    if got_iters == R:
        return
    assert abs(got_iters - R) == 1, (got_iters, R)
    t, j = want["totals"], min(got_iters, R)
    assert 1 <= j < len(t), (got_iters, R, len(t))
    assert abs(t[j] - t[j - 1]) <= 4 * np.spacing(abs(t[j])), (got_iters, R, t[j] - t[j - 1], t[j])


def _check_model(g, want, scale=1.0):
    assert np.allclose(g.weights, want["weights"], rtol=1e-9, atol=1e-13)
    assert np.allclose(g.means, want["means"], rtol=1e-9, atol=1e-11 * scale)
    assert np.allclose(g.covs, want["covs"], rtol=1e-9, atol=1e-11 * scale * scale)
    assert np.isclose(g.log_lik, want["log_lik"], rtol=1e-9, atol=0)


def _train_check(eng, x, K, eps, iters, standardize=True, seed=3, scale=1.0):
    n, d = x.shape
    rows = init_rows(n, K, seed=seed)
    g = eng.gmm_train(x, d, rows, eps, iters, standardize=standardize)
    z = ref.standardize(x) if standardize else x
    want = ref.gmm_train(z, rows, eps, iters)
    _same_stop(g.iters, want)
    if g.iters < want["iters"]:
        want = ref.gmm_train(z, rows, eps, g.iters)
    _check_model(g, want, scale)
    return g


def _predict_check(eng, g, x, standardize=True):
    let, post = eng.gmm_predict(g, x, standardize=standardize, want_post=True)
    z = ref.standardize(x) if standardize else x
    want_post, _ = ref.posteriors(z, g.weights, g.means, g.covs)
    assert np.all(np.abs(post - want_post) <= 1e-9)
    want = ref.letters(want_post)
    if g.k > 1:
        srt = np.sort(want_post, axis=1)
        gap = srt[:, -1] - srt[:, -2]
        excused = (gap > 0) & (gap < 1e-9)            # exact ties resolve to the first maximum on both sides
    else:
        excused = np.zeros(len(x), dtype=bool)
    assert excused.sum() < 1e-3 * len(x) + 1
    assert np.array_equal(let[~excused], want[~excused])
    assert np.array_equal(eng.gmm_predict(g, x, standardize=standardize), let)
    return let, post


@pytest.mark.parametrize("K,d,n,iters", GMM_CASES)
def test_gmm_shape_grid(eng, K, d, n, iters):
    x = _mixture(seed=K * 100 + d, K=K, d=d, n=n)
    g = _train_check(eng, x, K, 0.1, iters)
    _predict_check(eng, g, x)
    g.close()


def test_gmm_constant_column(eng):
    x = _mixture(seed=5)
    x[:, 3] = 5.0                                     # standardises to 0: that variance is eps alone
    g = _train_check(eng, x, 26, 0.1, 5)
    assert np.all(g.covs[:, 3, 3] > 0)
    _predict_check(eng, g, x)
    g.close()


def test_gmm_zero_iterations_is_the_start(eng):
    x = _mixture(seed=6, K=26, d=14)
    rows = init_rows(len(x), 26, seed=1)
    g = eng.gmm_train(x, 14, rows, 0.1, 0)
    z = ref.standardize(x)
    assert g.iters == 0 and g.log_lik == 0.0
    assert np.all(g.weights == 1.0 / 26)
    assert _close(g.means, z[rows.astype(np.int64)], 1e-12)            # the init rows, standardised
    _check_model(g, ref.gmm_train(z, rows, 0.1, 0))                      # covariances cov(z) + eps I
    _predict_check(eng, g, x)
    g.close()


def test_gmm_to_convergence(eng):
    # model in global memory, run until |delta ll| < 1e-15.  The restatement's delta ll falls from about 1e12 ulps of
    # ll to a few ulps in one step and is 0 two steps later (16 iterations), so the stop is not left to rounding noise
    # (a mixture whose ll creeps for hundreds of steps at 1-2 ulps would be)
    K, d = 26, 14
    x = _mixture(seed=27, K=K, d=d, n=8000)
    g = _train_check(eng, x, K, 0.1, 1000)
    assert g.iters < 1000
    g.close()


@pytest.mark.parametrize("d", STD_DIMS)
def test_standardize_dims(eng, d):
    x = _mixture(seed=d, K=7, d=d, n=20000) * 3.0 + 7.0
    assert _close(eng.standardize(x, d), ref.standardize(x), 1e-12)


@pytest.mark.parametrize("n", STD_NS)
def test_standardize_frames(eng, n):
    x = np.random.default_rng(n).normal(loc=2.0, scale=5.0, size=(n, 12))
    got = eng.standardize(x, 12)
    assert _close(got, ref.standardize(x), 1e-12)
    if n == 1:
        assert np.all(got == 0.0)


# unstandardised features: large column offsets and small scales (the M-step must not cancel against the means)
@pytest.mark.parametrize("kind", ["offset", "scaled"])
def test_unstandardised(eng, kind):
    x = _mixture(seed=8)
    x, eps, scale = (x + 1e3, 0.1, 1.0) if kind == "offset" else (x * 1e-3, 0.1e-6, 1e-3)
    g = _train_check(eng, x, 26, eps, 5, standardize=False, scale=scale)
    _predict_check(eng, g, x, standardize=False)
    seg = eng.partition(g, x, 5, 4, standardize=False)
    assert seg.tolist() == ref.partition(x, g.weights, g.means, g.covs, 5, 4, standardise=False)
    g.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8 if a.dtype == np.uint8 else np.uint64)


def test_device_pointers(eng):
    import torch
    L, ctx = nat.lib(), eng.ctx
    flags = nat.OUT_DEVICE | nat.GMM_STANDARDIZE
    n, d, K = 5003, 12, 26
    x = _mixture(seed=9, n=n)
    xd = torch.from_numpy(x).to("cuda")
    rows = init_rows(n, K, seed=2)
    # ssym_standardize
    zd = torch.empty_like(xd)
    torch.cuda.synchronize()
    nat.check(L.ssym_standardize(ctx, xd.data_ptr(), n, d, nat.OUT_DEVICE, zd.data_ptr()), ctx)
    assert np.array_equal(_bits(zd.cpu().numpy()), _bits(eng.standardize(x, d)))
    # ssym_gmm_train
    out = ctypes.c_void_p()
    nat.check(L.ssym_gmm_train(ctx, xd.data_ptr(), n, d, K, rows.ctypes.data, 0.1, 5, flags, ctypes.byref(out)), ctx)
    from soundsym_amd.engine import Gmm
    gd, gh = Gmm(eng, out.value, K, d), eng.gmm_train(x, d, rows, 0.1, 5)
    assert gd.iters == gh.iters and gd.log_lik == gh.log_lik
    for u, v in ((gd.weights, gh.weights), (gd.means, gh.means), (gd.covs, gh.covs)):
        assert np.array_equal(_bits(u), _bits(v))
    # ssym_gmm_predict: posteriors and letters in device memory
    post_d = torch.empty(n * K, dtype=torch.float64, device="cuda")
    let_d = torch.empty(n, dtype=torch.uint8, device="cuda")
    nat.check(L.ssym_gmm_predict(ctx, gh.ptr, xd.data_ptr(), n, flags, post_d.data_ptr(), let_d.data_ptr()), ctx)
    let, post = eng.gmm_predict(gh, x, want_post=True)
    assert np.array_equal(_bits(post_d.cpu().numpy().reshape(n, K)), _bits(post))
    assert np.array_equal(let_d.cpu().numpy(), let)
    # ssym_vote_segments on device symbols
    seg = np.zeros(n, dtype=np.uint64)
    votes = np.zeros((2, n + 1), dtype=np.uint32)
    m = ctypes.c_uint64()
    nat.check(L.ssym_vote_segments(ctx, let_d.data_ptr(), n, K, 5, 4, nat.OUT_DEVICE, votes.ctypes.data,
                                   seg.ctypes.data, ctypes.byref(m)), ctx)
    want_seg, want_votes = eng.vote_segments(let, K, 5, 4, want_votes=True)
    assert np.array_equal(seg[:m.value].astype(np.int64), want_seg)
    assert np.array_equal(votes, want_votes)
    # ssym_partition on device features
    seg[:] = 0
    nat.check(L.ssym_partition(ctx, gh.ptr, xd.data_ptr(), n, 5, 4, flags, seg.ctypes.data, ctypes.byref(m)), ctx)
    assert np.array_equal(seg[:m.value].astype(np.int64), eng.partition(gh, x, 5, 4))
    gd.close()
    gh.close()


def test_not_positive_definite_then_recovers(eng):
    L, ctx = nat.lib(), eng.ctx
    x = _mixture(seed=10)
    x[:, 5] = -2.0                                    # a zero column after standardising, and eps = 0
    rows = init_rows(len(x), 26, seed=4)
    out = ctypes.c_void_p()
    rc = L.ssym_gmm_train(ctx, x.ctypes.data, len(x), 12, 26, rows.ctypes.data, 0.0, 5, nat.GMM_STANDARDIZE,
                          ctypes.byref(out))
    assert rc == nat.SSYM_E_INVALID
    assert "not positive definite" in L.ssym_last_error(ctx).decode()
    assert not out.value
    with pytest.raises(SsymError, match="not positive definite"):
        eng.gmm_train(x, 12, rows, 0.0, 5)
    # the context goes on working
    g = _train_check(eng, _mixture(seed=12), 26, 0.1, 5)
    g.close()


def test_two_runs_same_bits_largest_model(eng):
    x = _mixture(seed=13, K=64, d=64, n=20000)
    rows = init_rows(len(x), 64, seed=5)
    a, b = eng.gmm_train(x, 64, rows, 0.1, 3), eng.gmm_train(x, 64, rows, 0.1, 3)
    assert a.iters == b.iters and a.log_lik == b.log_lik
    for u, v in ((a.weights, b.weights), (a.means, b.means), (a.covs, b.covs)):
        assert np.array_equal(_bits(u), _bits(v))
    la, pa = eng.gmm_predict(a, x, want_post=True)
    lb, pb = eng.gmm_predict(a, x, want_post=True)
    assert np.array_equal(_bits(pa), _bits(pb)) and np.array_equal(la, lb)
    a.close()
    b.close()


@pytest.mark.parametrize("ncoeffs", [13, 20])
def test_partitioner_more_coefficients(eng, ncoeffs):
    samples, rate = read_wav(SAMPLE)
    snd = Sound.from_samples(samples, rate, ncoeffs=ncoeffs, engine=eng)
    p = Partitioner(snd, eng)
    p.train(seed=0)
    splits = p.partition()
    feats = snd.mfccs().reshape(-1, ncoeffs)
    assert sum(splits) == len(feats) * HOP
    m = p.model
    assert m.dim == ncoeffs
    assert splits == [f * HOP for f in ref.partition(feats, m.weights, m.means, m.covs, 5, 4)]


@pytest.mark.parametrize("A,d", VOTE_CASES)
def test_votes_at_the_key_limits(eng, A, d):
    s = np.random.default_rng(A + d).integers(0, A, 5000)
    s[[17, 4000]] = A - 1                             # the largest symbol (255 at A = 256) is present
    for t in (2, d - 1):
        _check_votes(eng, s, A, d, t)


def _de_bruijn(k, n):
    """The linear de Bruijn string B(k, n): every n-gram over k symbols exactly once (length k^n + n - 1)."""
    a, out = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return np.array(out + out[:n - 1], dtype=np.uint8)


@pytest.mark.parametrize("kind", ["distinct", "constant", "period7"])
def test_votes_exact_ties(eng, kind):
    # z-scores exactly 0 (every n-gram distinct, or one n-gram per length): every window is an exact tie and both
    # sides must take the first maximum
    if kind == "distinct":
        s, A, depths = _de_bruijn(16, 3), 16, (5, 3)
        assert len({tuple(s[i:i + 3]) for i in range(len(s) - 2)}) == len(s) - 2
    elif kind == "constant":
        s, A, depths = np.zeros(5000, dtype=np.uint8), 2, (5, 2)
    else:
        s, A, depths = (np.arange(5000) % 7).astype(np.uint8), 7, (5, 8)
    for d in depths:
        for t in (1, d - 1):
            _check_votes(eng, s, A, d, t)


def test_vote_limits_rejected(eng):
    L, ctx = nat.lib(), eng.ctx
    s = np.zeros(100, dtype=np.uint8)
    seg = np.zeros(100, dtype=np.uint64)
    m = ctypes.c_uint64()
    for A, d, text in ((2, 63, "2^63"), (257, 3, "alphabet")):
        rc = L.ssym_vote_segments(ctx, s.ctypes.data, 100, A, d, 1, 0, None, seg.ctypes.data, ctypes.byref(m))
        assert rc == nat.SSYM_E_INVALID
        assert text in L.ssym_last_error(ctx).decode()
    # 2^62 is accepted
    _check_votes(eng, s, 2, 62, 1)
