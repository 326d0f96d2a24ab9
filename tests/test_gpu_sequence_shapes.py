"""ssym_sequence_distances at every dim and past its grid caps, against test_gpu_sequence.py's restatement.

tests/test_gpu_sequence.py runs at most 11 pairs in one distance workgroup and a few hundred means.  Here: every dim from
1 to 64; 10 000 sounds x 64 coefficients, so frame_means_kernel's grid (num_cus * 8 blocks of 256 threads) makes a thread
fold more than one (sound, coefficient) pair and neighbour_distances_kernel runs 9 999 pairs over 40 workgroups; one
sound of 100 003 frames in a batch; the device-input path with frame offsets that do not start at 0.  Means and
similarities must be bit-equal, distances within 1e-15, NaN in the same places (tests/test_descriptor_boundaries.py
checks the sizes against the kernels' constants).
"""
import numpy as np
import pytest

from soundsym_amd import Engine
from test_gpu_sequence import _check_distances, _mean_fold, _same_bits

pytestmark = pytest.mark.gpu
DIMS = list(range(1, 65))
MANY_SOUNDS, MANY_DIM = 10000, 64                  # n * dim = 640 000 (sound, coefficient) pairs, 9 999 pairs
LONG_FRAMES = 100003


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="refcos", dtype="f64")
    yield e
    e.close()


def _blocks(counts, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(int(t), dim)) * (0.02 if k % 3 else 3.0) + (0.5 if k % 5 == 1 else 0.0)
            for k, t in enumerate(counts)]


def _flat(blocks, dim):
    feats = np.concatenate([b.reshape(-1) for b in blocks]) if blocks else np.zeros(0)
    off = np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.uint64)
    return feats, off


def _run_and_check(eng, oracle, blocks, dim, feats=None, off=None, means=None):
    if feats is None:
        feats, off = _flat(blocks, dim)
    dist, mean, sim = eng.sequence_distances(feats, off, dim, want_mean=True, want_sim=True)
    if means is None:
        means = [_mean_fold(b, dim) for b in blocks]
    assert all(_same_bits(mean[i], means[i]) for i in range(len(blocks)))
    _check_distances(dist, sim, means, oracle)
    return dist, mean, sim


@pytest.mark.parametrize("dim", DIMS)
def test_every_dim(eng, oracle, dim):
    counts = [3, 1, 0, 7, 2, 5, 1, 1, 9, 4, 2, 6]
    _run_and_check(eng, oracle, _blocks(counts, dim, dim), dim)


def test_many_sounds_past_the_caps(eng, oracle):
    rng = np.random.default_rng(17)
    counts = rng.integers(0, 6, MANY_SOUNDS)
    blocks = _blocks(counts, MANY_DIM, 3)
    feats, off = _flat(blocks, MANY_DIM)
    # the block means restated vectorised: the same sequential fold over every block at once
    T = int(counts.max())
    acc = np.zeros((MANY_SOUNDS, MANY_DIM))
    for t in range(T):
        live = counts > t
        acc[live] = acc[live] + np.stack([b[t] for b, c in zip(blocks, counts) if c > t])
    with np.errstate(invalid="ignore"):
        means = acc / counts[:, None]
    for i in range(0, MANY_SOUNDS, 997):
        assert _same_bits(means[i], _mean_fold(blocks[i], MANY_DIM))
    dist, mean, sim = _run_and_check(eng, oracle, blocks, MANY_DIM, feats, off, means)
    assert dist.shape == (MANY_SOUNDS - 1,) and np.isnan(dist).any() and not np.isnan(dist).all()
    # host input whose frame offsets start past 0: the same values for the sounds [k, n)
    k = 333
    sub = eng.sequence_distances(feats, off[k:], MANY_DIM, want_mean=True, want_sim=True)
    assert _same_bits(sub[0], dist[k:]) and _same_bits(sub[1], mean[k:]) and _same_bits(sub[2], sim[k:])


def test_one_very_long_sound(eng, oracle):
    dim = 12
    blocks = _blocks([4, LONG_FRAMES, 0, 2, 300, 1], dim, 23)
    _run_and_check(eng, oracle, blocks, dim)


def test_device_input_offsets_not_at_zero(eng, oracle):
    import torch
    dim = 20
    rng = np.random.default_rng(29)
    counts = rng.integers(0, 9, 700)
    counts[:3] = (5, 0, 2)
    blocks = _blocks(counts, dim, 31)
    feats, off = _flat(blocks, dim)
    k = 2                                                 # the sequence starts at block 2: off[0] = 5 frames
    host = _run_and_check(eng, oracle, blocks[k:], dim, feats, off[k:])
    assert int(off[k]) == 5
    dev = torch.from_numpy(feats).to("cuda")
    got = eng.sequence_distances(dev, off[k:], dim, want_mean=True, want_sim=True)
    for a, b in zip(got, host):
        assert _same_bits(a, b)
