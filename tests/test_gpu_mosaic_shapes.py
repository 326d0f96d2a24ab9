"""ssym_dtw_mosaic on the GPU held to tests/mosaic_ref.py bit for bit at every shape it takes another path on (DESIGN.md
section 5.25): G of 1, 2, 63, 64, 65, the workgroup's 1024 threads -1 / +0 / +1 and 2 x 1024 + 3; segments of 0, 1 and 2
frames with empty segments in the middle; targets of 0, 1, 2 and 257 frames, ragged in one call; 1, 13 and 64 values per
frame; the squared option; integer features; penalties of 0, 0.3 and 20; no gaps and a gap price of 0.7; host and
SSYM_OUT_DEVICE outputs; outputs passed as NULL."""
import numpy as np
import pytest

from mosaic_gpu import INF, Sets, check, real
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

THREADS = 1024                      # kMosaicThreads


def split(rng, G, dim, ints=False):
    """G source frames as three segments around an empty one."""
    a = G // 3
    lens = [a, 0, G - a - (G - a) // 2, (G - a) // 2]
    if ints:
        return [rng.integers(0, 3, (f, dim)).astype(np.float64) for f in lens]
    return [real(rng, f, dim) for f in lens]


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 3])
def test_source_frames_around_the_wave_and_the_workgroup(G):
    rng = np.random.default_rng(G)
    src = split(rng, G, 3)
    tgt = [real(rng, 9, 3), real(rng, 4, 3)]
    with Sets(src, tgt, 3) as sets:
        check(sets, 0.3)
        check(sets, 0.3, 0.7, device=True)


def test_integer_features_tie_at_every_thread_count():
    """Ties everywhere: the smallest g must win whichever thread and wave holds it."""
    rng = np.random.default_rng(11)
    src = split(rng, 2 * THREADS + 3, 1, ints=True)
    tgt = [rng.integers(0, 3, (7, 1)).astype(np.float64), np.ones((5, 1))]
    with Sets(src, tgt, 1, squared=True) as sets:
        for penalty, gap in ((0.0, INF), (1.0, 1.0), (20.0, INF)):
            check(sets, penalty, gap)


def test_short_and_empty_segments():
    rng = np.random.default_rng(12)
    src = [real(rng, f, 2) for f in (2, 0, 1, 0, 0, 2, 1)]
    tgt = [real(rng, f, 2) for f in (5, 1, 0, 3)]
    with Sets(src, tgt, 2) as sets:
        for penalty in (0.0, 0.3, 20.0):
            check(sets, penalty)
            check(sets, penalty, 0.7)


@pytest.mark.parametrize("dim", [1, 13, 64])
def test_ragged_targets_of_0_1_2_and_257_frames(dim):
    rng = np.random.default_rng(dim)
    src = [real(rng, f, dim) for f in (64, 1, 65)]
    tgt = [real(rng, f, dim) for f in (0, 1, 2, 257, 5)]
    tgt[3][40:50] = src[2][3:13]                             # something worth a piece inside the long target
    with Sets(src, tgt, dim) as sets:
        check(sets, 0.3)
        check(sets, 20.0, 0.7, device=True)
    with Sets(src, tgt, dim, dtype="f32", squared=True) as sets:
        check(sets, 0.0)
        check(sets, 0.3, 0.7)


def test_null_outputs():
    """Every output is nullable, host and device: what is asked for keeps its bits, what is not stays unwritten."""
    rng = np.random.default_rng(13)
    src, tgt = [real(rng, 20, 4), real(rng, 30, 4)], [real(rng, 12, 4), real(rng, 3, 4)]
    with Sets(src, tgt, 4) as sets:
        for keep in ((True, True, False, False, False, False), (False, False, True, True, True, True),
                     (False, True, False, True, False, True), (False,) * 6):
            check(sets, 0.3, 0.7, keep=keep)
            check(sets, 0.3, 0.7, keep=keep, device=True)
        assert sets.e.timings()["n_pairs"] == 50 * 15
