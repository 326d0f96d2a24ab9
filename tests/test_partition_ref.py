"""The numpy restatement of the partitioner (tests/partition_ref.py) on hand-worked cases (CPU only)."""
import numpy as np
import pytest

import partition_ref as ref


def test_abab_depth2_votes_and_boundaries():
    # d = 2: every window has the one split i = 1, so both experts vote for w + 1 -> 2 votes at 1..N-1; only p = 1
    # rises above its left neighbour
    s = [0, 1] * 6
    vf, vh, _, _ = ref.vote_details(s, 2)
    assert list(vf) == [0] + [1] * 11 + [0] and list(vh) == list(vf)
    assert ref.boundaries(vf + vh, 1) == [1]
    assert ref.segments(s, 2, 1) == [1, 11]
    assert ref.segments(s, 2, 3) == [12]          # 2 votes never reach 3


def test_abab_depth3_votes_and_boundaries():
    # 1-grams a, b: 6 each (z = 0); 2-grams ab: 6, ba: 5 (z = +1, -1).  "aba" scores -1 at i = 1 and +1 at i = 2,
    # "bab" +1 at i = 1: the frequency expert votes at every even position twice.  All boundary entropies are 0
    # (z = 0), so the entropy expert takes the first split: one vote at each of 1..10.
    s = [0, 1] * 6
    vf, vh, _, _ = ref.vote_details(s, 3)
    assert list(vf) == [0, 0, 2, 0, 2, 0, 2, 0, 2, 0, 2, 0, 0]
    assert list(vh) == [0] + [1] * 10 + [0, 0]
    assert ref.boundaries(vf + vh, 1) == [2, 4, 6, 8, 10]
    assert ref.segments(s, 3, 1) == [2] * 6
    assert ref.segments(s, 3, 4) == [12]


def test_frequency_z_scores_from_integer_sums():
    s = [0, 0, 1, 0, 0, 1, 2]
    _, _, _, zf = ref.vote_details(s, 3)
    # 1-grams: counts 4, 2, 1 -> mean 7/3, var 21/3 - (7/3)^2
    mean = 7.0 / 3.0
    sd = np.sqrt(21.0 / 3.0 - mean * mean)
    assert np.array_equal(zf[0], (np.array([4.0, 2.0, 1.0]) - mean) / sd)


@pytest.mark.parametrize("seed", range(4))
def test_relabelling_keeps_the_segmentation(seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 6, 400)
    perm = rng.permutation(6)
    for d in (2, 3, 5):
        for t in (1, 2, d):
            assert ref.segments(s, d, t) == ref.segments(perm[s], d, t)


@pytest.mark.parametrize("n,d", [(1, 2), (4, 5), (5, 5), (300, 4), (1000, 7)])
def test_lengths_sum_to_n(n, d):
    s = np.random.default_rng(n).integers(0, 4, n)
    seg = ref.segments(s, d, 2)
    assert sum(seg) == n and all(x > 0 for x in seg)


def test_shorter_than_depth_is_one_segment():
    assert ref.segments([2, 1, 0], 5, 1) == [3]
    assert ref.segments([], 5, 1) == []


def test_standardiser_zero_variance_and_max_index():
    x = np.array([[1.0, 5.0], [2.0, 5.0], [4.0, 5.0]])
    z = ref.standardize(x)
    assert np.all(z[:, 1] == 0.0)
    assert np.isclose(z[:, 0].std(ddof=1), 1.0)
    assert ref.max_index([0.0, 0.0]) == 0 and ref.max_index([np.nan, 0.3, 0.3]) == 1
