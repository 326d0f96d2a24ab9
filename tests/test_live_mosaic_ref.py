"""The live mosaic's commit rule on the CPU (tests/live_mosaic_ref.py against tests/mosaic_ref.py): what is committed is
never revised, two weakened rules are, and the frames from reset to flush are the offline mosaic's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import live_mosaic_ref as ref  # noqa: E402
import mosaic_ref  # noqa: E402

INF = float("inf")
N_CASES = 500


def random_case(seed):
    """half-integer values (sums and ties are exact), dim 1-2, 1-3 segments of 0-9 frames, T 3-23, a NaN frame in ~15 %"""
    rng = np.random.default_rng(0x11FE0000 + seed)
    dim = int(rng.integers(1, 3))
    segs = [rng.integers(-4, 5, size=(int(rng.integers(0, 10)), dim)) / 2.0 for _ in range(int(rng.integers(1, 4)))]
    x = rng.integers(-4, 5, size=(int(rng.integers(3, 24)), dim)) / 2.0
    if rng.random() < 0.15:
        if rng.random() < 0.5 or not any(a.shape[0] for a in segs):
            x[int(rng.integers(0, x.shape[0]))] = np.nan
        else:
            a = segs[int(rng.choice([k for k, a in enumerate(segs) if a.shape[0]]))]
            a[int(rng.integers(0, a.shape[0]))] = np.nan
    penalty = float(rng.choice([0.0, 0.5, 1.0, 3.0]))
    gap = float(rng.choice([INF, 1.0, 2.0]))
    return segs, x, penalty, gap


CASES = [random_case(s) for s in range(N_CASES)]


def test_commits_are_never_revised():
    assert N_CASES >= 400
    for k, (segs, x, penalty, gap) in enumerate(CASES):
        assert not ref.revised(segs, x, penalty, gap), k


@pytest.mark.parametrize("rule", ["no_n", "arg_only"])
def test_weakened_rules_are_revised(rule):
    """the test above bites: without the N-state hypotheses, or with arg(n-1) alone, committed frames change later"""
    n = sum(ref.revised(segs, x, penalty, gap, rule=rule) for segs, x, penalty, gap in CASES)
    print(rule, "revised", n, "of", N_CASES)
    assert n > 0


def test_emitted_frames_are_the_offline_mosaic():
    """reset to flush, pushed in pieces of 1, 3 and everything: mosaic_ref.arrays of the whole target (of the prefix with a
    mosaic where the lane died)"""
    for k, (segs, x, penalty, gap) in enumerate(CASES):
        dim = x.shape[1]
        for step in (1, 3, x.shape[0]):
            lane = ref.Lane(segs, dim, penalty, gap)
            frames = []
            for a in range(0, x.shape[0], step):
                new = lane.push(x[a:a + step])
                assert [f[0] for f in new] == list(range(len(frames), len(frames) + len(new))), k
                frames += new
            total, covered, committed = lane.best()
            assert committed == len(frames), k
            frames += lane.flush()
            assert len(frames) == covered, k
            want = mosaic_ref.arrays(segs, [x[:covered]], penalty, gap)
            count, start, src, frame, cost = ref.frames_to_arrays(frames, covered)
            assert count == int(want[0][0]), k
            for got, exp in zip((start, src, frame, cost), want[2:]):
                assert got.tobytes() == exp.tobytes(), k
            whole = mosaic_ref.arrays(segs, [x], penalty, gap)
            assert total == whole[1][0], k


def test_commit_depends_on_frames_not_pushes():
    for segs, x, penalty, gap in CASES[:60]:
        want = ref.commits(segs, x, penalty, gap)
        lane = ref.Lane(segs, x.shape[1], penalty, gap)
        for n in range(1, x.shape[0] + 1):
            lane.push(x[n - 1:n])
            assert lane.done == max(want[:n])


def test_planted_case_commits():
    recs, x, _ = mosaic_ref.planted_case()
    want = list(range(11)) + [10, 12, 12, 14, 14, 16, 16, 18, 18, 20, 20, 22] + list(range(23, 31))
    assert ref.commits(recs, x, 1.0) == want


def test_boundary_case_commits():
    segs, x, _ = mosaic_ref.boundary_case()
    assert ref.commits(segs, x, 1.0) == [0, 1]


def test_intruder_case_commits():
    recs, x, _, _ = mosaic_ref.intruder_case()
    got = ref.commits(recs, x, 1.0, 1.5)
    assert len(got) == 26                                   # n = 26 is the whole target: all of it is committed but the lag
    assert all(n - 1 - c <= 1 for n, c in enumerate(got, start=1))
