"""The backward walk the mosaic and the live mosaic share (csrc/dtw_mosaic_common.hpp), against the Python restatement
(tests/mosaic_ref.py) through every kind of step: both callers run ONE walk, so a slip in it moves them together and no
"live equals offline" test sees it.

The case: three recordings of 40 / 33 / 27 frames x 2 values, G = 100 (two waves of source frames; recording 2 lies in the
second), and the first 20 frames of recording 2 are a copy of frames 10 ... 29 of recording 0.  The target has 48 frames: a
copy of frames 10 ... 31 of recording 0 (for 20 columns the walks through recording 0 and recording 2 tie bit for bit -- the
first least decides between the waves, and nothing commits until the copy runs past the shared stretch), frames 8 ... 11 of
recording 1 doubled (repeats), 6 frames that resemble nothing (gap frames at this gap_cost), every second frame of
14 ... 30 of recording 1 (skips, across source frame 64) and frames 21 ... 23 of recording 2, all with a little noise.  The
seed was chosen on the CPU with the restatement alone, so that `case` holds its conditions."""
import numpy as np
import pytest

import live_mosaic_ref as ref
import mosaic_ref
import mosaicker_gpu as mg
from mosaic_ref import GAP
from paced_match_gpu import bits

pytestmark = pytest.mark.gpu

PENALTY, GAP_COST, SEED = 1.0, 1.5, 0x5EED1


@pytest.fixture(scope="module")
def case():
    """(recordings, target, the six arrays of the restatement): computed once, conditions asserted before any comparison"""
    rng = np.random.default_rng(SEED)
    recs = [mosaic_ref._real(rng, (n, 2)) for n in (40, 33, 27)]
    recs[2][:20] = recs[0][10:30]
    x = np.concatenate([recs[0][10:32], np.repeat(recs[1][8:12], 2, axis=0), mosaic_ref._real(rng, (6, 2)) + 100.0,
                        recs[1][14:31:2], recs[2][21:24]], axis=0)
    x = (x + 0.02 * rng.standard_normal(x.shape)).astype(np.float32).astype(np.float64)
    assert x.shape == (48, 2) and 65 <= sum(r.shape[0] for r in recs) <= 130

    total, gmap, starts, _ = mosaic_ref.mosaic(recs, x, PENALTY, GAP_COST)
    assert np.isfinite(total)
    inside = [j for j in range(1, 48) if j not in starts and gmap[j] != GAP]          # columns that continue a piece
    assert {int(gmap[j] - gmap[j - 1]) for j in inside} == {0, 1, 2}                 # a repeat, a diagonal step and a skip
    assert sum(gmap[s] != GAP for s in starts) >= 3 and (gmap == GAP).sum() >= 1     # pieces open, and there are gap frames
    g = gmap[gmap != GAP]
    assert (g < 64).any() and (g >= 64).any()                                         # first minima in either wave
    # the mosaicker's lag passes a ring of 16 columns, so the ring regrows, and it commits before the end, through the wrap
    lag = [n - 1 - c for n, c in enumerate(ref.commits(recs, x, PENALTY, GAP_COST), start=1)]
    assert max(lag) >= 16 and min(lag[24:]) < 8 and lag[-1] > 0
    return recs, x, mosaic_ref.arrays(recs, [x], PENALTY, GAP_COST)


def _same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, k)
        assert (bits(a) if a.dtype == np.float64 else a).tolist() == (bits(b) if b.dtype == np.float64 else b).tolist(), (what, k)


def test_offline_walk_is_the_restatements(case):
    recs, x, want = case
    with mg.Dict(recs, 2) as D:
        _same(mg.offline(D, x, PENALTY, GAP_COST), want, "dtw_mosaic")


@pytest.mark.parametrize("step", [1, 5, 48])
def test_live_walk_is_the_restatements(case, step):
    recs, x, want = case
    with mg.Dict(recs, 2) as D, mg.hooks(SSYM_MOSAICKER_RING=16, SSYM_MOSAICKER_SLICE=7):
        mk = D.e.mosaicker(D.d, 1, PENALTY, GAP_COST)
        assert mk.counts()[1] == 16
        frames = []
        for a in range(0, 48, step):
            mk.push(x[a:a + step])
            frames += mg.by_lane(mk).get(0, [])
        assert 0 < len(frames) < 48 and mk.counts()[1] >= 32                          # committed through the wrap; regrown
        mk.flush()
        frames += mg.by_lane(mk).get(0, [])
        total = mk.best()[0]
        mk.close()
    assert [f[0] for f in frames] == list(range(48))
    count, start, src, frame, cost = ref.frames_to_arrays(frames, 48)
    _same(([count], total, start, src, frame, cost), want, "mosaicker, %d frames per push" % step)
