"""ssym_spotter_* at the shapes it accepts and test_gpu_watch.py stops short of: targets from 127 to 4096 frames (the ring
wrapping once, twice, 64 times; the limit itself), dynamic LDS on both sides of every 64 KiB crossing and at its
maximum, a 4096-frame state row next to 1-frame and 0-frame targets on three lanes that advance at different rates, and
the slice path with a long target.  Every push is held to tests/watch_ref.py through test_gpu_watch's machinery: profile,
events and best, bit for bit."""
import numpy as np
import pytest

import spot_ref
import watch_ref
import wave_lds
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments
from test_gpu_watch import NO, _W, _bits, _check_split, _frames

pytestmark = pytest.mark.gpu

# ---- 1. target lengths x splits -------------------------------------------------------------------------------------------

TGT_FRAMES = [127, 128, 129, 192, 193, 200, 257, 4096]    # ring 128 full; 3 and 4 refills; a ring slot's second reuse; the limit
LANE = 200
_RANDOM = [0, 0, 17, 17, 17, 80, 81, 144, 144, 145, 199, LANE, LANE]          # empty pushes, first, middle and last
SPLITS = {"whole": [0, LANE], "63": list(range(0, LANE, 63)) + [LANE], "64": list(range(0, LANE, 64)) + [LANE],
          "65": list(range(0, LANE, 65)) + [LANE], "random": _RANDOM}
_DATA = {}


def _data():
    """The lane, the targets and the profile cache of tests 1 and 4: made once, shared, never written to again."""
    if not _DATA:
        rng = np.random.default_rng(0x10A6)
        _DATA["x"] = (_frames(rng, LANE, 2, "int"), [_frames(rng, f, 2, "int") for f in TGT_FRAMES], {})
    return _DATA["x"]


def _limits(lane, tgt, prof):
    """One threshold per target, the 0.4 quantile of its own profile: some rows are candidates, some are not."""
    out = []
    for t in range(len(tgt)):
        if (0, t) not in prof:
            prof[(0, t)] = watch_ref.whole_profile(lane, tgt[t], True)
        out.append(float(np.quantile(prof[(0, t)][0], 0.4)))
    return out


@pytest.mark.parametrize("split", list(SPLITS))
def test_long_targets_under_every_split(split):
    lane, tgt, prof = _data()
    w = _W(tgt, 2, max_cost=_limits(lane, tgt, prof), squared=True)
    reps = _check_split(w, [lane], [SPLITS[split]], prof)
    w.close()
    assert sum(r.stats["events"] for r in reps.values()) >= 3
    # ties are real: the least value of an end column is held by several rows, and the cells of a 257-frame target's
    # matrix have tied predecessors
    assert any(np.count_nonzero(prof[(0, t)][0] == prof[(0, t)][0].min()) > 1 for t in range(len(tgt)))
    D = spot_ref.matrices(lane, tgt[6], True)[0]
    dg, up, lf = D[:-1, :-1], D[:-1, 1:], D[1:, :-1]
    least = np.minimum(np.minimum(dg, up), lf)
    assert np.count_nonzero((dg == least).astype(int) + (up == least) + (lf == least) > 1) > 100


# ---- 2. both sides of every LDS crossing ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,fb,above", wave_lds.CROSSINGS)
def test_every_lds_crossing(dim, fb, above):
    need = wave_lds.spot_lds_bytes(dim, fb)
    assert (need > wave_lds.LIMIT) == above, (dim, fb, need)     # the side this case is meant to be on
    if (dim, fb) == (64, 4096):
        assert need == 116736                                    # the largest launch there is
    if (dim, fb) == (14, 4096):
        assert need == 63488                                     # the largest below the attribute call
    rng = np.random.default_rng(0x1D5 + 4099 * dim + fb)
    lane, tgt = _frames(rng, 130, dim, "real"), [_frames(rng, fb, dim, "real")]
    w = _W(tgt, dim)
    # a one-row chunk, a full chunk, a one-row chunk right after a full one, a two-chunk push
    reps = _check_split(w, [lane], [[0, 1, 64, 65, 130]])
    w.close()
    assert sum(r.stats["events"] for r in reps.values()) >= 1


# ---- 3. state stride and offsets: a long row between tiny ones, three lanes, carried state -------------------------------

def test_a_4096_frame_state_row_next_to_tiny_ones_on_three_lanes():
    rng = np.random.default_rng(0x57A7E)
    dim = 2
    tgt = [_frames(rng, f, dim, "int") for f in (4096, 1, 0, 129, 2)]          # the empty target sits in the middle
    lanes = [_frames(rng, f, dim, "int") for f in (150, 90, 130)]
    # the lanes advance at different rates; lane 2 gets empty pushes until the last; lanes 0 and 2 keep frames back
    cuts = [[0, 64, 64, 129, 140], [0, 1, 2, 66, 90], [0, 0, 0, 0, 100]]
    w = _W(tgt, dim, n_lanes=3, squared=True)
    nT, prof = len(tgt), {}
    si, ti = np.repeat(np.arange(3, dtype=np.uint32), nT), np.tile(np.arange(nT, dtype=np.uint32), 3)

    def best_is_the_spot_of_the_prefix(p):
        sf, so = pack_segments([lanes[l][:cuts[l][p + 1]] for l in range(3)], dim)
        d = w.e.dictionary(sf, so, dim)
        c1, s1, e1 = w.e.dtw_spot(d, w.q, si, ti)
        cost, start, end = w.sp.best()
        assert np.array_equal(_bits(cost.reshape(-1)), _bits(c1)), p
        assert np.array_equal(start.reshape(-1), s1) and np.array_equal(end.reshape(-1), e1), p
        d.close()

    _check_split(w, lanes, cuts, prof, flush_end=False, after_push=best_is_the_spot_of_the_prefix)
    assert np.isinf(w.sp.best()[0][:, 2]).all() and (w.sp.best()[2][:, 2] == NO).all()     # the empty target
    assert np.isfinite(w.sp.best()[0][:, [0, 1, 3, 4]]).all()

    # lane 1 starts over; lanes 0 and 2 keep their best, their counts and -- shown by their next rows -- their state rows
    before = [x.copy() for x in w.sp.best()]
    w.sp.reset(1)
    assert w.sp.counts().tolist() == [140, 0, 100]
    after = w.sp.best()
    for x, y in zip(before, after):
        assert np.array_equal(x[[0, 2]].view(np.uint8), y[[0, 2]].view(np.uint8))
    assert np.isinf(after[0][1]).all() and (after[1][1] == NO).all() and (after[2][1] == NO).all()
    again = [[0, 0, 0], [0, 65, 90], [0, 0, 0]]
    empty = np.zeros((0, dim))
    for p in range(2):
        lo, hi = again[1][p], again[1][p + 1]
        rc, n, pd, ps, _ = w.push([empty, lanes[1][lo:hi], empty])
        assert rc == nat.SSYM_OK
        for t in (0, 1, 3, 4):
            d, s = prof[(1, t)]
            assert np.array_equal(_bits(pd[1][t]), _bits(d[lo:hi])) and np.array_equal(ps[1][t], s[lo:hi].astype(np.uint32)), (p, t)
    cost, start, end = w.sp.best()
    for x, y in zip(before, (cost, start, end)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))             # lane 1 is where it was, the others never moved
    rc, n, pd, ps, _ = w.push([lanes[0][140:], empty, lanes[2][100:]])
    assert rc == nat.SSYM_OK and w.sp.counts().tolist() == [150, 90, 130]
    for l, lo in ((0, 140), (2, 100)):
        for t in (0, 1, 3, 4):
            d, s = prof[(l, t)]
            assert np.array_equal(_bits(pd[l][t]), _bits(d[lo:])) and np.array_equal(ps[l][t], s[lo:].astype(np.uint32)), (l, t)
    w.close()


# ---- 4. the slice path with a 4096-frame target ----------------------------------------------------------------------------

def test_slices_with_a_4096_frame_target_equal_the_unsliced_run(monkeypatch):
    lane, tgt, prof = _data()
    limit = _limits(lane, tgt, prof)[7]
    whole = _W(tgt[7:], 2, max_cost=limit, squared=True)
    a = whole.push([lane])
    ev_a = whole.events()
    assert a[0] == nat.SSYM_OK and whole.e.timings()["main_launches"] == 1
    monkeypatch.setenv("SSYM_SPOTTER_SCRATCH_BYTES", str(12 * 23))            # one lane, one target: 23 rows per slice
    w = _W(tgt[7:], 2, max_cost=limit, squared=True)
    b = w.push([lane])
    ev_b = w.events()
    assert b[0] == nat.SSYM_OK and w.e.timings()["main_launches"] == 9        # ceil(200 / 23)
    assert a[1] == b[1] and np.array_equal(_bits(a[4][0]), _bits(b[4][0])) and np.array_equal(a[4][1], b[4][1])
    assert ev_a == ev_b and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(whole.sp.best(), w.sp.best()))
    w.sp.reset(0)
    reps = _check_split(w, [lane], [[0, LANE]], {(0, 0): prof[(0, 7)]})       # the same sliced push against the restatement
    assert sum(r.stats["events"] for r in reps.values()) >= 1
    whole.close()
    w.close()
