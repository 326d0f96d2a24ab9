"""ssym_spotter_* under SSYM_STEP_PACED at the shapes test_gpu_paced_watch.py stops short of: dynamic LDS (two hand-off rows
and the ring) on both sides of every 64 KiB crossing at or under the 2048-frame limit and at its maximum, a 2048-frame
pair of state rows next to 1-frame and 0-frame targets on three lanes that advance at different rates with a reset in
mid-stream, and the slice path down to slices of one and two rows.  Every push is held to tests/paced_watch_ref.py
through test_gpu_watch's machinery: profile, events and best, bit for bit."""
import numpy as np
import pytest

import wave_lds
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments
from test_gpu_paced_watch import _PW, _limits, _profiles
from test_gpu_watch import NO, _bits, _check_split, _frames

pytestmark = pytest.mark.gpu

PACED_MAX = 2048                             # kSpotterPacedMaxTargetFrames


def paced_lds_bytes(dim, max_fb):
    """Bytes of one paced launch whose longest target has max_fb frames of dim values (dtw_wave.hpp's spot_lds_bytes with
    SSYM_STEP_PACED): two hand-off rows of (f64, u32) per target frame and the ring of target frames."""
    return 2 * wave_lds.wave_fb_cap(max_fb) * 12 + wave_lds.wave_ring_rows(max_fb) * wave_lds.wave_ld(wave_lds.wave_dimr(dim)) * 8


def crossing(dim):
    """The longest target at or under the limit whose launch stays within 64 KiB, or None when every launch does."""
    below = [fb for fb in range(1, PACED_MAX + 1) if paced_lds_bytes(dim, fb) <= wave_lds.LIMIT]
    assert below == list(range(1, len(below) + 1))                             # one crossing: the bytes never come back down
    return None if len(below) == PACED_MAX else below[-1]


def _cases():
    out = []
    for dim in (64, 41, 40, 17, 16, 15):                                       # both ends of each DIMR's range of dims
        fb = crossing(dim)
        out += [(dim, fb, False), (dim, fb + 1, True)]
    return out + [(64, PACED_MAX, True), (2, PACED_MAX, False)]


def test_the_crossings_are_where_the_arithmetic_puts_them():
    assert [crossing(d) for d in (64, 41, 40, 17, 16, 15, 14, 2)] == [64, 64, 938, 938, 1962, 1962, None, None]
    assert paced_lds_bytes(64, PACED_MAX) == 116736 and paced_lds_bytes(2, PACED_MAX) == 63488
    assert paced_lds_bytes(40, 938) == paced_lds_bytes(16, 1962) == 65520 and paced_lds_bytes(64, 64) == 35328


# ---- 1. both sides of every LDS crossing ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,fb,above", _cases())
def test_every_lds_crossing(dim, fb, above):
    need = paced_lds_bytes(dim, fb)
    assert (need > wave_lds.LIMIT) == above and need <= 160 * 1024, (dim, fb, need)     # the side this case is meant to be on
    rng = np.random.default_rng(0x9D5 + 4099 * dim + fb)
    # a lane of 130 frames; no path of a target of more than 259 frames ends inside it (the shortest span has
    # floor((Fb-1)/2) + 1 frames), so such a target gets one more push that carries the lane 66 rows past that
    rows = 130 if fb <= 259 else (fb - 1) // 2 + 66
    lane, tgt = _frames(rng, rows, dim, "real"), [_frames(rng, fb, dim, "real")]
    prof = _profiles([lane], tgt, False)
    assert np.count_nonzero(np.isfinite(prof[(0, 0)][0])) >= 60
    w = _PW(tgt, dim)
    # a one-row chunk, a full chunk, a one-row chunk right after a full one, a two-chunk push
    reps = _check_split(w, [lane], [[0, 1, 64, 65, 130] + [rows] * (rows > 130)], prof)
    w.close()
    assert sum(r.stats["events"] for r in reps.values()) >= 1


# ---- 2. state stride and offsets: two long rows between tiny ones, three lanes, carried state, a reset --------------------

def test_a_2048_frame_state_next_to_tiny_ones_on_three_lanes_and_a_reset_in_mid_stream():
    rng = np.random.default_rng(0x57A9E)
    dim = 2
    tgt = [_frames(rng, f, dim, "int") for f in (1, PACED_MAX, 0, 129, 2)]
    lanes = [_frames(rng, f, dim, "int") for f in (150, 90, 130)]
    # no path of the 2048-frame target ends inside lanes this short: its two rows are state traffic between the others',
    # and a write that strays from them shows in their profiles.  The 129-frame target is planted in lane 0.
    lanes[0][10:139] = tgt[3]
    cuts = [[0, 64, 64, 129, 140], [0, 1, 2, 66, 90], [0, 0, 0, 0, 100]]
    nT = len(tgt)
    prof = _profiles(lanes, tgt, True)
    w = _PW(tgt, dim, n_lanes=3, squared=True)
    si, ti = np.repeat(np.arange(3, dtype=np.uint32), nT), np.tile(np.arange(nT, dtype=np.uint32), 3)

    def best_is_the_spot_of_the_prefix(p):
        sf, so = pack_segments([lanes[l][:cuts[l][p + 1]] for l in range(3)], dim)
        d = w.e.dictionary(sf, so, dim)
        c1, s1, e1 = w.e.dtw_spot(d, w.q, si, ti, step="paced")
        cost, start, end = w.sp.best()
        assert np.array_equal(_bits(cost.reshape(-1)), _bits(c1)), p
        assert np.array_equal(start.reshape(-1), s1) and np.array_equal(end.reshape(-1), e1), p
        d.close()

    _check_split(w, lanes, cuts, prof, flush_end=False, after_push=best_is_the_spot_of_the_prefix)
    best = w.sp.best()
    assert np.isinf(best[0][:, [1, 2]]).all() and (best[2][:, [1, 2]] == NO).all()      # too long for these lanes; empty
    assert np.isfinite(best[0][:, [0, 4]]).all() and (best[0][0, 3], best[1][0, 3], best[2][0, 3]) == (0.0, 10, 138)

    # lane 1 starts over; lanes 0 and 2 keep their best, their counts and -- shown by their next rows -- their state rows
    before = [x.copy() for x in best]
    w.sp.reset(1)
    assert w.sp.counts().tolist() == [140, 0, 100]
    after = w.sp.best()
    for x, y in zip(before, after):
        assert np.array_equal(x[[0, 2]].view(np.uint8), y[[0, 2]].view(np.uint8))
    assert np.isinf(after[0][1]).all() and (after[1][1] == NO).all() and (after[2][1] == NO).all()
    again = [0, 1, 2, 67, 90]                                                  # rows 0 and 1 on their own: no row above, then one
    empty = np.zeros((0, dim))
    for lo, hi in zip(again, again[1:]):
        rc, n, pd, ps, _ = w.push([empty, lanes[1][lo:hi], empty])
        assert rc == nat.SSYM_OK
        for t in (0, 1, 3, 4):
            d, s = prof[(1, t)]
            assert np.array_equal(_bits(pd[1][t]), _bits(d[lo:hi])) and np.array_equal(ps[1][t], s[lo:hi].astype(np.uint32)), (lo, t)
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


# ---- 3. the slice path, down to slices of one and two rows -----------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 2, 23])
def test_a_sliced_push_equals_the_unsliced_push(monkeypatch, rows):
    rng = np.random.default_rng(0x511C9)
    tgt = [_frames(rng, f, 3, "int") for f in (4, 70)]
    lane = _frames(rng, 130, 3, "int")
    prof = _profiles([lane], tgt, True)
    limit = _limits(prof, 2)
    whole = _PW(tgt, 3, max_cost=limit, squared=True)
    a = whole.push([lane])
    ev_a = whole.events()
    assert a[0] == nat.SSYM_OK and whole.e.timings()["main_launches"] == 1 and a[1] >= 3
    monkeypatch.setenv("SSYM_SPOTTER_SCRATCH_BYTES", str(12 * 2 * rows))       # one lane, two targets: `rows` rows per slice
    w = _PW(tgt, 3, max_cost=limit, squared=True)
    b = w.push([lane])
    ev_b = w.events()
    assert b[0] == nat.SSYM_OK and w.e.timings()["main_launches"] == -(-130 // rows)
    assert a[1] == b[1] and np.array_equal(_bits(a[4][0]), _bits(b[4][0])) and np.array_equal(a[4][1], b[4][1])
    assert ev_a == ev_b and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(whole.sp.best(), w.sp.best()))
    w.sp.reset(0)
    reps = _check_split(w, [lane], [[0, 1, 66, 130]], prof)                    # sliced pushes against the restatement
    assert sum(r.stats["events"] for r in reps.values()) >= 3
    whole.close()
    w.close()
