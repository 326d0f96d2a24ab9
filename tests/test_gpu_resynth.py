"""ssym_resynth_* on the GPU against the restatement (tests/live_resynth_ref.py), bit for bit, samples and pcm: a store of
sounds with 5000, 2600 and 1 samples; lanes 1 and 3 with an empty lane between; tiles of 1, 2, 3, 4, 5 and 17 frames (the
small ones make taps cross a tile start, 17 is more than one synthesis workgroup's 16 hops); gap runs of 1 and 3; a tile
whose source runs out and frames beyond their recording; pushes one frame at a time, all at once and cut at each tile start
and at +-1 of it; searches 0, 8, 256 | 257 (R goes from 5 to 6) and 512 (five lags per thread); tails of 0, 768, 1023 and
5000; reset then reuse; NaN samples; SSYM_OUT_DEVICE."""
import numpy as np
import pytest

import live_resynth_ref as ref
from resynth_gpu import G, Live, bits, columns, same, tile
from soundsym_amd import Engine
from warp_ref import HOP, pcm32

pytestmark = pytest.mark.gpu

SOUND_SAMPLES = (5000, 2600, 1)
SEARCHES = (0, 8, 256, 257, 512)
N_LANES = 4
LANE = {
    0: tile(0, [0, 1, 2]),
    1: ([G] + tile(0, [3]) + tile(0, [5, 5]) + tile(1, [0, 2, 2]) + [G, G, G] + tile(0, [10, 11, 11, 13]) + tile(1, [4, 5, 6, 6, 7])
        + tile(0, [0, 1, 1, 2, 3, 3, 4, 5, 6, 6, 7, 8, 10, 12, 13, 14, 15])        # 17 frames
        + tile(1, [7, 8, 9, 10, 11, 12])                                          # the source runs out at 2600 = 10 hops + 40
        + tile(2, [0, 1, 2]) + tile(2, [5, 5]) + tile(0, [25, 26])                # frames beyond their recording
        + tile(0, [17, 18, 19, 20])),                                             # open until the flush, inside the reach
    2: [],
    3: tile(1, [1, 2, 4, 4, 5]) + [G] + tile(0, [2]) + [G, G],
}
TAIL = {0: 0, 1: 1023, 2: 5000, 3: 768}
TOTAL = {l: len(rows) * HOP + TAIL[l] for l, rows in LANE.items()}
STARTS = [j for j, r in enumerate(LANE[1]) if r[2] and j]
CACHE = {s: {} for s in SEARCHES}


class _Rig:
    def __init__(self, sounds=None):
        rng = np.random.default_rng(0x7E5)
        self.sounds = sounds if sounds is not None else [rng.normal(size=n) * 0.3 for n in SOUND_SAMPLES]
        self.e = Engine(metric="dtw", dtype="f64", device=0)
        off = np.concatenate([[0], np.cumsum([s.size for s in self.sounds])]).astype(np.uint64)
        self.store = self.e.samples(np.concatenate(self.sounds), off)

    def live(self, search, cache=None, n_lanes=N_LANES):
        return Live(self.e, self.store, self.sounds, n_lanes, search, CACHE[search] if cache is None else cache)

    def close(self):
        self.store.close()
        self.e.close()


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    yield r
    r.close()


def _schedule(kind):
    """The pushes as {lane: (from, to)} per call."""
    n = {l: len(rows) for l, rows in LANE.items()}
    if kind == "all":
        return [{l: (0, n[l]) for l in LANE if n[l]}]
    if kind == "one":
        return [{l: (j, j + 1) for l in LANE if j < n[l]} for j in range(max(n.values()))]
    cuts = sorted({min(max(t + kind, 1), n[1]) for t in STARTS} | {n[1]})       # lane 1 cut at every tile start + kind
    calls, at = [], 0
    for c in cuts:
        if c > at:
            calls.append({1: (at, c)})
            at = c
    calls[0].update({l: (0, n[l]) for l in (0, 3)})
    return calls


@pytest.mark.parametrize("kind", ("one", "all", -1, 0, 1))
@pytest.mark.parametrize("search", SEARCHES)
def test_pushes_and_flushes_are_the_restatements(rig, search, kind):
    live = rig.live(search)
    try:
        R = ref.reach(search)
        for call in _schedule(kind):
            live.push({l: LANE[l][a:b] for l, (a, b) in call.items()}, "search %d, %r, %r" % (search, kind, call))
            assert all(live.held(l) <= 2 * R for l in LANE)
        for l in (3, 2, 1, 0):
            assert live.flush(l, TOTAL[l]) >= TAIL[l]
        assert sum(p.size for p in live.out[2]) == 5000 and not np.concatenate(live.out[2]).any()     # a lane without frames
    finally:
        live.close()


def test_reset_then_reuse(rig):
    live = rig.live(8)
    try:
        live.push({0: LANE[3][:4], 1: LANE[1][:20]})
        assert live.held(0) and live.held(1)                    # frames are held back when the lane is reset
        live.reset(0)
        live.push({0: LANE[1][:30]})
        live.flush(0, 30 * HOP + 5000)                          # a tail of 5000 behind an open sounding tile
        live.reset(0)
        live.push({0: LANE[0]})
        live.flush(0, TOTAL[0])
        live.push({1: LANE[1][20:]})                            # lane 1 was not disturbed
        live.flush(1, TOTAL[1])
    finally:
        live.close()


@pytest.mark.parametrize("search", (0, 64))
def test_nan_samples_stay_inside_their_taps(search):
    """Every sample outside the windows of the tiles is NaN: no output changes its bits.  One NaN inside a window: the NaN
    mask is the restatement's, and so are the bits wherever its sample is a number."""
    clean = _Rig()
    rows = tile(0, [4, 5, 5, 6, 8, 9]) + [G] + tile(1, [2, 3, 4])
    total = len(rows) * HOP + 300
    try:
        want = ref.offline(clean.sounds, rows, total, search)
        poisoned = [s.copy() for s in clean.sounds]
        poisoned[0][:4 * HOP] = np.nan
        poisoned[0][10 * HOP:] = np.nan
        poisoned[1][:2 * HOP] = np.nan
        poisoned[1][5 * HOP:] = np.nan
        poisoned[2][:] = np.nan
        inside = [s.copy() for s in clean.sounds]
        inside[0][6 * HOP + 17] = np.nan
        for sounds, exact in ((poisoned, True), (inside, False)):
            r = _Rig(sounds)
            try:
                rs = r.e.resynth(r.store, 1, search)
                got = []
                for a in range(0, len(rows), 2):
                    rs.push(*columns({0: rows[a:a + 2]}, {0: a}))
                    got.append(rs.samples()[1])
                rs.flush(0, total)
                off, smp, pcm = rs.samples(want_pcm32=True)
                got = np.concatenate(got + [smp])
                rs.close()
                if exact:
                    same(got, want, "NaN outside the windows, search %d" % search)
                else:
                    exp = ref.offline(sounds, rows, total, search)
                    nan = np.isnan(exp)
                    assert nan.any() and nan.sum() < 2 * 1024 and np.array_equal(np.isnan(got), nan)
                    assert np.array_equal(bits(got)[~nan], bits(exp)[~nan])
                    assert np.array_equal(pcm, pcm32(got[got.size - smp.size:]))          # NaN -> 0
            finally:
                r.close()
    finally:
        clean.close()


def test_device_outputs_and_nullable_outputs(rig):
    live = rig.live(0)
    try:
        live.push({1: LANE[1][:12], 3: LANE[3]})
        off, smp, pcm = live.rs.samples(want_pcm32=True)
        doff, dsmp, dpcm = live.rs.samples(want_pcm32=True, on_device=True)
        assert dsmp.is_cuda and dpcm.is_cuda and np.array_equal(off, doff)
        same(dsmp.cpu().numpy(), smp, "SSYM_OUT_DEVICE")
        assert np.array_equal(dpcm.cpu().numpy(), pcm)
        only_off, only_smp = live.rs.samples()
        assert np.array_equal(only_off, off) and np.array_equal(bits(only_smp), bits(smp))
        tm = live.rs.engine.timings()
        assert tm["main_ms"] == 0.0 and tm["main_launches"] == 0 and tm["n_pairs"] == 12 + len(LANE[3])
    finally:
        live.close()
