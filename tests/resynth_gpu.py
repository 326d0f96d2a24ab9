"""What the GPU tests of the resynthesiser share -- TEST INFRASTRUCTURE: a resynthesiser with one restatement lane
(tests/live_resynth_ref.py) per lane, every call made on both and compared bit for bit, samples and pcm."""
import numpy as np

import live_resynth_ref as ref
from live_resynth_ref import GAP, HOP, NO_MATCH
from warp_ref import pcm32

G = (GAP, NO_MATCH, 1)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:4]], want[bad[:4]])


def tile(src, fmap):
    return [(src, f, int(j == 0)) for j, f in enumerate(fmap)]


def columns(rows_by_lane, at):
    """The five arrays of one push: rows_by_lane {lane: rows}, at {lane: the lane's frames so far}, ordered by (lane, column)."""
    out = [[], [], [], [], []]
    for l in sorted(rows_by_lane):
        for j, (src, frame, start) in enumerate(rows_by_lane[l]):
            for a, v in zip(out, (l, at[l] + j, src, frame, start)):
                a.append(v)
    return [np.array(a, dtype=np.uint32) for a in out]


class Live:
    """A resynthesiser and its restatement, lane by lane."""

    def __init__(self, engine, store, sounds, n_lanes, search, cache=None):
        self.sounds, self.n_lanes, self.search, self.cache = sounds, n_lanes, search, cache
        self.rs = engine.resynth(store, n_lanes, search)
        self.refs = [ref.LiveResynth(sounds, search, None, cache) for _ in range(n_lanes)]
        self.rows = [[] for _ in range(n_lanes)]
        self.out = [[] for _ in range(n_lanes)]

    def _compare(self, n, want, what):
        off, smp, pcm = self.rs.samples(want_pcm32=True)
        assert n == self.rs.n_samples == smp.size == pcm.size == int(off[-1]) and off[0] == 0, what
        for l in range(self.n_lanes):
            a, b = int(off[l]), int(off[l + 1])
            same(smp[a:b], want[l], "%s, lane %d" % (what, l))
            assert np.array_equal(pcm[a:b], pcm32(want[l])), (what, l)
            self.out[l].append(want[l])
        frames, released = self.rs.counts()
        assert frames.tolist() == [r.n for r in self.refs], what
        assert released.tolist() == [sum(p.size for p in o) for o in self.out], what

    def push(self, rows_by_lane, what="push"):
        at = {l: self.refs[l].n for l in rows_by_lane}
        n = self.rs.push(*columns(rows_by_lane, at))
        want = [self.refs[l].push(rows_by_lane[l]) if l in rows_by_lane else np.zeros(0) for l in range(self.n_lanes)]
        for l, rows in rows_by_lane.items():
            self.rows[l] += list(rows)
        self._compare(n, want, what)
        return n

    def flush(self, lane, total):
        n = self.rs.flush(lane, total)
        want = [self.refs[l].flush(total) if l == lane else np.zeros(0) for l in range(self.n_lanes)]
        self._compare(n, want, "flush of lane %d" % lane)
        whole = np.concatenate(self.out[lane])
        same(whole, ref.offline(self.sounds, self.rows[lane], total, self.search, self.cache), "lane %d, reset to flush" % lane)
        return n

    def reset(self, lane):
        self.rs.reset(lane)
        self.refs[lane] = ref.LiveResynth(self.sounds, self.search, None, self.cache)
        self.rows[lane], self.out[lane] = [], []

    def held(self, lane):
        return self.refs[lane].held

    def close(self):
        self.rs.close()
