"""What the GPU tests of the resynthesiser share -- TEST INFRASTRUCTURE: a resynthesiser with one restatement lane
(tests/live_resynth_ref.py) per lane, every call made on both and compared bit for bit, samples and pcm (Live); the same
over the linear oracle of tests/resynth_slices.py, for many lanes and long tiles (SlicedLive)."""
import numpy as np

import live_resynth_ref as ref
from live_resynth_ref import GAP, HOP, NO_MATCH
from resynth_slices import SlicedLane
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


class SlicedLive:
    """A resynthesiser and the linear oracle (tests/resynth_slices.py), for many lanes and long tiles: lanes {lane: (rows,
    total_samples)} is what each lane will consume and end with, so a call names only how many rows each lane takes.  Every
    call is compared bit for bit, samples and pcm, with its count, the lane offsets and counts(); a flush compares the lane's
    concatenation since its reset with `offline`.  Only the lanes of a call are walked in Python: the others are held to empty
    stretches by the offsets, so 65535 lanes cost no more than five."""

    def __init__(self, engine, store, sounds, n_lanes, search, lanes, cache=None):
        self.sounds, self.n_lanes, self.search, self.cache = sounds, n_lanes, search, cache
        self.rs = engine.resynth(store, n_lanes, search)
        self.refs = {l: SlicedLane(sounds, rows, total, search, cache) for l, (rows, total) in lanes.items()}
        self.out = {l: [] for l in lanes}
        self.frames, self.samples = np.zeros(n_lanes, dtype=np.uint64), np.zeros(n_lanes, dtype=np.uint64)
        self.calls = []                              # per call {lane: (room, hops released)}: what the hop list held

    def _compare(self, n, want, what):
        sizes = np.zeros(self.n_lanes, dtype=np.uint64)
        for l, w in want.items():
            sizes[l] = w.size
        want_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        off, smp, pcm = self.rs.samples(want_pcm32=True)
        assert n == self.rs.n_samples == smp.size == pcm.size == int(want_off[-1]), (what, n, int(want_off[-1]))
        assert np.array_equal(off, want_off), what
        for l in sorted(want):
            a, b = int(off[l]), int(off[l + 1])
            same(smp[a:b], want[l], "%s, lane %d" % (what, l))
            assert np.array_equal(pcm[a:b], pcm32(want[l])), (what, l)
            self.out[l].append(want[l])
        self.samples += sizes
        frames, released = self.rs.counts()
        assert np.array_equal(frames, self.frames) and np.array_equal(released, self.samples), what

    def push(self, take, what="push"):
        """take {lane: rows to consume}; a lane with 0 is absent from the arrays, as a lane left out is."""
        rows = {l: self.refs[l].rows(k) for l, k in take.items() if k}
        at = {l: self.refs[l].n for l in rows}
        room = {l: self.refs[l].held + k for l, k in take.items() if k}
        n = self.rs.push(*columns(rows, at))
        want = {l: self.refs[l].push(k) for l, k in take.items()}
        for l, k in take.items():
            self.frames[l] += k
        self.calls.append({l: (room[l], want[l].size // HOP) for l in room})
        self._compare(n, want, what)
        return n

    def flush(self, lane, total=None):
        """Flush `lane`; a lane without frames ends with `total` samples."""
        if lane not in self.refs:
            self.refs[lane], self.out[lane] = SlicedLane(self.sounds, [], total, self.search, self.cache), []
        r = self.refs[lane]
        assert total is None or total == r.total
        n = self.rs.flush(lane, r.total)
        self._compare(n, {lane: r.flush()}, "flush of lane %d" % lane)
        same(np.concatenate(self.out[lane]), r.whole, "lane %d, reset to flush" % lane)
        return n

    def reset(self, lane, rows, total):
        self.rs.reset(lane)
        self.refs[lane], self.out[lane] = SlicedLane(self.sounds, rows, total, self.search, self.cache), []
        self.frames[lane] = self.samples[lane] = 0

    def held(self, lane):
        return self.refs[lane].held

    def close(self):
        self.rs.close()
