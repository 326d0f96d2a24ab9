"""What the GPU tests of the mosaicker share -- TEST INFRASTRUCTURE: a mosaicker on an engine with a resident dictionary
(coverer_gpu.Dict) with one restatement lane (tests/live_mosaic_ref.py) per lane, and the comparison of every call's frames
and state, bit for bit."""
import numpy as np

import live_mosaic_ref as ref
import mosaic_ref
from coverer_gpu import Dict, error, hooks  # noqa: F401
from paced_match_gpu import bits

INF = float("inf")


def same_frames(got, want, what=""):
    """Two lists of (column, src, frame, cost, start): everything, the cost by its bits."""
    assert [(f[0], f[1], f[2], int(f[4])) for f in got] == [(f[0], f[1], f[2], int(f[4])) for f in want], (what, got[:4], want[:4])
    assert bits([f[3] for f in got]).tolist() == bits([f[3] for f in want]).tolist(), what


def by_lane(mk):
    """lane -> [(column, src, frame, cost, start)] of the last call's frames; they are ordered by (lane, column)."""
    lane, col, src, frame, cost, start = mk.frames()
    assert lane.size == mk.n_frames
    key = list(zip(lane.tolist(), col.tolist()))
    assert key == sorted(key), key
    out = {}
    for k in range(lane.size):
        out.setdefault(int(lane[k]), []).append((int(col[k]), int(src[k]), int(frame[k]), float(cost[k]), int(start[k])))
    return out


class Live:
    """A mosaicker and its restatement, lane by lane: every call is made on both and compared."""

    def __init__(self, D, n_lanes=1, penalty=0.0, gap=None):
        self.D, self.n_lanes, self.penalty, self.gap = D, n_lanes, penalty, gap
        self.mk = D.e.mosaicker(D.d, n_lanes, penalty, gap)
        self.refs = [self._lane() for _ in range(n_lanes)]
        self.emitted = [[] for _ in range(n_lanes)]

    def _lane(self):
        segs = [np.asarray(a, dtype=np.float64).reshape(-1, self.D.dim) for a in self.D.src]
        return ref.Lane(segs, self.D.dim, self.penalty, INF if self.gap is None else self.gap, self.D.squared)

    def push(self, chunks):
        """One push of chunks[l] ([m][dim], possibly empty) to lane l; returns the frames per lane.  The restatement
        commits frame by frame: by consequence 2 the union after the push is c(n) whatever the slices were."""
        chunks = [np.asarray(c, dtype=np.float64).reshape(-1, self.D.dim) for c in chunks]
        off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
        n = self.mk.push(np.concatenate(chunks, axis=0), off)
        got = by_lane(self.mk)
        for l, (r, c) in enumerate(zip(self.refs, chunks)):
            want = r.push(c)
            same_frames(got.get(l, []), want, "lane %d at %d frames" % (l, r.n))
            self.emitted[l] += want
        assert n == sum(len(v) for v in got.values())
        self.check_best()
        return got

    def flush(self, lane=0):
        n = self.mk.flush(lane)
        got = by_lane(self.mk)
        want = self.refs[lane].flush()
        same_frames(got.get(lane, []), want, "flush of lane %d" % lane)
        assert n == len(want) and set(got) <= {lane}
        self.emitted[lane] += want
        self.check_best()
        return want

    def reset(self, lane=0):
        self.mk.reset(lane)
        self.refs[lane] = self._lane()
        self.emitted[lane] = []
        self.check_best()

    def check_best(self):
        total, covered, committed = self.mk.best()
        want = [r.best() for r in self.refs]
        assert bits(total).tolist() == bits([w[0] for w in want]).tolist(), (total, want)
        assert covered.tolist() == [w[1] for w in want] and committed.tolist() == [w[2] for w in want], (covered, committed, want)
        frames, cap = self.mk.counts()
        assert frames.tolist() == [r.n for r in self.refs]
        return cap

    def lag(self, lane=0):
        return self.refs[lane].n - 1 - self.refs[lane].done

    def close(self):
        self.mk.close()


def offline(D, x, penalty, gap=None):
    """ssym_dtw_mosaic on the same context for one target: the six arrays."""
    q = D.queries([x])
    try:
        return D.e.dtw_mosaic(D.d, q, penalty, gap)
    finally:
        q.close()


def same_as_offline(D, frames, x, penalty, gap=None, what=""):
    """the frames emitted from reset to flush for the target x: ssym_dtw_mosaic's six arrays on this context, and
    mosaic_ref.arrays"""
    T = np.asarray(x).shape[0]
    count, start, src, frame, cost = ref.frames_to_arrays(frames, T)
    segs = [np.asarray(a, dtype=np.float64).reshape(-1, D.dim) for a in D.src]
    for want in (offline(D, x, penalty, gap), mosaic_ref.arrays(segs, [x], penalty, INF if gap is None else gap, D.squared)):
        assert count == int(want[0][0]), what
        for got, exp in zip((start, src, frame), want[2:5]):
            assert got.tolist() == np.asarray(exp).tolist(), what
        assert bits(cost).tolist() == bits(want[5]).tolist(), what
