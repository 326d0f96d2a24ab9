"""What the GPU tests of the coverer share -- TEST INFRASTRUCTURE: an engine with a resident dictionary, a coverer on it with
one restatement lane (tests/live_cover_ref.py) per lane, and the comparison of every call's pieces and state, bit for bit."""
import os

import numpy as np

import live_cover_ref as ref
from paced_match_gpu import SENT32, SENTF, bits  # noqa: F401
from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

INF = float("inf")


class Dict:
    """An engine with a resident dictionary made from a list of [frames, dim] arrays."""

    def __init__(self, src, dim, dtype="f64", squared=False, band=-1, metric="dtw"):
        self.src, self.dim, self.squared = src, dim, squared
        self.npd = np.float32 if dtype == "f32" else np.float64
        self.e = Engine(metric=metric, dtype=dtype, band=band, squared=squared)
        self.d = self.e.dictionary(*pack_segments(src, dim, self.npd), dim)

    def queries(self, tgt):
        return self.e.queries(*pack_segments(tgt, self.dim, self.npd), self.dim)

    def close(self):
        self.e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def error(e):
    return (nat.lib().ssym_last_error(e.ctx) or b"").decode()


def same_pieces(got, want, what=""):
    """Two lists of (src, start, end, cost): sources, cuts and cost bits."""
    assert [p[:3] for p in got] == [p[:3] for p in want], (what, got[:4], want[:4])
    assert bits([p[3] for p in got]).tolist() == bits([p[3] for p in want]).tolist(), what


def by_lane(cv):
    """lane -> [(src, start, end, cost)] of the last call's pieces; they are ordered by (lane, start)."""
    lane, src, start, end, cost = cv.pieces()
    assert lane.size == cv.n_pieces
    key = list(zip(lane.tolist(), start.tolist()))
    assert key == sorted(key), key
    out = {}
    for k in range(lane.size):
        out.setdefault(int(lane[k]), []).append((int(src[k]), int(start[k]), int(end[k]), float(cost[k])))
    return out


class Live:
    """A coverer and its restatement, lane by lane: every call is made on both and compared."""

    def __init__(self, D, n_lanes=1, penalty=0.0):
        self.D, self.n_lanes = D, n_lanes
        self.cv = D.e.coverer(D.d, n_lanes, penalty)
        self.refs = [ref.Lane(D.src, penalty, D.squared) for _ in range(n_lanes)]
        self.penalty = penalty
        self.needs = []                                  # per slice: uncommitted frames before it + its frames (see capacity)
        self.emitted = [[] for _ in range(n_lanes)]

    def push(self, chunks, slice_frames=1 << 40, check_best=True):
        """One push of chunks[l] ([m][dim], possibly empty) to lane l; returns the pieces per lane.  slice_frames: the
        frames per slice the library was told to use (SSYM_COVERER_SLICE) -- the restatement then consumes slice by slice
        too, which by consequence 2 gives the same pieces, and notes what the back-pointer ring had to hold per slice."""
        chunks = [np.asarray(c, dtype=np.float64).reshape(-1, self.D.dim) for c in chunks]
        off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
        n = self.cv.push(np.concatenate(chunks, axis=0), off)
        got = by_lane(self.cv)
        wants, at = [[] for _ in chunks], 0
        while any(at < c.shape[0] for c in chunks):
            parts = [c[at:at + slice_frames] for c in chunks]
            self.needs.append(max(r.n - 1 - r.done + p.shape[0] for r, p in zip(self.refs, parts) if p.shape[0]))
            for want, r, p in zip(wants, self.refs, parts):
                want += r.push(p)
            at += slice_frames
        for l, want in enumerate(wants):
            same_pieces(got.get(l, []), want, "lane %d at %d frames" % (l, self.refs[l].n))
            self.emitted[l] += want
        assert n == sum(len(v) for v in got.values())
        if check_best:
            self.check_best()
        return got

    def flush(self, lane=0):
        n = self.cv.flush(lane)
        got = by_lane(self.cv)
        want = self.refs[lane].flush()
        same_pieces(got.get(lane, []), want, "flush of lane %d" % lane)
        assert n == len(want) and set(got) <= {lane}
        self.emitted[lane] += want
        self.check_best()
        return want

    def reset(self, lane=0):
        self.cv.reset(lane)
        self.refs[lane] = ref.Lane(self.D.src, self.penalty, self.D.squared)
        self.emitted[lane] = []
        self.check_best()

    def check_best(self):
        total, covered, committed = self.cv.best()
        want = [r.state() for r in self.refs]
        assert bits(total).tolist() == bits([w[0] for w in want]).tolist(), (total, want)
        assert covered.tolist() == [w[1] for w in want] and committed.tolist() == [w[2] for w in want], (covered, committed, want)
        frames, cap = self.cv.counts()
        assert frames.tolist() == [r.n for r in self.refs]
        return cap

    def close(self):
        self.cv.close()


class hooks:
    """SSYM_TEST_HOOKS=1 with the given knobs for the block; the environment is put back."""

    def __init__(self, **knobs):
        self.env = dict({"SSYM_TEST_HOOKS": "1"}, **{k: str(v) for k, v in knobs.items()})

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def offline(D, x, penalty):
    """ssym_dtw_cover on the same context for one target: (pieces, total)."""
    q = D.queries([x])
    try:
        count, total, src, start, end, cost = D.e.dtw_cover(D.d, q, penalty)
    finally:
        q.close()
    k = int(count[0])
    return [(int(src[i]), int(start[i]), int(end[i]), float(cost[i])) for i in range(k)], float(total[0])
