"""The coverer with 300 lanes: one grid row or workgroup per lane over per-lane slices of the tail,
the ring of best values, the back-pointer store and the piece log, a second block of coverer_best_kernel from lane 256 on,
and coverer_regrow_kernel over 300 lanes with different `done` and `n`.  A seeded schedule (tests/count_cases.py, checked
in tests/test_count_cases.py) feeds about half of the lanes per call, never feeds some, ends some and starts some over;
coverer_gpu.Live holds every call's pieces, best and counts to tests/live_cover_ref.py, and at the end every lane's pieces
to ONE ssym_dtw_cover call over the 300 sequences.

The restatement costs a millisecond per lane and push, so it runs once per penalty: the first run of a penalty writes what
every lane answered on a tape and a knob run of the same schedule reads the tape, where coverer_gpu.Live would ask a lane."""
import collections

import numpy as np
import pytest

import count_cases as cc
import cover_ref
import coverer_gpu as cg
import live_cover_ref as ref

pytestmark = pytest.mark.gpu

INF = float("inf")


class Taped:
    """What coverer_gpu.Live asks of a restatement lane.  With a lane: the lane's answers, written on the tape as well.
    Without one: the answers the tape holds, which were given to the same calls (the frames are compared)."""

    def __init__(self, tape, lane=None):
        self.tape, self.lane = tape, lane
        self.n, self.done, self.now = 0, -1, (INF, 0, 0)

    def _answer(self, what, frames, call):
        if self.lane is not None:
            out = call()
            self.tape.append((what, frames.tobytes(), out, self.lane.n, self.lane.done, self.lane.state()))
        asked, data, out, self.n, self.done, self.now = self.tape[-1] if self.lane is not None else self.tape.popleft()
        assert (asked, data) == (what, frames.tobytes())
        return list(out)

    def push(self, frames):
        frames = np.asarray(frames, dtype=np.float64)
        return self._answer("push", frames, lambda: self.lane.push(frames)) if frames.shape[0] else []

    def flush(self):
        return self._answer("flush", np.zeros(0), lambda: self.lane.flush())

    def state(self):
        return self.now


class TapedLive(cg.Live):
    """coverer_gpu.Live whose restatement lanes write tapes (tapes=None) or are read from them."""

    def __init__(self, D, n_lanes, penalty, tapes=None):
        super().__init__(D, n_lanes, penalty)
        self.record = tapes is None
        self.tapes = [[] for _ in range(n_lanes)] if tapes is None else [collections.deque(t) for t in tapes]
        self.refs = [self._lane(l) for l in range(n_lanes)]

    def _lane(self, l):
        return Taped(self.tapes[l], ref.Lane(self.D.src, self.penalty, self.D.squared) if self.record else None)

    def reset(self, lane=0):
        self.cv.reset(lane)
        self.refs[lane] = self._lane(lane)
        self.emitted[lane] = []
        self.check_best()


@pytest.fixture(scope="module")
def schedule():
    return cc.Schedule()


@pytest.fixture(scope="module")
def D(schedule):
    with cg.Dict(schedule.segs, cc.LANES_DIM) as d:
        yield d


@pytest.fixture(scope="module")
def tables_once():
    """cover_ref.tables does not take the penalty: the runs at penalty 2 and 20 ask for the same windows, once each."""
    tables, memo = cover_ref.tables, {}

    def remembered(src, x, squared=False):
        key = (id(src), squared, np.asarray(x).shape, np.asarray(x).tobytes())
        if key not in memo:
            memo[key] = tables(src, x, squared)
        return tuple(a.copy() for a in memo[key])

    cover_ref.tables = remembered
    yield
    cover_ref.tables = tables


def run(D, schedule, penalty, tapes=None, after_push=None):
    """The schedule on a new coverer, then a flush of every lane that has not ended: (emitted pieces per lane, tapes)."""
    live = TapedLive(D, cc.LANES, penalty, tapes)
    try:
        for op in schedule.ops:
            if op[0] == "push":
                live.push(op[1])
                if after_push:
                    after_push(live)
            elif op[0] == "flush":
                live.flush(op[1])
            else:
                live.reset(op[1])
        for l in range(cc.LANES):
            if l not in schedule.ended:
                live.flush(l)
        assert live.cv.counts()[0].tolist() == [x.shape[0] for x in schedule.whole]
        return live.emitted, live.tapes
    finally:
        live.close()


class _Runs:
    def __init__(self):
        self.plain = {}                                  # penalty -> (emitted, tapes) of the run without knobs


@pytest.fixture(scope="module")
def runs():
    return _Runs()


def plain(runs, D, schedule, penalty):
    if penalty not in runs.plain:
        runs.plain[penalty] = run(D, schedule, penalty)
    return runs.plain[penalty]


def same_emitted(got, want):
    for l, (g, w) in enumerate(zip(got, want)):
        cg.same_pieces(g, w, "lane %d" % l)


def test_300_lanes_and_one_cover_call_over_their_sequences(runs, D, schedule, tables_once):
    emitted, _ = plain(runs, D, schedule, 2.0)
    assert sum(1 for e in emitted if e) > 250 and all(not emitted[l] for l in schedule.never)
    assert len(emitted[256]) > 20 and len(emitted[299]) > 20
    q = D.queries(schedule.whole)
    try:
        count, total, src, start, end, cost = D.e.dtw_cover(D.d, q, 2.0)
    finally:
        q.close()
    off = np.concatenate([[0], np.cumsum([x.shape[0] for x in schedule.whole])])
    for l in range(cc.LANES):
        k = slice(int(off[l]), int(off[l]) + int(count[l]))
        cg.same_pieces(emitted[l], list(zip(src[k].tolist(), start[k].tolist(), end[k].tolist(), cost[k].tolist())),
                       "lane %d against ssym_dtw_cover" % l)


def test_slices_of_5_frames_emit_the_same(runs, D, schedule, tables_once):
    """Lanes drop out of a call's later slices at different times (0 ... 35 frames per lane and call)."""
    emitted, tapes = plain(runs, D, schedule, 2.0)
    launches = []
    with cg.hooks(SSYM_COVERER_SLICE=5):
        got, _ = run(D, schedule, 2.0, tapes, lambda live: launches.append(D.e.timings()["main_launches"]))
    same_emitted(got, emitted)
    longest = [max(c.shape[0] for c in op[1]) for op in schedule.ops if op[0] == "push"]
    assert launches == [-(-m // 5) for m in longest] and max(launches) == 7


def test_a_small_store_regrows_under_300_lanes(D, schedule, tables_once):
    """SSYM_COVERER_BACK=8 and penalty 20 (long pieces, long uncommitted stretches): the capacity follows the rule."""
    caps = []

    def capacity(live):
        caps.append(live.cv.counts()[1])
        assert caps[-1] == ref.capacity(live.needs, 8)

    with cg.hooks(SSYM_COVERER_BACK=8):
        got, tapes = run(D, schedule, 20.0, None, capacity)
    assert caps[0] >= 8 and caps == sorted(caps) and len(set(caps)) >= 3 and caps[-1] < ref.BACK_MIN
    emitted, _ = run(D, schedule, 20.0, tapes)           # the store of kCovererBackMin frames: it never regrows
    same_emitted(got, emitted)
    assert sum(1 for e in emitted if e) > 250


def test_out_device_for_best_and_pieces_of_300_lanes(D, schedule):
    chunks = next(op[1] for op in schedule.ops if op[0] == "push")
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
    cv = D.e.coverer(D.d, cc.LANES, 0.0)
    try:
        for _ in range(2):
            n = cv.push(np.concatenate(chunks, axis=0), off)
        host, dev = cv.pieces(), cv.pieces(on_device=True)
        assert n > 300 and host[0].max() > 256 and host[0].min() < 256
        for h, d in zip(host, dev):
            d = d.cpu().numpy()
            assert h.tobytes() == (d if h.dtype == np.float64 else d.view(np.uint32)).tobytes()
        best = cv.best()
        assert np.isfinite(best[0][256:]).any() and np.isposinf(best[0][sorted(schedule.never)]).all()
        assert best[1].tolist() == (2 * np.diff(off)).tolist()
        for h, d in zip(best, cv.best(on_device=True)):
            d = d.cpu().numpy()
            assert h.tobytes() == (d if h.dtype == np.float64 else d.view(np.uint32)).tobytes()
    finally:
        cv.close()
