"""A coverer made by ssym_coverer_create_gaps on the GPU held to the live restatement of tests/cover_gaps_ref.py and to
ssym_dtw_cover_gaps on the same context, bit for bit (DESIGN.md section 2 "Live cover" with gaps, section 5.24): totals after
every push, the same pieces however the frames are cut, never revised, flush = the offline cover with gaps, a frame that is
not finite as a gap frame the lane goes on past, follow from a stream, and ssym_coverer_create as it was."""
import ctypes

import numpy as np
import pytest

import cover_gaps_ref as ref
import coverer_gpu as cg
import live_cover_ref
from coverer_gpu import INF, bits, by_lane, same_pieces
from paced_match_gpu import real
from soundsym_amd import SsymError
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

GAP = ref.GAP
LENS = (40, 17, 9, 25, 33, 5, 1, 21, 12, 29)             # Fmax = 40: W = 80


def _segments(seed=0x11C0):
    rng = np.random.default_rng(seed)
    return [real(rng, n, 13) for n in LENS]


def _recording(segs, frames, seed):
    """Noisy copies of dictionary segments (a few tenths per frame away) between frames of the recording's own (about 5 per
    frame away from every segment): with a gap_cost between the two a cover has pieces and gaps."""
    rng = np.random.default_rng(seed)
    parts, k = [], 0
    while sum(p.shape[0] for p in parts) < frames:
        a = segs[(3, 0, 7, 2, 9, 4)[k % 6]]
        parts += [(a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32).astype(np.float64), real(rng, 2 + 5 * (k % 3), 13)]
        k += 1
    return np.concatenate(parts)[:frames]


def offline(D, x, penalty, gap_cost):
    """ssym_dtw_cover_gaps on the same context for one target: (pieces, one per gap frame; total)."""
    q = D.queries([x])
    try:
        count, total, src, start, end, cost = D.e.dtw_cover(D.d, q, penalty, gap_cost=gap_cost)
    finally:
        q.close()
    return [(int(src[i]), int(start[i]), int(end[i]), float(cost[i])) for i in range(int(count[0]))], float(total[0])


class Live:
    """A coverer with gaps and its restatement, lane by lane: every call is made on both and compared."""

    def __init__(self, D, n_lanes, penalty, gap_cost):
        self.D = D
        self.cv = D.e.coverer(D.d, n_lanes, penalty, gap_cost)
        self.refs = [ref.Lane(D.src, penalty, gap_cost, D.squared) for _ in range(n_lanes)]
        self.emitted = [[] for _ in range(n_lanes)]

    def push(self, chunks):
        chunks = [np.asarray(c, dtype=np.float64).reshape(-1, self.D.dim) for c in chunks]
        off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
        n = self.cv.push(np.concatenate(chunks, axis=0), off)
        got = by_lane(self.cv)
        for l, (r, c) in enumerate(zip(self.refs, chunks)):
            want = r.push(c)
            same_pieces(got.get(l, []), want, "lane %d at %d frames" % (l, r.n))
            self.emitted[l] += want
        assert n == sum(len(v) for v in got.values())
        self.check_best()
        return got

    def flush(self, lane):
        n = self.cv.flush(lane)
        got = by_lane(self.cv)
        want = self.refs[lane].flush()
        same_pieces(got.get(lane, []), want, "flush of lane %d" % lane)
        assert n == len(want) and set(got) <= {lane}
        self.emitted[lane] += want
        self.check_best()

    def check_best(self):
        total, covered, committed = self.cv.best()
        want = [r.state() for r in self.refs]
        assert bits(total).tolist() == bits([w[0] for w in want]).tolist(), (total, want)
        assert covered.tolist() == [w[1] for w in want] and committed.tolist() == [w[2] for w in want]
        assert self.cv.counts()[0].tolist() == [r.n for r in self.refs]

    def close(self):
        self.cv.close()


@pytest.fixture(scope="module")
def world():
    """The dictionary on one engine, a recording of 700 frames, and the restatement of the whole recording per (penalty,
    gap_cost), computed once: its best(e) are the totals after every push, however the frames are cut."""
    class Wd:
        pass
    w = Wd()
    w.segs = _segments()
    w.x = _recording(w.segs, 700, 0x70F)
    w.whole = {}
    for penalty, gap_cost in ((0.0, 1.0), (2.0, 3.0)):
        lane = ref.Lane(w.segs, penalty, gap_cost)
        lane.push(w.x)
        lane.flush()
        w.whole[penalty, gap_cost] = lane
    with cg.Dict(w.segs, 13) as D:
        w.D = D
        yield w


@pytest.mark.parametrize("penalty,gap_cost", [(0.0, 1.0), (2.0, 3.0)])
def test_one_push_sixteen_frame_pushes_and_frame_by_frame(world, penalty, gap_cost):
    D, x, whole = world.D, world.x, world.whole[penalty, gap_cost]
    want, want_total = whole.emitted, whole.total()
    kinds = {p[0] == GAP for p in want}
    assert kinds == {True, False} and ref.tiles(want, 700)
    off, off_total = offline(D, x, penalty, gap_cost)
    same_pieces(off, want, "ssym_dtw_cover_gaps")
    assert bits(off_total) == bits(want_total)

    # 16-frame pushes against the restatement cut the same way: every push's pieces, total, covered and committed
    live = Live(D, 1, penalty, gap_cost)
    for a in range(0, 700, 16):
        live.push([x[a:a + 16]])
        assert live.refs[0].state()[1] == min(a + 16, 700)                    # every best(e) is finite: covered = n
        same_pieces(live.emitted[0], want[:len(live.emitted[0])], "never revised")
    assert 0 < len(live.emitted[0]) < len(want)
    live.flush(0)
    same_pieces(live.emitted[0], off, "flush = the offline cover with gaps")
    live.close()

    # one push, and frame by frame over a shorter stretch (the whole's best(e) are the totals of every prefix)
    for frames, step in ((700, 700), (150, 1)):
        cv = D.e.coverer(D.d, 1, penalty, gap_cost)
        want_f, want_f_total = (want, want_total) if frames == 700 else offline(D, x[:frames], penalty, gap_cost)
        emitted = []
        for a in range(0, frames, step):
            cv.push(x[a:a + step])
            emitted += by_lane(cv).get(0, [])
            total, covered, committed = cv.best()
            assert bits(total[0]) == bits(whole.best[min(a + step, frames)]) and covered[0] == min(a + step, frames)
            assert committed[0] == (emitted[-1][2] + 1 if emitted else 0)
            if step == 1:
                same_pieces(emitted, want[:len(emitted)], "never revised, frame by frame")
        cv.flush(0)
        emitted += by_lane(cv).get(0, [])
        same_pieces(emitted, want_f, "%d frames in pushes of %d" % (frames, step))
        assert bits(cv.best()[0][0]) == bits(want_f_total)
        with pytest.raises(SsymError):
            cv.push(x[:1])                                                     # flushed: the lane has ended
        cv.close()


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_frame_that_is_not_finite_on_one_of_three_lanes(world, value):
    D = world.D
    lanes = [_recording(world.segs, n, 0x3A + k) for k, n in enumerate((200, 230, 170))]
    broken = [x.copy() for x in lanes]
    broken[1][90] = value
    runs = []
    for data in (lanes, broken):
        live = Live(D, 3, 0.0, 1.0)
        per_push = []
        for a in range(0, 230, 48):
            per_push.append(live.push([x[a:a + 48] for x in data]))
        for l in range(3):
            live.flush(l)
        runs.append((per_push, live.emitted))
        live.close()
    (clean_push, clean), (bad_push, bad) = runs
    for l in (0, 2):                                                           # the other lanes: bit-identical
        assert [p.get(l, []) for p in clean_push] == [p.get(l, []) for p in bad_push]
        same_pieces(bad[l], clean[l], "lane %d beside the broken one" % l)
    assert (GAP, 90, 90, 1.0) in bad[1] and ref.tiles(bad[1], 230)             # the lane goes on past the frame
    assert sum(len(p.get(1, [])) for p in bad_push[2:]) > 0                    # ... and commits past it before the flush
    assert max(e for p in bad_push for _, _, e, _ in p.get(1, [])) > 90
    same_pieces(bad[1], offline(D, broken[1], 0.0, 1.0)[0], "flush = the offline cover with gaps")


def test_follow_is_push_of_the_streams_frames():
    rng = np.random.default_rng(0xF0110)
    segs = [real(rng, n, 12, 4.0) for n in (1, 3, 6, 2, 9)]
    waves = [rng.standard_normal(9000) * 0.3, np.sin(0.03 * np.arange(7000)) + 0.1 * rng.standard_normal(7000)]
    with cg.Dict(segs, 12) as D:
        e = D.e
        st = e.stream(2, 44100.0, 12)
        followed, pushed = e.coverer(D.d, 2, 1.0, 20.0), Live(D, 2, 1.0, 20.0)
        have, gaps = [0, 0], 0
        for cut in ((0, 0), (3000, 500), (3000, 4000), (9000, 7000)):
            chunks = [w[h:c] for w, h, c in zip(waves, have, cut)]
            have = list(cut)
            st.push(np.concatenate(chunks), np.concatenate([[0], np.cumsum([c.size for c in chunks])]))
            consumed = followed.counts()[0]
            n = followed.follow(st)
            got = by_lane(followed)
            want = pushed.push([st.read(l)[int(consumed[l]):] for l in range(2)])
            assert got == want and n == sum(len(v) for v in want.values())
            gaps += sum(p[0] == GAP for v in got.values() for p in v)
            for a, b in zip(followed.best(), pushed.cv.best()):
                assert a.tobytes() == b.tobytes()
        assert followed.counts()[0].tolist() == st.counts()[1].tolist() and min(followed.counts()[0]) > 20
        for l in range(2):
            followed.flush(l)
            got = by_lane(followed).get(l, [])
            pushed.flush(l)
            gaps += sum(p[0] == GAP for p in got)
            same_pieces(pushed.emitted[l][len(pushed.emitted[l]) - len(got):], got, "flush of lane %d" % l)
            assert ref.tiles(pushed.emitted[l], int(st.counts()[1][l]))
        kinds = {p[0] == GAP for l in range(2) for p in pushed.emitted[l]}
        assert gaps > 0 and kinds == {True, False}
        for h in (followed, pushed, st):
            h.close()


def test_a_coverer_without_gaps_is_as_it_was(world):
    """ssym_coverer_create, and ssym_coverer_create_gaps with +inf: live_cover_ref's lane, which ends at a NaN frame."""
    D = world.D
    x = _recording(world.segs, 200, 0x51)
    x[120] = np.nan
    for make in (lambda: D.e.coverer(D.d, 1, 0.0), lambda: D.e.coverer(D.d, 1, 0.0, INF)):
        cv = make()
        lane = live_cover_ref.Lane(world.segs, 0.0)
        for a in range(0, 200, 40):
            cv.push(x[a:a + 40])
            same_pieces(by_lane(cv).get(0, []), lane.push(x[a:a + 40]), "push at %d" % a)
            total, covered, committed = cv.best()
            assert (bits(total[0]), covered[0], committed[0]) == (bits(lane.state()[0]), lane.state()[1], lane.state()[2])
        assert cv.best()[1][0] == 120 and cv.best()[0][0] == INF               # the coverable prefix ended at the NaN
        cv.flush(0)
        same_pieces(by_lane(cv).get(0, []), lane.flush(), "flush")
        assert lane.emitted[-1][2] == 119 and all(p[0] != GAP for p in lane.emitted)
        cv.close()


def test_refusals_at_creation(world):
    D = world.D
    out = ctypes.c_void_p(0x1234)
    for bad in (float("nan"), -1.0, -INF):
        rc = nat.lib().ssym_coverer_create_gaps(D.e.ctx, D.d.ptr, 1, 0.0, bad, ctypes.byref(out))
        assert rc == nat.SSYM_E_INVALID and out.value is None and "gap_cost" in cg.error(D.e)
    for kw in (dict(metric="refcos"), dict(band=8)):
        with cg.Dict(world.segs, 13, **kw) as other:
            with pytest.raises(SsymError) as err:
                other.e.coverer(other.d, 1, 0.0, 1.0)
            assert err.value.code == nat.SSYM_E_UNSUPPORTED and "ssym_coverer_create_gaps" in str(err.value)
