"""The probes of the mosaicker for tests/test_gpu_history.py's property: ssym_mosaicker_* give the same bits on a context that
ran something else before as on a fresh one.

tests/test_history_cases.py asks for a probe of every compute entry point the header declares; a call added after
tests/history_cases.py was written brings its probe in a file of its own (tests/test_gpu_history_paced_match.py says how
that works): importing this module registers the probes in history_cases.PROBES, their reference checks in
test_gpu_history.CHECKS and the mosaicker's lifecycle calls in history_cases.LIFECYCLE, and the bodies of the parametrised
history tests are run here for these probes."""
import numpy as np
import pytest

import history_cases as hc
import live_mosaic_ref as ref
import test_gpu_history as gh
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME, FOLLOW = "mosaicker", "mosaicker_follow"
PENALTY, GAP = 2.0, 9.0            # a frame is about 7 from another frame: some frames stay uncovered, most do not
hc.LIFECYCLE |= {"ssym_mosaicker_create", "ssym_mosaicker_destroy", "ssym_mosaicker_counts"}


def _state(mk):
    return list(mk.frames()) + list(mk.best())


def _chunks(lanes, cuts, p):
    """Push p of every lane; the lane that was reset starts again with its whole recording in the last push."""
    last = p == len(hc.SPOTTER_CUTS) - 2
    return [x if last and l == hc.SPOTTER_RESET_LANE else x[c[p]:c[p + 1]] for l, (x, c) in enumerate(zip(lanes, cuts))]


def _mosaicker(e, D, h, dictionary=None):
    """Every target of the set as a lane of one mosaicker on the set's sources, cut by spotter_cuts; one lane is reset."""
    if dictionary is None:
        sf, so = D.flat("src", e.np_dtype)
        dictionary = h.add(e.dictionary(sf, so, D.dim))
    lanes = D["tgt"]
    mk = h.add(e.mosaicker(dictionary, len(lanes), PENALTY, GAP))
    cuts = [hc.spotter_cuts(x.shape[0], D.variant.grow) for x in lanes]
    outs = []
    for p in range(len(hc.SPOTTER_CUTS) - 1):
        chunks = _chunks(lanes, cuts, p)
        off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
        outs += [np.array([mk.push(np.concatenate(chunks), off)])] + _state(mk)
        if p == hc.SPOTTER_RESET_AFTER:
            mk.reset(hc.SPOTTER_RESET_LANE)
    outs += [mk.counts()[0]]
    for lane in range(len(lanes)):
        outs += [np.array([mk.flush(lane)])] + list(mk.frames())
    return tuple(outs + list(mk.best()))


def _same_frames(got, want):
    lane, col, src, frame, cost, start = got
    assert list(zip(lane.tolist(), col.tolist(), src.tolist(), frame.tolist(), start.tolist())) == [
        (w[0], w[1], w[2], w[3], int(w[5])) for w in want]
    assert cost.view(np.uint64).tolist() == np.array([w[4] for w in want], dtype=np.float64).view(np.uint64).tolist()


def _same_best(got, refs):
    total, covered, committed = got
    want = [r.best() for r in refs]
    assert total.view(np.uint64).tolist() == np.array([w[0] for w in want]).view(np.uint64).tolist()
    assert covered.tolist() == [w[1] for w in want] and committed.tolist() == [w[2] for w in want]


def _lane(D):
    return ref.Lane([np.asarray(a, dtype=np.float64).reshape(-1, D.dim) for a in D["src"]], D.dim, PENALTY, GAP)


def check_mosaicker(oracle, probe, D, out):
    """tests/live_mosaic_ref.py, lane by lane: every push's and flush's frames and the state after them, bit for bit."""
    lanes = D["tgt"]
    refs = [_lane(D) for _ in lanes]
    cuts = [hc.spotter_cuts(x.shape[0]) for x in lanes]
    at = emitted = 0
    for p in range(len(hc.SPOTTER_CUTS) - 1):
        want = [(l, *f) for l, (r, c) in enumerate(zip(refs, _chunks(lanes, cuts, p))) for f in r.push(c)]
        assert out[at][0] == len(want)
        _same_frames(out[at + 1:at + 7], want)
        _same_best(out[at + 7:at + 10], refs)
        emitted += len(want)
        at += 10
        if p == hc.SPOTTER_RESET_AFTER:
            refs[hc.SPOTTER_RESET_LANE] = _lane(D)
    assert out[at].tolist() == [r.n for r in refs]
    at += 1
    for l, r in enumerate(refs):
        want = [(l, *f) for f in r.flush()]
        assert out[at][0] == len(want)
        _same_frames(out[at + 1:at + 7], want)
        at += 7
    _same_best(out[at:at + 3], refs)
    assert at + 3 == len(out) and emitted > 40


def _follow(e, D, h):
    """A two-lane stream fed in the stream probe's pushes, followed by a mosaicker on a small dictionary."""
    lanes = D["snd"]
    g = D.variant.grow
    sf, so = D.flat("src", e.np_dtype)
    d = h.add(e.dictionary(sf, so, D.dim))
    st = h.add(e.stream(len(lanes), hc.RATE, D.dim))
    mk = h.add(e.mosaicker(d, len(lanes), PENALTY, GAP))
    cuts = [[min(c * g, x.size) for c in hc.STREAM_CUTS] + [x.size] for x in lanes]
    outs = []
    for p in range(len(hc.STREAM_CUTS)):
        chunks = [x[c[p]:c[p + 1]] for x, c in zip(lanes, cuts)]
        st.push(np.concatenate(chunks), np.concatenate([[0], np.cumsum([c.size for c in chunks])]))
        outs += [st.counts()[1], np.array([mk.follow(st)])] + _state(mk)
    outs += [st.read(l) for l in range(len(lanes))]
    for lane in range(len(lanes)):
        outs += [np.array([mk.flush(lane)])] + list(mk.frames())
    return tuple(outs)


def check_follow(oracle, probe, D, out):
    """The restatement pushed the frames the stream analysed (they are among the outputs)."""
    n_l, n_p = len(D["snd"]), len(hc.STREAM_CUTS)
    frames = out[11 * n_p:11 * n_p + n_l]
    refs = [_lane(D) for _ in range(n_l)]
    held = [0] * n_l
    for p in range(n_p):
        block = out[11 * p:11 * p + 11]
        now = [int(v) for v in block[0]]
        want = [(l, *f) for l, r in enumerate(refs) for f in r.push(frames[l][held[l]:now[l]])]
        held = now
        assert block[1][0] == len(want)
        _same_frames(block[2:8], want)
        _same_best(block[8:11], refs)
    assert held == [f.shape[0] for f in frames] and min(held) >= 15
    at = 11 * n_p + n_l
    for l, r in enumerate(refs):
        want = [(l, *f) for f in r.flush()]
        assert out[at][0] == len(want)
        _same_frames(out[at + 1:at + 7], want)
        at += 7
    assert at == len(out) and all(r.done + 1 == r.n for r in refs)


# dtw_search's sets (33 sources of 0 ... 64 frames; its 65 targets of up to 64 frames are the lanes) on the f64 dtw context
PROBE = hc.Probe(NAME, hc.DTW64, _mosaicker, ("ssym_mosaicker_push", "ssym_mosaicker_frames", "ssym_mosaicker_flush",
                                              "ssym_mosaicker_best", "ssym_mosaicker_reset"),
                 {"src": (hc.F, hc.SRC33), "tgt": (hc.F, hc.TGT65)}, 13, 0x4126, scale=hc._sigma(13), takes_dict=True)
# the stream probe's lanes, and three short recordings of MFCC-sized values to tile them with
PROBE_FOLLOW = hc.Probe(FOLLOW, hc.DTW64, _follow, ("ssym_mosaicker_follow",), {"snd": (hc.S, [6000, 5200]), "src": (hc.F, [5, 9, 1])},
                        12, 0x4426, scale=4.0, grow_dim=False)
for _probe, _check in ((PROBE, check_mosaicker), (PROBE_FOLLOW, check_follow)):
    hc.PROBES.setdefault(_probe.name, _probe)
    gh.CHECKS.setdefault(_probe.name, _check)
BOTH = [NAME, FOLLOW]


def test_the_probes_are_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_mosaicker
    assert hc.PROBES[FOLLOW] is PROBE_FOLLOW and gh.CHECKS[FOLLOW] is check_follow
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1] and PROBE_FOLLOW in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    assert {"ssym_mosaicker_create", "ssym_mosaicker_destroy", "ssym_mosaicker_counts"} <= hc.LIFECYCLE
    data = PROBE.data()
    assert len(data["src"]) == 33 and len(data["tgt"]) == 65


@pytest.mark.parametrize("name", BOTH)
def test_two_fresh_contexts_agree_bit_for_bit(fresh, name):  # noqa: F811
    gh.test_two_fresh_contexts_agree_bit_for_bit(fresh, name)


@pytest.mark.parametrize("name", BOTH)
def test_the_fresh_answer_is_the_references(oracle, fresh, name):  # noqa: F811
    gh.test_the_fresh_answer_is_the_references(oracle, fresh, name)


@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
@pytest.mark.parametrize("name", BOTH)
def test_the_dirty_answer_is_the_fresh_answer(fresh, name, prelude):  # noqa: F811
    gh.test_the_dirty_answer_is_the_fresh_answer(fresh, name, prelude)


def test_used_handles(fresh):  # noqa: F811
    gh.test_used_handles(fresh, NAME)


@pytest.mark.parametrize("other", ["mosaic", "coverer", "stream"])
def test_another_call_first(fresh, other):  # noqa: F811
    """The offline mosaic, a coverer and a stream with its spotter before the mosaicker, and after it."""
    if other not in hc.PROBES:
        import test_gpu_history_coverer  # noqa: F401  (these register their probes when this file runs alone)
        import test_gpu_history_mosaic  # noqa: F401
    for mine in (PROBE, PROBE_FOLLOW):
        gh.run_dirty(mine, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (mine.name, other))
        gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, mine, hc.PLAIN), fresh, "%s after %s" % (other, mine.name))
