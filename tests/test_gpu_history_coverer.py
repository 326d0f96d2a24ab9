"""The probes of the coverer for tests/test_gpu_history.py's property: ssym_coverer_* give the same bits on a context that ran
something else before as on a fresh one.

tests/test_history_cases.py asks for a probe of every compute entry point the header declares; a call added after
tests/history_cases.py was written brings its probe in a file of its own (tests/test_gpu_history_paced_match.py says how
that works): importing this module registers the probes in history_cases.PROBES, their reference checks in
test_gpu_history.CHECKS and the coverer's lifecycle calls in history_cases.LIFECYCLE, and the bodies of the parametrised
history tests are run here for these probes."""
import numpy as np
import pytest

import history_cases as hc
import live_cover_ref as ref
import test_gpu_history as gh
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME, FOLLOW = "coverer", "coverer_follow"
PENALTY = 2.0
hc.LIFECYCLE |= {"ssym_coverer_create", "ssym_coverer_destroy", "ssym_coverer_counts"}


def _state(cv):
    return list(cv.pieces()) + list(cv.best())


def _chunks(lanes, cuts, p):
    """Push p of every lane; the lane that was reset starts again with its whole recording in the last push."""
    last = p == len(hc.SPOTTER_CUTS) - 2
    return [x if last and l == hc.SPOTTER_RESET_LANE else x[c[p]:c[p + 1]] for l, (x, c) in enumerate(zip(lanes, cuts))]


def _coverer(e, D, h, dictionary=None):
    """Every target of the set as a lane of one coverer on the set's sources, cut by spotter_cuts; one lane is reset."""
    if dictionary is None:
        sf, so = D.flat("src", e.np_dtype)
        dictionary = h.add(e.dictionary(sf, so, D.dim))
    lanes = D["tgt"]
    cv = h.add(e.coverer(dictionary, len(lanes), PENALTY))
    cuts = [hc.spotter_cuts(x.shape[0], D.variant.grow) for x in lanes]
    outs = []
    for p in range(len(hc.SPOTTER_CUTS) - 1):
        chunks = _chunks(lanes, cuts, p)
        off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
        outs += [np.array([cv.push(np.concatenate(chunks), off)])] + _state(cv)
        if p == hc.SPOTTER_RESET_AFTER:
            cv.reset(hc.SPOTTER_RESET_LANE)
    outs += [cv.counts()[0], np.array([cv.counts()[1]])]
    for lane in range(len(lanes)):
        outs += [np.array([cv.flush(lane)])] + list(cv.pieces())
    return tuple(outs + list(cv.best()))


def _same_pieces(got, want):
    lane, src, start, end, cost = got
    assert list(zip(lane.tolist(), src.tolist(), start.tolist(), end.tolist())) == [w[:4] for w in want]
    assert cost.view(np.uint64).tolist() == np.array([w[4] for w in want], dtype=np.float64).view(np.uint64).tolist()


def _same_best(got, refs):
    total, covered, committed = got
    want = [r.state() for r in refs]
    assert total.view(np.uint64).tolist() == np.array([w[0] for w in want]).view(np.uint64).tolist()
    assert covered.tolist() == [w[1] for w in want] and committed.tolist() == [w[2] for w in want]


def check_coverer(oracle, probe, D, out):
    """tests/live_cover_ref.py, lane by lane: every push's and flush's pieces and the state after them, bit for bit."""
    lanes = D["tgt"]
    refs = [ref.Lane(D["src"], PENALTY) for _ in lanes]
    cuts = [hc.spotter_cuts(x.shape[0]) for x in lanes]
    at = 0
    for p in range(len(hc.SPOTTER_CUTS) - 1):
        want = [(l, *piece) for l, (r, c) in enumerate(zip(refs, _chunks(lanes, cuts, p))) for piece in r.push(c)]
        assert out[at][0] == len(want)
        _same_pieces(out[at + 1:at + 6], want)
        _same_best(out[at + 6:at + 9], refs)
        at += 9
        if p == hc.SPOTTER_RESET_AFTER:
            refs[hc.SPOTTER_RESET_LANE] = ref.Lane(D["src"], PENALTY)
    assert out[at].tolist() == [r.n for r in refs] and out[at + 1][0] == ref.BACK_MIN
    at += 2
    emitted = 0
    for l, r in enumerate(refs):
        want = [(l, *piece) for piece in r.flush()]
        assert out[at][0] == len(want)
        _same_pieces(out[at + 1:at + 6], want)
        at += 6
        emitted += len(r.emitted)
    _same_best(out[at:at + 3], refs)
    assert at + 3 == len(out) and emitted > 40


def _follow(e, D, h):
    """A two-lane stream fed in the stream probe's pushes, followed by a coverer on a small dictionary."""
    lanes = D["snd"]
    g = D.variant.grow
    sf, so = D.flat("src", e.np_dtype)
    d = h.add(e.dictionary(sf, so, D.dim))
    st = h.add(e.stream(len(lanes), hc.RATE, D.dim))
    cv = h.add(e.coverer(d, len(lanes), PENALTY))
    cuts = [[min(c * g, x.size) for c in hc.STREAM_CUTS] + [x.size] for x in lanes]
    outs = []
    for p in range(len(hc.STREAM_CUTS)):
        chunks = [x[c[p]:c[p + 1]] for x, c in zip(lanes, cuts)]
        st.push(np.concatenate(chunks), np.concatenate([[0], np.cumsum([c.size for c in chunks])]))
        outs += [st.counts()[1], np.array([cv.follow(st)])] + _state(cv)
    outs += [st.read(l) for l in range(len(lanes))]
    for lane in range(len(lanes)):
        outs += [np.array([cv.flush(lane)])] + list(cv.pieces())
    return tuple(outs)


def check_follow(oracle, probe, D, out):
    """The restatement pushed the frames the stream analysed (they are among the outputs)."""
    n_l, n_p = len(D["snd"]), len(hc.STREAM_CUTS)
    frames = out[10 * n_p:10 * n_p + n_l]
    refs = [ref.Lane(D["src"], PENALTY) for _ in range(n_l)]
    held = [0] * n_l
    for p in range(n_p):
        block = out[10 * p:10 * p + 10]
        now = [int(v) for v in block[0]]
        want = [(l, *piece) for l, r in enumerate(refs) for piece in r.push(frames[l][held[l]:now[l]])]
        held = now
        assert block[1][0] == len(want)
        _same_pieces(block[2:7], want)
        _same_best(block[7:10], refs)
    assert held == [f.shape[0] for f in frames] and min(held) >= 15
    at = 10 * n_p + n_l
    for l, r in enumerate(refs):
        want = [(l, *piece) for piece in r.flush()]
        assert out[at][0] == len(want)
        _same_pieces(out[at + 1:at + 6], want)
        at += 6
    assert at == len(out) and all(r.emitted for r in refs)


# dtw_search's sets (33 sources of 0 ... 64 frames; its 65 targets of up to 64 frames are the lanes) on the f64 dtw context
PROBE = hc.Probe(NAME, hc.DTW64, _coverer, ("ssym_coverer_push", "ssym_coverer_pieces", "ssym_coverer_flush", "ssym_coverer_best",
                                            "ssym_coverer_reset"),
                 {"src": (hc.F, hc.SRC33), "tgt": (hc.F, hc.TGT65)}, 13, 0x4101, scale=hc._sigma(13), takes_dict=True)
# the stream probe's lanes, and three short segments of MFCC-sized values to cover them with
PROBE_FOLLOW = hc.Probe(FOLLOW, hc.DTW64, _follow, ("ssym_coverer_follow",), {"snd": (hc.S, [6000, 5200]), "src": (hc.F, [5, 9, 1])},
                        12, 0x4409, scale=4.0, grow_dim=False)
for _probe, _check in ((PROBE, check_coverer), (PROBE_FOLLOW, check_follow)):
    hc.PROBES.setdefault(_probe.name, _probe)
    gh.CHECKS.setdefault(_probe.name, _check)
BOTH = [NAME, FOLLOW]


def test_the_probes_are_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_coverer
    assert hc.PROBES[FOLLOW] is PROBE_FOLLOW and gh.CHECKS[FOLLOW] is check_follow
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1] and PROBE_FOLLOW in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    assert {"ssym_coverer_create", "ssym_coverer_destroy", "ssym_coverer_counts"} <= hc.LIFECYCLE
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


@pytest.mark.parametrize("other", ["cover", "spotter_paced", "stream", "dtw_search"])
def test_another_call_first(fresh, other):  # noqa: F811
    """The offline cover, a paced spotter, a stream with its spotter and a search before the coverer, and after it."""
    if other not in hc.PROBES:
        import test_gpu_history_cover  # noqa: F401  (registers the cover's probe when this file runs alone)
    for mine in (PROBE, PROBE_FOLLOW):
        gh.run_dirty(mine, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (mine.name, other))
        gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, mine, hc.PLAIN), fresh, "%s after %s" % (other, mine.name))
