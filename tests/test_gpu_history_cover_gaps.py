"""The probe of the cover with gaps for tests/test_gpu_history.py's property: ssym_dtw_cover_gaps and a coverer made by
ssym_coverer_create_gaps give the same bits on a context that ran something else before as on a fresh one.

tests/test_history_cases.py asks for a probe of every compute entry point the header declares; a call added after
tests/history_cases.py was written brings its probe in a file of its own (tests/test_gpu_history_paced_match.py says how
that works): importing this module registers the probe in history_cases.PROBES and its reference check in
test_gpu_history.CHECKS, and the bodies of the parametrised history tests are run here for this probe."""
import numpy as np
import pytest

import cover_gaps_ref
import cover_ref
import history_cases as hc
import test_gpu_history as gh
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME = "cover_gaps"
CASES = ((0.0, 6.0), (2.0, 9.0), (0.0, float("inf")))       # (piece_penalty, gap_cost); a frame is about 7 from another
LIVE = (2.0, 6.0)                                         # the coverer's


def _cover_gaps(e, D, h, dictionary=None):
    """The cover with gaps of every target of the set, then every target as a lane of a coverer with gaps on the same
    dictionary: one push of everything, the flush of every lane."""
    d, q = hc._sets(e, D, h, dictionary)
    outs = [x for penalty, gap in CASES for x in e.dtw_cover(d, q, penalty, gap_cost=gap)]
    lanes = D["tgt"]
    cv = h.add(e.coverer(d, len(lanes), *LIVE))
    off = np.concatenate([[0], np.cumsum([x.shape[0] for x in lanes])])
    outs += [np.array([cv.push(np.concatenate(lanes), off)])] + list(cv.pieces()) + list(cv.best())
    for lane in range(len(lanes)):
        outs += [np.array([cv.flush(lane)])] + list(cv.pieces())
    return tuple(outs + list(cv.best()))


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def check_cover_gaps(oracle, probe, D, out):
    """tests/cover_gaps_ref.py: the six arrays of every call bit for bit; the coverer's pieces from push to flush are the
    offline cover's, lane by lane, and its totals are the offline totals."""
    tabs = cover_ref.all_tables(D["src"], D["tgt"])
    for k, (penalty, gap) in enumerate(CASES):
        want = cover_gaps_ref.arrays(D["src"], D["tgt"], penalty, gap, tabs=tabs)
        for got, w in zip(out[6 * k:6 * k + 6], want):
            assert got.dtype == w.dtype and np.array_equal(got.view(np.uint8), w.view(np.uint8))
    at = 6 * len(CASES)
    lanes = D["tgt"]
    want = [cover_gaps_ref.chain(*tabs[t], *LIVE) if tabs[t] is not None else ([], np.inf) for t in range(len(lanes))]
    emitted = [[] for _ in lanes]

    def take(block):
        lane, src, start, end, cost = block
        for k in range(lane.size):
            emitted[int(lane[k])].append((int(src[k]), int(start[k]), int(end[k]), float(cost[k])))
        return lane.size

    assert out[at][0] == take(out[at + 1:at + 6])
    total, covered, committed = out[at + 6:at + 9]
    assert _bits(total).tolist() == _bits([w[1] for w in want]).tolist()
    assert covered.tolist() == [x.shape[0] for x in lanes] and (committed <= covered).all()
    at += 9
    for lane in range(len(lanes)):
        assert out[at][0] == take(out[at + 1:at + 6]) and set(out[at + 1].tolist()) <= {lane}
        at += 6
    for got, (pieces, _) in zip(emitted, want):
        assert [p[:3] for p in got] == [p[:3] for p in pieces]
        assert _bits([p[3] for p in got]).tolist() == _bits([p[3] for p in pieces]).tolist()
    total, covered, committed = out[at:at + 3]
    assert at + 3 == len(out) and committed.tolist() == covered.tolist() == [x.shape[0] for x in lanes]


# dtw_search's sets (33 sources of 0 ... 64 frames, 65 targets of up to 64) on the f64 dtw context
PROBE = hc.Probe(NAME, hc.DTW64, _cover_gaps, ("ssym_dtw_cover_gaps", "ssym_coverer_create_gaps"),
                 {"src": (hc.F, hc.SRC33), "tgt": (hc.F, hc.TGT65)}, 13, 0x4101, scale=hc._sigma(13), takes_dict=True)
hc.PROBES.setdefault(NAME, PROBE)
gh.CHECKS.setdefault(NAME, check_cover_gaps)


def test_the_probe_is_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_cover_gaps
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    data = PROBE.data()
    assert len(data["src"]) == 33 and len(data["tgt"]) == 65
    # the gap costs leave some frames uncovered and cover others
    src = cover_gaps_ref.arrays(data["src"], data["tgt"], *CASES[0])[2]
    gaps = int((src == cover_gaps_ref.GAP).sum())
    assert 20 < gaps < int((src != cover_ref.NONE).sum()) - 20


def test_two_fresh_contexts_agree_bit_for_bit(fresh):  # noqa: F811
    gh.test_two_fresh_contexts_agree_bit_for_bit(fresh, NAME)


def test_the_fresh_answer_is_the_references(oracle, fresh):  # noqa: F811
    gh.test_the_fresh_answer_is_the_references(oracle, fresh, NAME)


@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
def test_the_dirty_answer_is_the_fresh_answer(fresh, prelude):  # noqa: F811
    gh.test_the_dirty_answer_is_the_fresh_answer(fresh, NAME, prelude)


def test_used_handles(fresh):  # noqa: F811
    gh.test_used_handles(fresh, NAME)


@pytest.mark.parametrize("other", ["cover", "coverer"])
def test_another_call_first(fresh, other):  # noqa: F811
    """The cover and the coverer without gaps before the ones with gaps, and after them."""
    if other not in hc.PROBES:
        import test_gpu_history_cover  # noqa: F401  (register the probes when this file runs alone)
        import test_gpu_history_coverer  # noqa: F401
    gh.run_dirty(PROBE, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (NAME, other))
    gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, PROBE, hc.PLAIN), fresh, "%s after %s" % (other, NAME))
