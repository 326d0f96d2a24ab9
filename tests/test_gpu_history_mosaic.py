"""The probe of the mosaic for tests/test_gpu_history.py's property: ssym_dtw_mosaic gives the same bits on a context that ran
something else before as on a fresh one.

tests/test_history_cases.py asks for a probe of every compute entry point the header declares; a call added after
tests/history_cases.py was written brings its probe in a file of its own (tests/test_gpu_history_paced_match.py says how
that works): importing this module registers the probe in history_cases.PROBES and its reference check in
test_gpu_history.CHECKS, and the bodies of the parametrised history tests are run here for this probe."""
import numpy as np
import pytest

import history_cases as hc
import mosaic_ref
import test_gpu_history as gh
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME = "mosaic"
# (piece_penalty, gap_cost); a frame is about 7 from another frame, and about 3.5 from the nearest of the dictionary's 1000
CASES = ((0.0, float("inf")), (2.0, 3.5), (20.0, 9.0))


def _mosaic(e, D, h, dictionary=None):
    """The mosaic of every target of the set at every case."""
    d, q = hc._sets(e, D, h, dictionary)
    return tuple(x for penalty, gap in CASES for x in e.dtw_mosaic(d, q, penalty, gap))


def check_mosaic(oracle, probe, D, out):
    """tests/mosaic_ref.py: the six arrays of every call bit for bit."""
    for k, (penalty, gap) in enumerate(CASES):
        want = mosaic_ref.arrays(D["src"], D["tgt"], penalty, gap)
        for got, w in zip(out[6 * k:6 * k + 6], want):
            assert got.dtype == w.dtype and np.array_equal(got.view(np.uint8), w.view(np.uint8))
    assert len(out) == 6 * len(CASES)


# dtw_search's sets (33 sources of 0 ... 64 frames, 65 targets of up to 64) on the f64 dtw context
PROBE = hc.Probe(NAME, hc.DTW64, _mosaic, ("ssym_dtw_mosaic",),
                 {"src": (hc.F, hc.SRC33), "tgt": (hc.F, hc.TGT65)}, 13, 0x305A, scale=hc._sigma(13), takes_dict=True)
hc.PROBES.setdefault(NAME, PROBE)
gh.CHECKS.setdefault(NAME, check_mosaic)


def test_the_probe_is_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_mosaic
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    data = PROBE.data()
    assert len(data["src"]) == 33 and len(data["tgt"]) == 65
    # the middle case leaves some frames uncovered and covers others
    src = mosaic_ref.arrays(data["src"], data["tgt"], *CASES[1])[3]
    gaps = int((src == mosaic_ref.GAP).sum())
    assert 20 < gaps < int((src != mosaic_ref.NONE).sum()) - 20


def test_two_fresh_contexts_agree_bit_for_bit(fresh):  # noqa: F811
    gh.test_two_fresh_contexts_agree_bit_for_bit(fresh, NAME)


def test_the_fresh_answer_is_the_references(oracle, fresh):  # noqa: F811
    gh.test_the_fresh_answer_is_the_references(oracle, fresh, NAME)


@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
def test_the_dirty_answer_is_the_fresh_answer(fresh, prelude):  # noqa: F811
    gh.test_the_dirty_answer_is_the_fresh_answer(fresh, NAME, prelude)


def test_used_handles(fresh):  # noqa: F811
    gh.test_used_handles(fresh, NAME)


def test_the_cover_first_and_after(fresh):  # noqa: F811
    """The cover with gaps, which shares the chain's gap step and none of the scratch, before the mosaic and after it."""
    if "cover_gaps" not in hc.PROBES:
        import test_gpu_history_cover_gaps  # noqa: F401  (register the probe when this file runs alone)
    other = hc.PROBES["cover_gaps"]
    gh.run_dirty(PROBE, lambda e: hc.dirty_run(e, other, hc.PLAIN), fresh, "%s after cover_gaps" % NAME)
    gh.run_dirty(other, lambda e: hc.dirty_run(e, PROBE, hc.PLAIN), fresh, "cover_gaps after %s" % NAME)
