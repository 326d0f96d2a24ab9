"""The probe of the cover for tests/test_gpu_history.py's property: ssym_dtw_cover gives the same bits on a context that ran
something else before as on a fresh one.

tests/test_history_cases.py asks for a probe of every compute entry point the header declares; a call added after
tests/history_cases.py was written brings its probe in a file of its own (tests/test_gpu_history_paced_match.py says how
that works): importing this module registers the probe in history_cases.PROBES and its reference check in
test_gpu_history.CHECKS, and the bodies of the parametrised history tests are run here for this probe."""
import numpy as np
import pytest

import cover_ref
import history_cases as hc
import test_gpu_history as gh
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME = "cover"
PENALTIES = (0.0, 2.0)


def _cover(e, D, h, dictionary=None):
    """The cover of every target of the set, without and with a penalty per piece."""
    d, q = hc._sets(e, D, h, dictionary)
    return tuple(x for penalty in PENALTIES for x in e.dtw_cover(d, q, penalty))


def check_cover(oracle, probe, D, out):
    """tests/cover_ref.py: counts, totals, the four piece arrays and their padding, bit for bit."""
    tabs = cover_ref.all_tables(D["src"], D["tgt"])
    for k, penalty in enumerate(PENALTIES):
        want = cover_ref.arrays(D["src"], D["tgt"], penalty, tabs=tabs)
        for got, w in zip(out[6 * k:6 * k + 6], want):
            assert got.dtype == w.dtype and np.array_equal(got.view(np.uint8), w.view(np.uint8))


# dtw_search's sets (33 sources of 0 ... 64 frames, 65 targets of up to 64) on the f64 dtw context
PROBE = hc.Probe(NAME, hc.DTW64, _cover, ("ssym_dtw_cover",), {"src": (hc.F, hc.SRC33), "tgt": (hc.F, hc.TGT65)}, 13, 0x4101,
                 scale=hc._sigma(13), takes_dict=True)
hc.PROBES.setdefault(NAME, PROBE)
gh.CHECKS.setdefault(NAME, check_cover)


def test_the_probe_is_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_cover
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    data = PROBE.data()
    assert len(data["src"]) == 33 and len(data["tgt"]) == 65
    count = cover_ref.arrays(data["src"], data["tgt"])[0]
    assert (count > 0).sum() > 40 and count.max() > 1


def test_two_fresh_contexts_agree_bit_for_bit(fresh):  # noqa: F811
    gh.test_two_fresh_contexts_agree_bit_for_bit(fresh, NAME)


def test_the_fresh_answer_is_the_references(oracle, fresh):  # noqa: F811
    gh.test_the_fresh_answer_is_the_references(oracle, fresh, NAME)


@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
def test_the_dirty_answer_is_the_fresh_answer(fresh, prelude):  # noqa: F811
    gh.test_the_dirty_answer_is_the_fresh_answer(fresh, NAME, prelude)


def test_used_handles(fresh):  # noqa: F811
    gh.test_used_handles(fresh, NAME)


@pytest.mark.parametrize("other", ["dtw_search", "align_paced", "spot_paced", "paced_match"])
def test_another_call_first(fresh, other):  # noqa: F811
    """A symmetric search, a paced alignment, a paced spot and the paced search before the cover, and after it."""
    if other not in hc.PROBES:
        import test_gpu_history_paced_match  # noqa: F401  (registers the paced search's probe when this file runs alone)
    gh.run_dirty(PROBE, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (NAME, other))
    gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, PROBE, hc.PLAIN), fresh, "%s after %s" % (other, NAME))
