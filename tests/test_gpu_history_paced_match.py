"""The probe of paced matching for tests/test_gpu_history.py's property: ssym_match_queries_step and ssym_pair_matrix_step
give the same bits on a context that ran something else before as on a fresh one.

tests/history_cases.py lists the probes of the calls that existed when it was written, and tests/test_history_cases.py
asks for a probe of every compute entry point the header declares.  A call added later brings its probe in a file of its
own, as here: importing this module registers the probe in history_cases.PROBES and its reference check in
test_gpu_history.CHECKS (pytest imports every test module before it runs a test, so tests/test_history_cases.py sees the
probe whenever the suite is collected as a whole; run on its own it reports the two calls as unprobed).  The tests of
tests/test_gpu_history.py that are parametrised over the probes were parametrised before this module is imported, so
their bodies are run here for this probe: fresh against fresh, the reference, every prelude, a used dictionary.  The
gauntlet reads the probe list when it runs and includes it."""
import numpy as np
import pytest

import history_cases as hc
import paced_match_ref
import test_gpu_history as gh
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME = "paced_match"


def _paced_match(e, D, h, dictionary=None):
    """The search and the cost matrix under the paced step pattern, without and with distances (and an index base)."""
    d, q = hc._sets(e, D, h, dictionary)
    idx, cost = e.match(d, q, step="paced")
    idx2, cost2 = e.match(d, q, hc._edge_distances(q.n, 0.0, 60.0, 1e6), index_base=3, step="paced")
    return (idx, cost, idx2, cost2, e.pair_matrix(d, q, step="paced"))


def check_paced_match(oracle, probe, D, out):
    """tests/paced_match_ref.py: the matrix bit for bit, both folds."""
    want = paced_match_ref.matrix(D["src"], D["tgt"])
    assert np.array_equal(out[4].view(np.uint64), want.view(np.uint64))
    for k, (dist, base) in enumerate(((None, 0), (hc._edge_distances(len(D["tgt"]), 0.0, 60.0, 1e6), 3))):
        wi, wc = paced_match_ref.fold(want, dist, base)
        assert np.array_equal(out[2 * k], wi) and np.array_equal(out[2 * k + 1].view(np.uint64), wc.view(np.uint64))


# dtw_search's sets (33 sources of 0 ... 64 frames, 65 targets of up to 64) on the f64 dtw context
PROBE = hc.Probe(NAME, hc.DTW64, _paced_match, ("ssym_match_queries_step", "ssym_pair_matrix_step"),
                 {"src": (hc.F, hc.SRC33), "tgt": (hc.F, hc.TGT65)}, 13, 0x4101, scale=hc._sigma(13), takes_dict=True)
hc.PROBES.setdefault(NAME, PROBE)
gh.CHECKS.setdefault(NAME, check_paced_match)


def test_the_probe_is_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_paced_match
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    data = PROBE.data()
    assert len(data["src"]) == 33 and len(data["tgt"]) == 65 and np.isfinite(paced_match_ref.matrix(data["src"], data["tgt"])).sum() > 500


def test_two_fresh_contexts_agree_bit_for_bit(fresh):  # noqa: F811
    gh.test_two_fresh_contexts_agree_bit_for_bit(fresh, NAME)


def test_the_fresh_answer_is_the_references(oracle, fresh):  # noqa: F811
    gh.test_the_fresh_answer_is_the_references(oracle, fresh, NAME)


@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
def test_the_dirty_answer_is_the_fresh_answer(fresh, prelude):  # noqa: F811
    gh.test_the_dirty_answer_is_the_fresh_answer(fresh, NAME, prelude)


def test_used_handles(fresh):  # noqa: F811
    gh.test_used_handles(fresh, NAME)


@pytest.mark.parametrize("other", ["dtw_search", "align_paced", "spot_paced", "dtw_pair_matrix"])
def test_another_call_first(fresh, other):  # noqa: F811
    """A symmetric search, a paced alignment, a paced spot and the symmetric matrix before the paced search, and after it."""
    gh.run_dirty(PROBE, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (NAME, other))
    gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, PROBE, hc.PLAIN), fresh, "%s after %s" % (other, NAME))
