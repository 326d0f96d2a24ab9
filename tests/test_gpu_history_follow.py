"""The probe of envelope following for tests/test_gpu_history.py's property: ssym_follow_envelope gives the same bits on a
context that ran something else before as on a fresh one, and what runs after it gives what it gives on a fresh context.

tests/test_history_cases.py asks for a probe of every compute entry point the header declares; a call added after
tests/history_cases.py was written brings its probe in a file of its own (tests/test_gpu_history_paced_match.py says how
that works): importing this module registers the probe in history_cases.PROBES and its reference check in
test_gpu_history.CHECKS, and the bodies of the parametrised history tests are run here for this probe."""
import numpy as np
import pytest

import follow_ref
import history_cases as hc
import test_gpu_history as gh
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME = "follow"
GAINS = (8.0, 1.0, 2.0 ** 30)


def _follow(e, D, h):
    """Every reconstruction of the set against its reference at every max_gain: samples, conversion and gains; then the
    same from device memory into device memory."""
    import torch
    (y, off), (x, r_off) = D.samples("rec"), D.samples("ref")
    outs = [a for g in GAINS for a in e.follow_envelope(y, off, x, r_off, g, want_pcm32=True, want_gains=True)]
    dy = torch.from_numpy(y if y.size else np.zeros(1)).cuda()
    dev = e.follow_envelope(dy, off, torch.from_numpy(x if x.size else np.zeros(1)).cuda(), r_off, GAINS[0], True, True, on_device=True)
    return tuple(outs) + tuple(t.cpu().numpy() for t in dev)


def check_follow(oracle, probe, D, out):
    """tests/follow_ref.py: the three arrays of every call bit for bit."""
    (y, off), (x, r_off) = D.samples("rec"), D.samples("ref")
    for k, g in enumerate(GAINS + (GAINS[0],)):
        want = follow_ref.follow(y, off, x, r_off, g)
        for got, w in zip(out[3 * k:3 * k + 3], want):
            assert got.dtype == w.dtype and np.array_equal(got.view(np.uint8), w.view(np.uint8))
    assert len(out) == 3 * (len(GAINS) + 1)


# reconstructions around the gain kernel's block of 32 boundaries (7936 samples), the apply kernel's chunk and a hop; references
# of other lengths
PROBE = hc.Probe(NAME, hc.DTW64, _follow, ("ssym_follow_envelope",),
                 {"rec": (hc.S, [7937, 0, 4096, 1, 300]), "ref": (hc.S, [8000, 300, 4000, 1, 0])}, 1, 0x4529, grow_dim=False)
hc.PROBES.setdefault(NAME, PROBE)
gh.CHECKS.setdefault(NAME, check_follow)


def test_the_probe_is_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_follow
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    data = PROBE.data()
    (y, off), (x, r_off) = data.samples("rec"), data.samples("ref")
    g = follow_ref.follow(y, off, x, r_off, 8.0)[2]
    assert off.size == r_off.size == 6 and np.any((g > 0.0) & (g < 8.0)) and np.any(g == 0.0)


def test_two_fresh_contexts_agree_bit_for_bit(fresh):  # noqa: F811
    gh.test_two_fresh_contexts_agree_bit_for_bit(fresh, NAME)


def test_the_fresh_answer_is_the_references(oracle, fresh):  # noqa: F811
    gh.test_the_fresh_answer_is_the_references(oracle, fresh, NAME)


@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
def test_the_dirty_answer_is_the_fresh_answer(fresh, prelude):  # noqa: F811
    gh.test_the_dirty_answer_is_the_fresh_answer(fresh, NAME, prelude)


@pytest.mark.parametrize("other", ["reconstruct", "mosaic", "dtw_search", "dtw_begin_finish"])
def test_another_call_first_and_after(fresh, other):  # noqa: F811
    """The warp and the WSOLA (one probe), the mosaic and a match: before the follower, and after it, where each must
    return what it returns on a fresh context."""
    if other not in hc.PROBES:
        import test_gpu_history_mosaic  # noqa: F401  (it registers its probe when this file runs alone)
    gh.run_dirty(PROBE, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (NAME, other))
    gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, PROBE, hc.PLAIN), fresh, "%s after %s" % (other, NAME))
