"""The probe of the live envelope follower for tests/test_gpu_history.py's property: ssym_follower_* give the same bits on a
context that ran something else before -- or between the follower's own calls -- as on a fresh one.

tests/test_history_cases.py asks for a probe of every compute entry point the header declares; a call added after
tests/history_cases.py was written brings its probe in a file of its own (tests/test_gpu_history_paced_match.py says how
that works): importing this module registers the probe in history_cases.PROBES, its reference check in
test_gpu_history.CHECKS and the follower's lifecycle calls in history_cases.LIFECYCLE, and the bodies of the parametrised
history tests are run here for this probe."""
import numpy as np
import pytest

import history_cases as hc
import live_follow_ref as lf
import test_gpu_history as gh
from follow_ref import pcm32
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME = "follower"
MAX_GAIN = 8.0
RESET_LANE, RESET_AFTER = 1, 1
Y_CUTS, X_CUTS = (0, 300, 2900), (0, 700, 2500)     # three pushes: the first below two hops of one signal, the rest at the end
hc.LIFECYCLE |= {"ssym_follower_create", "ssym_follower_destroy", "ssym_follower_counts"}


def _lanes(D):
    (y, off), (x, r_off) = D.samples("rec"), D.samples("ref")
    return [(y[int(a):int(b)], x[int(c):int(d)]) for a, b, c, d in zip(off[:-1], off[1:], r_off[:-1], r_off[1:])]


def _pushes(lanes):
    """Per push, per lane (new y, new x); the lane that was reset starts again with everything in the last push."""
    out = []
    for p in range(len(Y_CUTS)):
        ya, yb = Y_CUTS[p], Y_CUTS[p + 1] if p + 1 < len(Y_CUTS) else None
        xa, xb = X_CUTS[p], X_CUTS[p + 1] if p + 1 < len(X_CUTS) else None
        last = p == len(Y_CUTS) - 1
        out.append([(y, x) if last and l == RESET_LANE else (y[ya:yb], x[xa:xb]) for l, (y, x) in enumerate(lanes)])
    return out


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([a.size for a in parts])]).astype(np.uint64)


def _follower(e, D, h, between=None):
    """Every reconstruction of the set on a lane of its own against its reference, pushed in three cuts; one lane is reset;
    every lane flushed.  between: called after every call of the follower (the history tests put other calls there)."""
    lanes = _lanes(D)
    fl = h.add(e.follower(len(lanes), MAX_GAIN))
    outs = []

    def block(n):
        outs.extend([np.array([n])] + list(fl.samples(want_pcm32=True, want_gains=True)))
        if between is not None:
            between()
    for p, new in enumerate(_pushes(lanes)):
        ys, xs = [a for a, _ in new], [b for _, b in new]
        block(fl.push(np.concatenate(ys), _offsets(ys), np.concatenate(xs), _offsets(xs)))
        if p == RESET_AFTER:
            fl.reset(RESET_LANE)
    outs += list(fl.counts())
    for l in range(len(lanes)):
        block(fl.flush(l))
    return tuple(outs)


def _same_block(block, want):
    """(count, lane offsets, samples, pcm, gain offsets, gains) of one call against the restatement's (samples, gains) per lane."""
    n, off, smp, pcm, g_off, g = block
    assert n[0] == sum(o.size for o, _ in want)
    assert off.tolist() == _offsets([o for o, _ in want]).tolist() and g_off.tolist() == _offsets([q for _, q in want]).tolist()
    flat, gains = np.concatenate([o for o, _ in want]), np.concatenate([q for _, q in want])
    assert np.array_equal(np.asarray(smp, dtype=np.float64).view(np.uint64), flat.view(np.uint64))
    assert np.array_equal(pcm, pcm32(flat))
    assert np.array_equal(np.asarray(g, dtype=np.float64).view(np.uint64), gains.view(np.uint64))


def check_follower(oracle, probe, D, out):
    """tests/live_follow_ref.py: every push's and flush's samples, conversion and gains, bit for bit."""
    lanes = _lanes(D)
    ref = lf.LiveFollower(len(lanes), MAX_GAIN)
    at = released = 0
    for p, new in enumerate(_pushes(lanes)):
        want = ref.push([a for a, _ in new], [b for _, b in new])
        _same_block(out[at:at + 6], want)
        released += sum(o.size for o, _ in want)
        at += 6
        if p == RESET_AFTER:
            ref.reset(RESET_LANE)
    assert [a.tolist() for a in out[at:at + 3]] == [list(c) for c in ref.counts()]
    at += 3
    empty = (np.zeros(0), np.zeros(0))
    for l in range(len(lanes)):
        want = [ref.flush(k) if k == l else empty for k in range(len(lanes))]
        _same_block(out[at:at + 6], want)
        at += 6
    assert at == len(out) and released > 20 * lf.HOP


# reconstructions around the gain kernel's block of 32 boundaries (7936 samples), the apply kernel's chunk and a hop; references
# of other lengths
PROBE = hc.Probe(NAME, hc.DTW64, _follower, ("ssym_follower_push", "ssym_follower_flush", "ssym_follower_samples", "ssym_follower_reset"),
                 {"rec": (hc.S, [7937, 0, 4096, 1, 300]), "ref": (hc.S, [8000, 300, 4000, 1, 0])}, 1, 0x452A, grow_dim=False)
hc.PROBES.setdefault(NAME, PROBE)
gh.CHECKS.setdefault(NAME, check_follower)


def test_the_probe_is_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_follower
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    assert {"ssym_follower_create", "ssym_follower_destroy", "ssym_follower_counts"} <= hc.LIFECYCLE
    lanes = _lanes(PROBE.data())
    assert len(lanes) == 5 and lanes[RESET_LANE][1].size > 0


def test_two_fresh_contexts_agree_bit_for_bit(fresh):  # noqa: F811
    gh.test_two_fresh_contexts_agree_bit_for_bit(fresh, NAME)


def test_the_fresh_answer_is_the_references(oracle, fresh):  # noqa: F811
    gh.test_the_fresh_answer_is_the_references(oracle, fresh, NAME)


@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
def test_the_dirty_answer_is_the_fresh_answer(fresh, prelude):  # noqa: F811
    gh.test_the_dirty_answer_is_the_fresh_answer(fresh, NAME, prelude)


def _others():
    for name in ("follow", "resynth"):
        if name not in hc.PROBES:
            import test_gpu_history_follow  # noqa: F401  (they register their probes when this file runs alone)
            import test_gpu_history_resynth  # noqa: F401
    return ["dtw_search", "follow", "resynth"]


@pytest.mark.parametrize("other", ["dtw_search", "follow", "resynth"])
def test_another_call_first_and_after(fresh, other):  # noqa: F811
    """The search, ssym_follow_envelope and a resynthesiser: before the follower, and after it, where each must return what
    it returns on a fresh context."""
    assert other in _others()
    gh.run_dirty(PROBE, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (NAME, other))
    gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, PROBE, hc.PLAIN), fresh, "%s after %s" % (other, NAME))


@pytest.mark.parametrize("other", ["dtw_search", "follow", "resynth"])
def test_another_call_between_the_followers_calls(fresh, other):  # noqa: F811
    """The same calls on the same context after every push and flush of the follower: its rings, its records and its logs
    are its own, and what the context's scratch holds in between is nothing to it."""
    assert other in _others()
    want, _ = fresh(NAME)
    e = hc.new_engine(PROBE.ctx)
    try:
        got, _ = PROBE.run(e, between=lambda: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN))
    finally:
        e.close()
    gh.assert_same_outputs(got, want, "%s with %s between its calls" % (NAME, other))
