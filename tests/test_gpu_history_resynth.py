"""The probes of the resynthesiser for tests/test_gpu_history.py's property: ssym_resynth_* give the same bits on a context that
ran something else before as on a fresh one.

tests/test_history_cases.py asks for a probe of every compute entry point the header declares; a call added after
tests/history_cases.py was written brings its probe in a file of its own (tests/test_gpu_history_paced_match.py says how
that works): importing this module registers the probes in history_cases.PROBES, their reference checks in
test_gpu_history.CHECKS and the resynthesiser's lifecycle calls in history_cases.LIFECYCLE, and the bodies of the
parametrised history tests are run here for these probes."""
import numpy as np
import pytest

import history_cases as hc
import live_resynth_ref as ref
import test_gpu_history as gh
from live_resynth_ref import GAP, HOP, NO_MATCH
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)
from warp_ref import pcm32

pytestmark = pytest.mark.gpu

NAME, TAKE = "resynth", "resynth_take"
SEARCHES = (0, 40)
LANES, RESET_LANE, RESET_AFTER = 3, 1, 1
CUTS = (0, 1, 9)                    # pushes of 1 frame, of 8 and of the rest
PENALTY, GAP_COST = 2.0, 9.0
hc.LIFECYCLE |= {"ssym_resynth_create", "ssym_resynth_destroy", "ssym_resynth_counts"}


def _rows(D):
    """Per lane, (src, frame, start) rows on the first three sounds of the set: tiles of 1 ... 9 frames on paced maps that
    start anywhere up to two hops beyond their recording, and gap runs."""
    out = []
    for l in range(LANES):
        rng = np.random.default_rng(0x5E7 + l)
        rows = []
        for t in range(5):
            src = int(rng.integers(0, 3))
            fmap, prev = [int(rng.integers(0, D["snd"][src].size // HOP + 3))], 1
            for _ in range(int(rng.integers(0, 9))):
                prev = int(rng.integers(0 if prev else 1, 3))
                fmap.append(fmap[-1] + prev)
            rows += [(src, f, int(j == 0)) for j, f in enumerate(fmap)]
            rows += [(GAP, NO_MATCH, 1)] * int(rng.integers(0, 3))
        out.append(rows)
    return out


def _pushes(rows):
    """Per push {lane: rows}; the lane that was reset starts again with all its rows in the last push."""
    cuts = [list(CUTS) + [len(r)] for r in rows]
    last = len(CUTS) - 1
    return [{l: (r if p == last and l == RESET_LANE else r[c[p]:c[p + 1]]) for l, (r, c) in enumerate(zip(rows, cuts))}
            for p in range(len(CUTS))]


def _arrays(by_lane, at):
    cols = [[], [], [], [], []]
    for l in sorted(by_lane):
        for j, (src, frame, start) in enumerate(by_lane[l]):
            for a, v in zip(cols, (l, at[l] + j, src, frame, start)):
                a.append(v)
    return [np.array(a, dtype=np.uint32) for a in cols]


def _total(rows, l):
    return len(rows) * HOP + (0, 300, 1023)[l % 3]


def _resynth(e, D, h):
    """Three lanes pushed in three cuts on the plain warp and on a search; one lane is reset; every lane flushed."""
    x, off = D.samples("snd")
    smp = h.add(e.samples(x, off))
    rows = _rows(D)
    outs = []
    for search in SEARCHES:
        rs = h.add(e.resynth(smp, LANES, search))
        at = {l: 0 for l in range(LANES)}
        for p, by_lane in enumerate(_pushes(rows)):
            outs += [np.array([rs.push(*_arrays(by_lane, at))])] + list(rs.samples(want_pcm32=True))
            for l, r in by_lane.items():
                at[l] += len(r)
            if p == RESET_AFTER:
                rs.reset(RESET_LANE)
                at[RESET_LANE] = 0
        outs += list(rs.counts())
        for l in range(LANES):
            outs += [np.array([rs.flush(l, _total(rows[l], l))])] + list(rs.samples(want_pcm32=True))
    return tuple(outs)


def _same_block(block, want):
    """(count, lane offsets, samples, pcm) of one call against the restatement's samples per lane."""
    n, off, smp, pcm = block
    sizes = [w.size for w in want]
    assert n[0] == sum(sizes) and off.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    flat = np.concatenate(want) if want else np.zeros(0)
    assert np.array_equal(np.asarray(smp, dtype=np.float64).view(np.uint64), flat.view(np.uint64))
    assert np.array_equal(pcm, pcm32(flat))


def check_resynth(oracle, probe, D, out):
    """tests/live_resynth_ref.py, lane by lane: every push's and flush's samples, bit for bit."""
    rows, at, released = _rows(D), 0, 0
    for search in SEARCHES:
        cache = {}
        refs = [ref.LiveResynth(D["snd"], search, None, cache) for _ in range(LANES)]
        for p, by_lane in enumerate(_pushes(rows)):
            want = [refs[l].push(by_lane[l]) for l in range(LANES)]
            _same_block(out[at:at + 4], want)
            released += sum(w.size for w in want)
            at += 4
            if p == RESET_AFTER:
                refs[RESET_LANE] = ref.LiveResynth(D["snd"], search, None, cache)
        assert out[at].tolist() == [r.n for r in refs] and out[at + 1].tolist() == [r.released * HOP for r in refs]
        at += 2
        for l in range(LANES):
            want = [refs[k].flush(_total(rows[l], l)) if k == l else np.zeros(0) for k in range(LANES)]
            _same_block(out[at:at + 4], want)
            at += 4
    assert at == len(out) and released > 20 * HOP


def _take(e, D, h):
    """A mosaicker on a small dictionary pushed in three cuts; a resynthesiser takes every frame log device to device."""
    sf, so = D.flat("src", e.np_dtype)
    d = h.add(e.dictionary(sf, so, D.dim))
    x, off = D.samples("snd")
    smp = h.add(e.samples(x, off))
    lanes = D["tgt"]
    mk = h.add(e.mosaicker(d, len(lanes), PENALTY, GAP_COST))
    rs = h.add(e.resynth(smp, len(lanes), SEARCHES[1]))
    cuts = [list(CUTS) + [t.shape[0]] for t in lanes]
    outs = []
    for p in range(len(CUTS)):
        chunks = [t[c[p]:c[p + 1]] for t, c in zip(lanes, cuts)]
        mk.push(np.concatenate(chunks), np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])]))
        outs += list(mk.frames()) + [np.array([rs.take(mk)])] + list(rs.samples(want_pcm32=True))
    for l, t in enumerate(lanes):
        mk.flush(l)
        outs += list(mk.frames()) + [np.array([rs.take(mk)])] + list(rs.samples(want_pcm32=True))
        outs += [np.array([rs.flush(l, t.shape[0] * HOP + 100)])] + list(rs.samples(want_pcm32=True))
    return tuple(outs)


def check_take(oracle, probe, D, out):
    """The restatement pushed the frames the mosaicker logged (they are among the outputs)."""
    n_l = len(D["tgt"])
    refs = [ref.LiveResynth(D["snd"], SEARCHES[1], None, {}) for _ in range(n_l)]
    at, frames = 0, 0

    def taken(block):
        lane, col, src, frame, cost, start = block[:6]
        want = []
        for l, r in enumerate(refs):
            k = np.flatnonzero(lane == l)
            assert col[k].tolist() == list(range(r.n, r.n + k.size))
            want.append(r.push(list(zip(src[k].tolist(), frame[k].tolist(), start[k].tolist()))) if k.size else np.zeros(0))
        _same_block(block[6:10], want)
        return lane.size

    for p in range(len(CUTS)):
        frames += taken(out[at:at + 10])
        at += 10
    for l, t in enumerate(D["tgt"]):
        frames += taken(out[at:at + 10])
        at += 10
        want = [refs[k].flush(t.shape[0] * HOP + 100) if k == l else np.zeros(0) for k in range(n_l)]
        _same_block(out[at:at + 4], want)
        at += 4
    assert at == len(out) and frames == sum(t.shape[0] for t in D["tgt"])


PROBE = hc.Probe(NAME, hc.DTW64, _resynth, ("ssym_resynth_push", "ssym_resynth_samples", "ssym_resynth_flush", "ssym_resynth_reset"),
                 {"snd": (hc.S, [5000, 2600, 1])}, 1, 0x4527, grow_dim=False)
# three short recordings of MFCC-sized values with samples to play them from, and two targets to tile
PROBE_TAKE = hc.Probe(TAKE, hc.DTW64, _take, ("ssym_resynth_take",),
                      {"snd": (hc.S, [1500, 2500, 300]), "src": (hc.F, [5, 9, 1]), "tgt": (hc.F, [23, 14])}, 12, 0x4528, scale=4.0,
                      grow_dim=False)
for _probe, _check in ((PROBE, check_resynth), (PROBE_TAKE, check_take)):
    hc.PROBES.setdefault(_probe.name, _probe)
    gh.CHECKS.setdefault(_probe.name, _check)
BOTH = [NAME, TAKE]


def test_the_probes_are_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_resynth
    assert hc.PROBES[TAKE] is PROBE_TAKE and gh.CHECKS[TAKE] is check_take
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1] and PROBE_TAKE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    assert {"ssym_resynth_create", "ssym_resynth_destroy", "ssym_resynth_counts"} <= hc.LIFECYCLE
    assert [len(r) > CUTS[-1] for r in _rows(PROBE.data())] == [True] * LANES


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


@pytest.mark.parametrize("other", ["reconstruct", "mosaicker", "stream"])
def test_another_call_first(fresh, other):  # noqa: F811
    """The offline resynthesis, a mosaicker and a stream with its spotter before the resynthesiser, and after it."""
    if other not in hc.PROBES:
        import test_gpu_history_mosaicker  # noqa: F401  (it registers its probes when this file runs alone)
    for mine in (PROBE, PROBE_TAKE):
        gh.run_dirty(mine, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (mine.name, other))
        gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, mine, hc.PLAIN), fresh, "%s after %s" % (other, mine.name))
