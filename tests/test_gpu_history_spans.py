"""The probe of the span calls for tests/test_gpu_history.py's property: ssym_dtw_align_spans, its sizes call and the two
window reconstructions give the same bits on a context that ran something else before as on a fresh one.

As tests/test_gpu_history_paced_match.py: importing this module registers the probe in history_cases.PROBES and its
reference check in test_gpu_history.CHECKS, and the bodies of the tests that were parametrised before this module was
imported are run here for this probe.  The probe's spans and windows are functions of the lengths alone, so the hostile
twins and the larger preludes (other lengths, other values per frame) run the same calls on their own data."""
import numpy as np
import pytest

import history_cases as hc
import span_ref
import test_gpu_history as gh
from test_gpu_history import fresh  # noqa: F401  (the module-scoped fixture, one per module that uses it)

pytestmark = pytest.mark.gpu

NAME = "spans"
NO = span_ref.NO_MATCH
SPAN_SRC, SPAN_TGT = [300, 70, 1, 257], [33, 64, 1, 256]       # (257 frames against 256: the slab)
SPAN_SND, SPAN_OUT = [5000, 1023, 2600, 1], [2500, 1500, 3100, 700]
SEARCH = 40


def spans_of(lengths, tgt_lengths):
    """(src, tgt, first, last) of the probe's pairs: per source a span in its middle against its own target, the whole of
    it against the same target, and one pair without a span."""
    src, tgt, first, last = [], [], [], []
    for s, (fa, fb) in enumerate(zip(lengths, tgt_lengths)):
        a = fa // 5
        b = min(a + max(fb, 1) + fa // 7, fa - 1)
        for lo, hi in ((a, b), (0, fa - 1)):
            src.append(s), tgt.append(s), first.append(lo), last.append(hi)
    src.append(0), tgt.append(0), first.append(NO), last.append(NO)
    return tuple(np.array(x, dtype=np.uint32) for x in (src, tgt, first, last))


def windows_of(lengths):
    """(first, len) per target, target t reading sound RECON_IDX-like t % sounds: a window in the middle, to the end, empty."""
    n = len(lengths)
    first = np.array([lengths[t] // 3 for t in range(n)], dtype=np.uint64)
    length = np.array([(lengths[t] - lengths[t] // 3) // (1 + t % 2) if t % 4 != 3 else 0 for t in range(n)], dtype=np.uint64)
    return first, length


def recon_args(D):
    sounds, out_len = D.lengths["snd"], D.lengths["out"]
    n = len(out_len)
    idx = np.array([t % len(sounds) for t in range(n)], dtype=np.uint32)
    first, length = windows_of([sounds[int(i)] for i in idx])
    rng = np.random.default_rng(0x3A96 + sum(out_len))
    ooff = np.concatenate([[0], np.cumsum(out_len)]).astype(np.uint64)
    frames = np.array([max(o // hc.HOP, 1) for o in out_len], dtype=np.uint32)
    moff = np.concatenate([[0], np.cumsum(frames + 1)]).astype(np.uint64)
    maps = np.zeros(int(moff[-1]), dtype=np.uint32)
    for t, f in enumerate(frames):
        w_frames = int(length[t]) // hc.HOP + 2
        base = np.arange(f) * w_frames // max(int(f), 1)
        maps[int(moff[t]):int(moff[t]) + f] = np.clip(base + rng.integers(-1, 2, size=f), 0, w_frames)
    pair_len = frames.copy()
    pair_len[1 % n] = 0
    return idx, first, length, ooff, maps, moff, frames, pair_len


def _flat(paths, maps):
    return (np.concatenate([np.zeros((0, 2), dtype=np.uint32)] + [np.asarray(x).reshape(-1, 2) for x in paths]),
            np.concatenate([np.zeros(0, dtype=np.uint32)] + [np.asarray(x).reshape(-1) for x in maps]))


def _spans(e, D, h):
    d, q = hc._sets(e, D, h)
    src, tgt, first, last = spans_of(D.lengths["src"], D.lengths["tgt"])
    outs = list(e.dtw_align_sizes(d, q, src, tgt, spans=(first, last)))
    for step in ("symmetric", "paced"):
        cost, length, paths, maps = e.dtw_align(d, q, src, tgt, step=step, spans=(first, last))
        outs += [cost, length] + list(_flat(paths, maps))
    x, off = D.samples("snd")
    smp = h.add(e.samples(x, off))
    idx, wf, wl, ooff, maps, moff, frames, pair_len = recon_args(D)
    w, wpcm = e.reconstruct_warped(smp, idx, ooff, maps, moff, frames, pair_len, want_pcm32=True, windows=(wf, wl))
    s, spcm, pos = e.reconstruct_wsola(smp, idx, ooff, maps, moff, frames, pair_len, search=SEARCH, want_pcm32=True,
                                       want_pos=True, windows=(wf, wl))
    return tuple(outs) + (w, wpcm, s, spcm, pos)


def check_spans(oracle, probe, D, out):
    """tests/span_ref.py: sizes, both alignments and both reconstructions, bit for bit."""
    import dtw_path_ref
    import warp_ref
    src, tgt, first, last = spans_of(D.lengths["src"], D.lengths["tgt"])
    spans = [(int(s), int(a), int(b)) for s, a, b in zip(np.where(first == NO, NO, src), first, last)]
    segs, tgts = [D["src"][int(s)] for s in src], [D["tgt"][int(t)] for t in tgt]
    p_off, m_off = span_ref.sizes([len(t) for t in tgts], spans)
    assert np.array_equal(out[0], p_off) and np.array_equal(out[1], m_off)
    for k, step in enumerate(("symmetric", "paced")):
        cost, length, paths, maps = out[2 + 4 * k:6 + 4 * k]
        want = span_ref.align_spans(segs, tgts, spans, step)
        assert dtw_path_ref.same_floats(cost, np.array([w[0] for w in want])), step
        assert np.array_equal(length, [len(w[1]) for w in want]), step
        assert np.array_equal(paths.astype(np.int64), np.concatenate([w[1] for w in want])), step
        assert np.array_equal(maps.astype(np.int64), np.concatenate([w[2] for w in want])), step
    assert np.isfinite(out[2]).sum() == len(spans) - 1 and 2 <= np.isfinite(out[6]).sum() < len(spans) - 1
    w, wpcm, s, spcm, pos = out[10:]
    idx, wf, wl, ooff, maps, moff, frames, pair_len = recon_args(D)
    bits = lambda v: np.asarray(v, dtype=np.float64).view(np.uint64)
    assert np.array_equal(bits(w), bits(span_ref.warp_spans(D["snd"], idx, wf, wl, ooff, maps, moff, frames, pair_len)))
    assert np.array_equal(wpcm, warp_ref.pcm32(w))
    want, want_pos = span_ref.wsola_spans(D["snd"], idx, wf, wl, ooff, maps, moff, frames, pair_len, SEARCH)
    assert np.array_equal(pos, want_pos)
    assert np.array_equal(bits(s), bits(want)) and np.array_equal(spcm, warp_ref.pcm32(s))
    assert not np.array_equal(bits(s), bits(w))                  # (the search does move frames here)


PROBE = hc.Probe(NAME, hc.DTW64, _spans,
                 ("ssym_dtw_align_spans_sizes", "ssym_dtw_align_spans", "ssym_reconstruct_warped_spans", "ssym_reconstruct_wsola_spans"),
                 {"src": (hc.F, SPAN_SRC), "tgt": (hc.F, SPAN_TGT), "snd": (hc.S, SPAN_SND), "out": ("lengths", SPAN_OUT)},
                 13, 0x4207, scale=hc._sigma(13))
hc.PROBES.setdefault(NAME, PROBE)
gh.CHECKS.setdefault(NAME, check_spans)


def test_the_probe_is_registered_where_the_history_tests_look():
    assert hc.PROBES[NAME] is PROBE and gh.CHECKS[NAME] is check_spans
    assert PROBE in hc.by_ctx()[hc.ctx_key(hc.DTW64)][1]
    # every variant's spans and windows are inside their segments and sounds: no prelude is refused for its shape
    for variant in (hc.PLAIN, hc.twin("nan"), hc.larger("same")):
        ls = {name: hc.variant_lengths(lengths, variant) for name, (_, lengths) in PROBE.sets.items()}
        src, tgt, first, last = spans_of(ls["src"], ls["tgt"])
        seg = [ls["src"][int(s)] for s in src]
        assert span_ref.align_status(seg, [ls["tgt"][int(t)] for t in tgt], list(zip(first.tolist(), last.tolist())),
                                     13 * variant.grow) == span_ref.OK
        idx = [t % len(ls["snd"]) for t in range(len(ls["out"]))]
        wf, wl = windows_of([ls["snd"][i] for i in idx])
        assert span_ref.window_status(ls["snd"], idx, wf, wl) == span_ref.OK


def test_two_fresh_contexts_agree_bit_for_bit(fresh):  # noqa: F811
    gh.test_two_fresh_contexts_agree_bit_for_bit(fresh, NAME)


def test_the_fresh_answer_is_the_references(oracle, fresh):  # noqa: F811
    gh.test_the_fresh_answer_is_the_references(oracle, fresh, NAME)


@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
def test_the_dirty_answer_is_the_fresh_answer(fresh, prelude):  # noqa: F811
    gh.test_the_dirty_answer_is_the_fresh_answer(fresh, NAME, prelude)


@pytest.mark.parametrize("other", ["align", "align_paced", "align_slab", "spot_sym", "reconstruct"])
def test_another_call_first(fresh, other):  # noqa: F811
    """The plain alignments, a spot and the plain reconstructions before the span calls, and after them."""
    gh.run_dirty(PROBE, lambda e: hc.dirty_run(e, hc.PROBES[other], hc.PLAIN), fresh, "%s after %s" % (NAME, other))
    gh.run_dirty(hc.PROBES[other], lambda e: hc.dirty_run(e, PROBE, hc.PLAIN), fresh, "%s after %s" % (other, NAME))
