"""reconstruct_covered with gaps on the GPU (DESIGN.md section 2 "Cover with gaps"): on the planted-intruder target with
synthetic samples the gap's stretch is exactly silence or exactly the target's samples, everything else is bit for bit what
warp returns for the same cut sounds and indices, and gap_cost=None is today's reconstruct_covered.  Also cover, cover_long
and cover_live with gap_cost against each other and the restatement."""
import numpy as np
import pytest

import cover_gaps_ref as ref
from paced_match_gpu import bits
from soundsym_amd import HOP, Engine, Gap, Piece, Sound, SoundDictionary, SoundSequence, push_sounds

pytestmark = pytest.mark.gpu

GAP = ref.GAP


def _sound(rng, feats, extra=0):
    return Sound(rng.standard_normal(feats.shape[0] * HOP + extra), 16000.0, feats.reshape(-1), None, ncoeffs=feats.shape[1])


@pytest.fixture(scope="module")
def intruder():
    """The planted-intruder case as a dictionary of sounds and a target sound with synthetic samples, with the restatement's
    cover at gap_cost 1."""
    class I:
        pass
    i = I()
    i.segs, i.x, i.planted, (i.first, i.last) = ref.intruder_case()
    rng = np.random.default_rng(0x5EED)
    i.d = SoundDictionary(engine=Engine(metric="dtw", dtype="f64"))
    i.d.sounds = [_sound(rng, s) for s in i.segs]
    i.target = _sound(rng, i.x, 100)
    i.want = ref.merged(ref.cover(i.segs, i.x, 0.0, 1.0)[0])
    yield i
    i.d.engine.close()


def _same_cover(cover, want, total):
    assert [(GAP if p.is_gap else p.source_index, p.start_frame, p.end_frame) for p in cover.pieces] == [w[:3] for w in want]
    assert bits([p.cost for p in cover.pieces]).tolist() == bits([w[3] for w in want]).tolist()
    assert bits(cover.total) == bits(total)


@pytest.mark.parametrize("search", [0, 64])
def test_gap_stretches_are_spliced_between_what_warp_returns(intruder, search):
    i, d, target = intruder, intruder.d, intruder.target
    smp = target.samples()
    outs = {}
    for fill in ("silence", "target"):
        cover, samples, pcm = d.reconstruct_covered(target, search=search, want_pcm32=True, gap_cost=1.0, gap_fill=fill)
        _same_cover(cover, i.want, 7.0)
        assert samples.size == smp.size == pcm.size and pcm.dtype == np.int32
        outs[fill] = (cover, samples, pcm)
    cover = outs["silence"][0]
    gap, = cover.gaps
    assert isinstance(gap, Gap) and (gap.start_frame, gap.end_frame, gap.cost) == (i.first, i.last, 7.0)
    assert [(p.source_index, p.start_frame, p.end_frame) for p in cover.sounding] == i.planted and cover.covered_frames == i.x.shape[0] - 7
    a, b = gap.sample_span(smp.size)
    assert (a, b) == (i.first * HOP, (i.last + 1) * HOP)
    assert not outs["silence"][1][a:b].any() and not outs["silence"][2][a:b].any()
    assert np.array_equal(outs["target"][1][a:b], smp[a:b]) and smp[a:b].any()
    x = 2147483647.0 * smp[a:b]
    assert np.array_equal(outs["target"][2][a:b], np.trunc(np.clip(x, -2147483648.0, 2147483647.0)).astype(np.int64).astype(np.int32))
    # everywhere else: warp called directly with the same cut sounds and indices
    cuts = SoundSequence.from_cover(target, cover).sounds()
    assert len(cuts) == len(i.planted) and all(isinstance(p, Piece) for p in cover.sounding)
    by_hand, by_hand_pcm = d.warp(cuts, indices=cover.indices(), want_pcm32=True, search=search, step="paced")
    assert by_hand.size == smp.size - (b - a)
    for _, samples, pcm in outs.values():
        assert np.array_equal(np.concatenate([samples[:a], samples[b:]]), by_hand)
        assert np.array_equal(np.concatenate([pcm[:a], pcm[b:]]), by_hand_pcm)
    # without want_pcm32 the samples alone
    again = d.reconstruct_covered(target, search=search, gap_cost=1.0)
    assert len(again) == 2 and np.array_equal(again[1], outs["silence"][1])


def test_gap_cost_none_and_inf_are_todays_reconstruct_covered(intruder):
    d, target = intruder.d, intruder.target
    cover, samples = d.reconstruct_covered(target)
    assert cover and not cover.gaps and cover.covered_frames == cover.num_frames
    by_hand = d.warp(SoundSequence.from_cover(target, cover).sounds(), indices=cover.indices(), step="paced")
    assert np.array_equal(samples, by_hand)
    for same in (d.reconstruct_covered(target, gap_cost=None), d.reconstruct_covered(target, gap_cost=float("inf"), gap_fill="target")):
        assert np.array_equal(same[1], samples) and bits(same[0].total) == bits(cover.total)
        assert [(p.source_index, p.start_frame, p.end_frame, p.cost) for p in same[0].pieces] == \
               [(p.source_index, p.start_frame, p.end_frame, p.cost) for p in cover.pieces]
    plain = d.cover([target])[0]
    assert [(p.source_index, p.start_frame, p.end_frame, p.cost) for p in plain.pieces] == \
           [(p.source_index, p.start_frame, p.end_frame, p.cost) for p in cover.pieces]


def test_a_cover_of_gaps_alone_and_a_gap_at_the_end(intruder):
    d = intruder.d
    rng = np.random.default_rng(3)
    lone = _sound(rng, intruder.x[intruder.first:intruder.last + 1], 40)       # the intruder's frames alone
    for fill, want in (("silence", np.zeros(lone.samples().size)), ("target", lone.samples())):
        cover, samples = d.reconstruct_covered(lone, gap_cost=1.0, gap_fill=fill)
        assert [type(p) for p in cover.pieces] == [Gap] and cover.covered_frames == 0 and cover.total == 7.0
        assert np.array_equal(samples, want)                                   # a gap that ends the target runs to its last sample
    tail = _sound(rng, intruder.x[:intruder.last + 1], 40)                     # three planted pieces, then the gap
    cover, samples = d.reconstruct_covered(tail, gap_cost=1.0, gap_fill="target")
    assert cover.pieces[-1].is_gap and len(cover.sounding) == 3
    at = intruder.first * HOP
    assert np.array_equal(samples[at:], tail.samples()[at:])
    assert np.array_equal(samples[:at], d.warp(SoundSequence.from_cover(tail, cover).sounds(), indices=cover.indices(), step="paced"))


def test_cover_long_and_cover_live_give_covers_with_gaps(intruder):
    i, d = intruder, intruder.d
    cover = d.cover([i.target, i.target], 0.0, 1.0)
    for c in cover:
        _same_cover(c, i.want, 7.0)
    long = d.cover_long(i.target, 0.0, 64, 1.0)
    _same_cover(long, i.want, 7.0)
    assert not d.cover([_sound(np.random.default_rng(4), i.x[:0])], 0.0, 1.0)[0]       # no frames: no cover, gaps or not
    # live: growing sounds whose stream the coverer follows; covers() after flush = cover(gap_cost=) of the finished sounds
    e = d.engine
    rng = np.random.default_rng(0x11FE)
    recs = [rng.standard_normal(20000) * 0.3, np.sin(0.05 * np.arange(15000)) + 0.05 * rng.standard_normal(15000)]
    live_d = SoundDictionary(engine=e)
    live_d.sounds = [Sound.from_samples(r[4000:4000 + n], 16000.0, engine=e) for r, n in zip(recs, (2304, 3328))]
    sounds = [Sound.from_samples(r[:1500], 16000.0, engine=e) for r in recs]
    push_sounds(sounds, [r[1500:2000] for r in recs], e)
    gap_cost = 5.0
    live = live_d.cover_live(sounds, 0.5, gap_cost)
    emitted = live.poll()
    for lo, hi in ((2000, 9000), (9000, 20000)):
        push_sounds(sounds, [r[lo:hi] for r in recs], e)
        emitted += live.poll()
    emitted += live.flush()
    assert all(isinstance(p, (Piece, Gap)) for _, p in emitted)
    want = live_d.cover(sounds, 0.5, gap_cost)
    for got, w in zip(live.covers(), want):
        assert w and got.num_frames == w.num_frames
        assert [(type(p), p.start_frame, p.end_frame) for p in got.pieces] == [(type(p), p.start_frame, p.end_frame) for p in w.pieces]
        assert bits([p.cost for p in got.pieces]).tolist() == bits([p.cost for p in w.pieces]).tolist()
        assert bits(got.total) == bits(w.total)
    live.close()
