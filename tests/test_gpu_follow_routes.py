"""dynamics="target" on every reconstructing method, on the recordings in tests/golden/audio/ and on a small synthetic
dictionary: the result is the method's plain output put through Engine.follow_envelope against the targets' own samples, bit
for bit (samples and 32-bit conversion); dynamics=None is the call without the keyword, bit for bit; and
reconstruct_mosaic(gap_fill="target") keeps the target's bits inside a long gap from two hops inside its ends."""
import os

import numpy as np
import pytest

import follow_ref as fr
import mirror_cases as mc
import mosaic_ref
from soundsym_amd import HOP, Engine, Sound, SoundDictionary, SoundSequence, follow_envelope
from soundsym_amd import io as sio
from soundsym_amd.api import frame_features

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAINS = (8.0, 1.5)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


class World:
    """An f64 dtw engine; S a dictionary of cut segments, C those a cover takes, R one of uncut recordings, the targets."""


@pytest.fixture(scope="module")
def engine():
    e = Engine(metric="dtw", dtype="f64")
    yield e
    e.close()


def _dictionary(e, sounds):
    d = SoundDictionary(engine=e)
    d.sounds = [s for s in sounds if s.num_frames() > 0]
    return d


@pytest.fixture(scope="module")
def synthetic(engine):
    c = mc.build()
    snd = lambda pair: Sound(pair[0], mc.RATE, pair[1].reshape(-1))      # noqa: E731
    w = World()
    w.e, w.S, w.R = engine, _dictionary(engine, [snd(p) for p in c.segs]), _dictionary(engine, [snd(p) for p in c.recs])
    w.C = _dictionary(engine, [s for s in w.S.sounds if s.num_frames() <= 128])       # a cover takes no longer segment
    w.tgts = [t for t in (snd(p) for p in c.tgts) if t.num_frames() > 0]
    w.one = w.tgts[3]                                                     # 33 frames
    return w


@pytest.fixture(scope="module")
def recorded(engine):
    """Excerpts of the two recordings: sample.wav's first 160 frames as ten 16-frame segments (S) and as two uncut halves (R);
    four stretches of Section_7_1.wav of 5 ... 40 frames as the targets."""
    gold = os.path.join(ROOT, "tests", "golden", "audio")
    s_smp, srate = sio.read_wav(os.path.join(gold, "sample.wav"))
    t_smp, rate = sio.read_wav(os.path.join(gold, "Section_7_1.wav"))
    start = int(np.argmax(np.abs(s_smp) > 0.02))                          # past the leading silence
    s_smp = s_smp[start:start + 160 * HOP]
    sound = lambda x, r: Sound(x, r, frame_features(x, r, engine=engine))      # noqa: E731
    w = World()
    w.e = engine
    w.S = SoundDictionary.from_segments(sound(s_smp, srate), [16 * HOP] * 10, engine=engine)
    w.R = _dictionary(engine, [sound(s_smp[:80 * HOP], srate), sound(s_smp[80 * HOP:], srate)])
    w.C = w.S
    first = int(np.argmax(np.abs(t_smp) > 0.02))
    cuts = [(0, 5), (30, 40), (90, 17), (140, 33)]
    w.tgts = [sound(t_smp[first + a * HOP:first + (a + n) * HOP + 100], rate) for a, n in cuts]
    w.one = w.tgts[3]
    assert len(w.S.sounds) == 10 and all(t.num_frames() >= 5 for t in w.tgts)
    return w


def _followed(w, plain, targets, max_gain):
    """What dynamics="target" must give: the plain samples through Engine.follow_envelope, and the restatement's word on it."""
    off = np.concatenate([[0], np.cumsum([t.samples().size for t in targets])]).astype(np.uint64)
    ref = np.concatenate([t.samples() for t in targets])
    out, pcm = w.e.follow_envelope(plain, off, ref, off, max_gain, want_pcm32=True)
    want = fr.follow(plain, off, ref, off, max_gain)
    assert np.array_equal(_bits(out), _bits(want[0])) and np.array_equal(pcm, want[1])
    return out, pcm


def _check(w, call, targets, pick=lambda res: res):
    """call(**kw) is one of the seven methods with want_pcm32; pick takes (samples, pcm) out of what it returns."""
    plain = pick(call())
    none = pick(call(dynamics=None, max_gain=3.0))
    assert np.array_equal(_bits(none[0]), _bits(plain[0])) and np.array_equal(none[1], plain[1])
    assert plain[0].size == sum(t.samples().size for t in targets)
    for g in GAINS:
        got = pick(call(dynamics="target", max_gain=g))
        out, pcm = _followed(w, plain[0], targets, g)
        assert np.array_equal(_bits(got[0]), _bits(out)) and np.array_equal(got[1], pcm), g
    # the follower changes the samples, unless the method gave the target back whole (one gap filled with the target): identity
    whole = np.array_equal(_bits(plain[0]), _bits(np.concatenate([t.samples() for t in targets])))
    assert np.array_equal(_bits(got[0]), _bits(plain[0])) == whole
    return plain[0], got[0]


@pytest.fixture(scope="module", params=["synthetic", "recorded"])
def world(request):
    return request.getfixturevalue(request.param)


@pytest.mark.parametrize("search", [0, 32])
def test_warp(world, search):
    w = world
    _check(w, lambda **kw: w.S.warp(w.tgts, None, True, search, **kw), w.tgts)
    seq = SoundSequence.new(w.tgts)
    _check(w, lambda **kw: seq.reconstruct_warped_from_dictionary(w.S, True, search, **kw), w.tgts)


def test_warp_keeps_what_else_it_returns(world):
    w = world
    plain = w.S.warp(w.tgts, None, True, 32, want_pos=True)
    got = w.S.warp(w.tgts, None, True, 32, want_pos=True, dynamics="target")
    assert len(got) == len(plain) == 4 and np.array_equal(got[2], plain[2]) and np.array_equal(got[3], plain[3])
    out, pcm = _followed(w, plain[0], w.tgts, 8.0)
    assert np.array_equal(_bits(got[0]), _bits(out)) and np.array_equal(got[1], pcm)


def test_reconstruct_from_dictionary(world):
    w = world
    seq = SoundSequence.new(w.tgts)
    _check(w, lambda **kw: seq.reconstruct_from_dictionary(w.S, True, **kw), w.tgts)
    alone = seq.reconstruct_from_dictionary(w.S, dynamics="target")
    assert isinstance(alone, np.ndarray) and np.array_equal(_bits(alone), _bits(seq.reconstruct_from_dictionary(w.S, True, dynamics="target")[0]))


@pytest.mark.parametrize("step", ["symmetric", "paced"])
def test_reconstruct_spotted(world, step):
    w = world
    spots = w.R.reconstruct_spotted(w.tgts, step)[0]
    assert any(not s.empty() for s in spots)
    _check(w, lambda **kw: w.R.reconstruct_spotted(w.tgts, step, 0, True, **kw), w.tgts, pick=lambda res: res[1:])
    seq = SoundSequence.new(w.tgts)
    _check(w, lambda **kw: seq.reconstruct_spotted_from_dictionary(w.R, step, 16, True, **kw), w.tgts, pick=lambda res: res[1:])
    assert [s.source_index for s in w.R.reconstruct_spotted(w.tgts, step, dynamics="target")[0]] == [s.source_index for s in spots]


@pytest.mark.parametrize("gap", [None, 6.0])
def test_reconstruct_covered(world, gap):
    w = world
    kw0 = dict(piece_penalty=2.0, want_pcm32=True, gap_cost=gap, gap_fill="target")
    cover = w.C.reconstruct_covered(w.one, **kw0)[0]
    assert len(cover.pieces) >= 1
    _check(w, lambda **kw: w.C.reconstruct_covered(w.one, **kw0, **kw), [w.one], pick=lambda res: res[1:])


@pytest.mark.parametrize("gap", [None, 6.0])
def test_reconstruct_mosaic(world, gap):
    w = world
    kw0 = dict(piece_penalty=1.0, gap_cost=gap, gap_fill="target", search=16, want_pcm32=True)
    mosaic = w.R.reconstruct_mosaic(w.one, **kw0)[0]
    assert len(mosaic.pieces) >= 1
    _check(w, lambda **kw: w.R.reconstruct_mosaic(w.one, **kw0, **kw), [w.one], pick=lambda res: res[1:])
    again = w.R.reconstruct_mosaic(w.one, mosaic=mosaic, gap_fill="target", search=16, dynamics="target")
    assert np.array_equal(_bits(again[1]), _bits(w.R.reconstruct_mosaic(w.one, **kw0, dynamics="target")[1]))


def test_the_convenience_function(world):
    w = world
    plain = w.S.warp([w.one])
    got = follow_envelope(Sound(plain, w.one.sample_rate(), None, "warped"), w.one, 4.0, engine=w.e)
    out, _ = _followed(w, plain, [w.one], 4.0)
    assert isinstance(got, Sound) and np.array_equal(_bits(got.samples()), _bits(out)) and got.name == "warped"


def test_a_long_gap_keeps_the_targets_bits_from_two_hops_inside(engine):
    """Two recordings of 9 and 8 frames; the target is a span of one, EIGHT frames far from everything, a span of the other.
    With gap_fill="target" the gap's stretch is the target's own samples, so every boundary whose window lies inside it has
    the gain 1: the samples from two hops inside the stretch's ends keep the target's bits; outside, the pieces are scaled."""
    rng = np.random.default_rng(0x3052)
    recs = [mosaic_ref._real(rng, (9, 12)), mosaic_ref._real(rng, (8, 12))]
    x = np.concatenate([recs[1][2:7], mosaic_ref._real(rng, (8, 12)) + 100.0, np.repeat(recs[0][3:6], 2, axis=0)], axis=0)
    rec_smp = [rng.standard_normal(a.shape[0] * HOP + 100) * 0.1 for a in recs]
    tgt_smp = rng.standard_normal(x.shape[0] * HOP + 37) * 0.02
    D = SoundDictionary(engine=engine)
    D.sounds = [Sound(s, mc.RATE, a.reshape(-1)) for s, a in zip(rec_smp, recs)]
    target = Sound(tgt_smp, mc.RATE, x.reshape(-1))
    mosaic, plain = D.reconstruct_mosaic(target, 1.0, 1.5, "target")
    mosaic2, out = D.reconstruct_mosaic(target, 1.0, 1.5, "target", dynamics="target")
    lengths = mosaic.segment_lengths(tgt_smp.size)
    gaps = [(sum(lengths[:i]), sum(lengths[:i + 1])) for i, p in enumerate(mosaic.pieces) if p.is_gap]
    assert len(gaps) == 1 and [p.is_gap for p in mosaic2.pieces] == [p.is_gap for p in mosaic.pieces]
    a, b = gaps[0]
    assert a % HOP == 0 and b % HOP == 0 and b - a == 8 * HOP > 4 * HOP and a > 0 and b < tgt_smp.size
    assert np.array_equal(_bits(plain[a:b]), _bits(tgt_smp[a:b]))
    inside = slice(a + 2 * HOP, b - 2 * HOP)
    assert np.array_equal(_bits(out[inside]), _bits(tgt_smp[inside]))
    assert not np.array_equal(_bits(out[:a]), _bits(plain[:a])) and not np.array_equal(_bits(out[b:]), _bits(plain[b:]))
    g = fr.gains(plain, tgt_smp, 8.0)
    assert np.all(g[a // HOP + 2:b // HOP - 1] == 1.0) and g[a // HOP + 1] != 1.0 and g[b // HOP - 1] != 1.0
    # with silence in the gap the same stretch is silent and stays so
    _, quiet = D.reconstruct_mosaic(target, 1.0, 1.5, "silence", dynamics="target")
    assert not quiet[a:b].any()
