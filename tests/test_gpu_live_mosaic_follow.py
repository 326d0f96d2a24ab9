"""SoundDictionary.mosaic_live(audio=True, dynamics="target") on the GPU: two sounds fed by push_sounds in odd blocks, every
poll's audio() through the LiveMosaic's Follower after the gap splice; the concatenated audio() of each sound equals
reconstruct_mosaic(dynamics="target") on its finished mosaic, bit for bit, samples and pcm, for the plain warp and a search
and both gap_fills under a gap_cost that leaves gaps.  With dynamics=None audio() has the bits of a LiveMosaic made without
the argument, and no follower is created."""
import numpy as np
import pytest

from soundsym_amd import Engine, Sound, SoundDictionary, push_sounds

pytestmark = pytest.mark.gpu

BLOCK = 1777
PENALTY, GAP = 2.0, 8.0
FRAMES = lambda n: 1024 + (n - 1) * 256      # noqa: E731


@pytest.fixture(scope="module")
def spoken():
    """a dictionary of two synthetic recordings of 64 frames and two targets of about 48 that string spans of them together,
    at other levels than they were recorded at and with a stretch of noise no recording covers"""
    rng = np.random.default_rng(0xF0110A)
    e = Engine(metric="dtw", dtype="f64")
    rate = 16000.0
    t = np.arange(FRAMES(64)) / rate
    recs = [np.sin(2 * np.pi * (200 + 300 * k) * t * (1 + 0.3 * t)) * 0.4 + 0.05 * rng.standard_normal(t.size) for k in range(2)]
    d = SoundDictionary(engine=e)
    d.sounds = [Sound.from_samples(r, rate, engine=e) for r in recs]
    level = lambda n: 0.6 * (1.0 + 0.25 * np.sin(np.arange(n) / 900.0))      # noqa: E731
    targets = [np.concatenate([recs[1][2000:7000], rng.standard_normal(2500) * 0.2, recs[0][1000:7000]])[:FRAMES(48) + 77],
               np.concatenate([recs[0][500:6000], recs[1][9000:15000]])[:FRAMES(45)]]
    targets = [x * level(x.size) for x in targets]
    yield e, d, targets, rate
    e.close()


def _feed(e, d, targets, rate, **kw):
    sounds = [Sound.from_samples(x[:2 * BLOCK], rate, engine=e) for x in targets]
    push_sounds(sounds, [x[2 * BLOCK:3 * BLOCK] for x in targets], e)          # (the first push makes the shared stream)
    live = d.mosaic_live(sounds, PENALTY, GAP, audio=True, **kw)
    live.poll()
    audio = [live.audio(want_pcm32=True)]
    for lo in range(3 * BLOCK, max(x.size for x in targets), BLOCK):
        push_sounds(sounds, [x[lo:lo + BLOCK] for x in targets], e)
        live.poll()
        audio.append(live.audio(want_pcm32=True))
    live.flush()
    audio.append(live.audio(want_pcm32=True))
    return live, sounds, audio


@pytest.mark.parametrize("search,gap_fill", [(0, "silence"), (0, "target"), (8, "silence"), (8, "target")])
def test_followed_audio_is_reconstruct_mosaic_with_dynamics(spoken, search, gap_fill):
    e, d, targets, rate = spoken
    live, sounds, audio = _feed(e, d, targets, rate, search=search, gap_fill=gap_fill, dynamics="target", max_gain=4.0)
    try:
        assert live.follower is not None and live.follower.max_gain == 4.0
        mosaics = live.mosaics()
        assert any(p.is_gap for p in mosaics[0].pieces) and len(mosaics[0].sounding) >= 2
        early = 0
        for l, x in enumerate(targets):
            smp = np.concatenate([a[l][0] for a in audio])
            pcm = np.concatenate([a[l][1] for a in audio])
            _, want, want_pcm = d.reconstruct_mosaic(sounds[l], gap_fill=gap_fill, search=search, want_pcm32=True, mosaic=mosaics[l],
                                                     dynamics="target", max_gain=4.0)
            _, plain = d.reconstruct_mosaic(sounds[l], gap_fill=gap_fill, search=search, mosaic=mosaics[l])
            assert smp.size == x.size == want.size
            assert np.array_equal(smp.view(np.uint64), want.view(np.uint64)), (l, search, gap_fill)
            assert np.array_equal(pcm, want_pcm)
            assert not np.array_equal(want, plain)                  # the follower had something to do
            early += sum(a[l][0].size for a in audio[:-1])
        assert early > 0                                            # audio came out while the sounds were still growing
        assert live.audio()[0].size == 0                            # nothing is returned twice
    finally:
        live.close()


def test_without_dynamics_nothing_changes(spoken):
    e, d, targets, rate = spoken
    named, _, audio_named = _feed(e, d, targets, rate, search=8, gap_fill="target", dynamics=None)
    plain, _, audio_plain = _feed(e, d, targets, rate, search=8, gap_fill="target")
    try:
        assert named.follower is None and plain.follower is None
        assert len(audio_named) == len(audio_plain)
        for a, b in zip(audio_named, audio_plain):
            for l in range(len(targets)):
                assert a[l][0].tobytes() == b[l][0].tobytes() and a[l][1].tobytes() == b[l][1].tobytes()
    finally:
        named.close()
        plain.close()


def test_mosaic_live_checks_the_dynamics_first(spoken):
    e, d, targets, rate = spoken
    for kw in ({"dynamics": "source"}, {"dynamics": "target", "max_gain": 0.5}, {"dynamics": "target", "audio": False}):
        with pytest.raises(ValueError):
            d.mosaic_live([], PENALTY, GAP, **{"audio": True, **kw})
