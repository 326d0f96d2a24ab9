"""SoundDictionary.mosaic_live(audio=True) on the GPU: two sounds fed by push_sounds in 1000-sample blocks, every poll's
committed frames taken by the LiveMosaic's Resynth device to device; the concatenated audio() of each sound equals
reconstruct_mosaic on its finished mosaic, bit for bit, samples and pcm, for the plain warp and a search and both
gap_fills.  With audio=False the polls, the pieces and the mosaics are what they are with it, and audio() refuses."""
import numpy as np
import pytest

from soundsym_amd import Engine, Sound, SoundDictionary, push_sounds

pytestmark = pytest.mark.gpu

BLOCK = 1000
PENALTY, GAP = 2.0, 8.0


@pytest.fixture(scope="module")
def spoken():
    """a dictionary of three synthetic recordings and two targets that string spans of them together"""
    rng = np.random.default_rng(0xA0D10)
    e = Engine(metric="dtw", dtype="f64")
    rate = 16000.0
    t = np.arange(20000) / rate
    recs = [np.sin(2 * np.pi * (200 + 300 * k) * t * (1 + 0.3 * t)) * 0.4 + 0.05 * rng.standard_normal(t.size) for k in range(3)]
    d = SoundDictionary(engine=e)
    d.sounds = [Sound.from_samples(r, rate, engine=e) for r in recs]
    # (a frame of the noise is about 25 from every frame of the recordings, a frame of a copied span about 1.3: GAP lies between)
    targets = [np.concatenate([recs[1][3000:9000], rng.standard_normal(2500) * 0.2, recs[0][1000:7700]])[:1024 + 55 * 256 + 77],
               np.concatenate([recs[2][500:6000], recs[1][10000:14000]])[:1024 + 33 * 256]]
    yield e, d, targets, rate
    e.close()


def _feed(e, d, targets, rate, **kw):
    """The targets pushed BLOCK samples at a time with a poll after every push, then the flush: (live, pieces per poll,
    audio per poll)."""
    sounds = [Sound.from_samples(x[:2 * BLOCK], rate, engine=e) for x in targets]
    push_sounds(sounds, [x[2 * BLOCK:3 * BLOCK] for x in targets], e)          # (the first push makes the shared stream)
    live = d.mosaic_live(sounds, PENALTY, GAP, **kw)
    polls, audio = [live.poll()], []
    if kw.get("audio"):
        audio.append(live.audio(want_pcm32=True))
    for lo in range(3 * BLOCK, max(x.size for x in targets), BLOCK):
        push_sounds(sounds, [x[lo:lo + BLOCK] for x in targets], e)
        polls.append(live.poll())
        if kw.get("audio"):
            audio.append(live.audio(want_pcm32=True))
    polls.append(live.flush())
    if kw.get("audio"):
        audio.append(live.audio(want_pcm32=True))
    return live, sounds, polls, audio


def _tiles(polls):
    return [[(l, p.is_gap, p.start_frame, p.end_frame, np.float64(p.cost).tobytes()) for l, p in poll] for poll in polls]


@pytest.mark.parametrize("search,gap_fill", [(0, "silence"), (0, "target"), (48, "silence"), (48, "target")])
def test_audio_is_reconstruct_mosaic(spoken, search, gap_fill):
    e, d, targets, rate = spoken
    live, sounds, polls, audio = _feed(e, d, targets, rate, audio=True, search=search, gap_fill=gap_fill)
    try:
        mosaics = live.mosaics()
        assert any(p.is_gap for p in mosaics[0].pieces) and len(mosaics[0].sounding) >= 2
        early = 0
        for l, x in enumerate(targets):
            smp = np.concatenate([a[l][0] for a in audio])
            pcm = np.concatenate([a[l][1] for a in audio])
            _, want, want_pcm = d.reconstruct_mosaic(sounds[l], gap_fill=gap_fill, search=search, want_pcm32=True, mosaic=mosaics[l])
            assert smp.size == x.size == want.size
            assert np.array_equal(smp.view(np.uint64), want.view(np.uint64)), (l, search, gap_fill)
            assert np.array_equal(pcm, want_pcm)
            early += sum(a[l][0].size for a in audio[:-1])
        assert early > 0                                        # audio came out while the sounds were still growing
        assert live.audio()[0].size == 0                        # nothing is returned twice
    finally:
        live.close()


def test_without_audio_nothing_changes(spoken):
    e, d, targets, rate = spoken
    with_audio, _, polls_a, _ = _feed(e, d, targets, rate, audio=True)
    plain, sounds, polls, _ = _feed(e, d, targets, rate)
    try:
        assert plain.resynth is None and with_audio.resynth is not None
        assert _tiles(polls) == _tiles(polls_a)
        for a, b, s in zip(plain.mosaics(), with_audio.mosaics(), sounds):
            want = d.mosaic([s], PENALTY, GAP)[0]
            assert np.float64(a.total).tobytes() == np.float64(b.total).tobytes() == np.float64(want.total).tobytes()
            assert a.frame_costs.tobytes() == want.frame_costs.tobytes() and len(a.pieces) == len(want.pieces)
        with pytest.raises(ValueError, match="without audio"):
            plain.audio()
    finally:
        plain.close()
        with_audio.close()


def test_the_example_writes_the_same_wav_with_live_audio(spoken, tmp_path, capsys):
    import importlib.util
    import os
    from soundsym_amd.io import write_wav32
    e, d, targets, rate = spoken
    paths = [str(tmp_path / name) for name in ("target.wav", "rec.wav", "offline.wav", "live.wav")]
    write_wav32(paths[0], targets[1], rate)
    write_wav32(paths[1], np.asarray(d.sounds[2].samples()), rate)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("live_mosaic_example", os.path.join(root, "examples", "live_mosaic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["-s", paths[0], "-d", paths[1], "--block", "3000", "--penalty", "2", "--search", "32"]
    _, offline = mod.main(common + ["-o", paths[2]])
    plain = capsys.readouterr().out
    _, live = mod.main(common + ["-o", paths[3], "--live-audio"])
    told = capsys.readouterr().out
    assert open(paths[2], "rb").read() == open(paths[3], "rb").read() and offline.tobytes() == live.tobytes()
    pieces = lambda text: [l for l in text.splitlines() if "<- recording" in l]
    assert pieces(plain) == pieces(told) and pieces(plain)
    released = [int(l.split("]")[1].split()[0]) for l in told.splitlines() if "samples released" in l]
    assert len(released) == -(-targets[1].size // 3000) + 1 and sum(released) == live.size and sum(released[:-1]) > 0
    assert "samples released" not in plain


def test_mosaic_live_checks_the_audio_arguments_first(spoken):
    e, d, targets, rate = spoken
    for kw in ({"search": 513}, {"search": -1}, {"search": 2.5}, {"gap_fill": "noise"}):
        with pytest.raises(ValueError):
            d.mosaic_live([], PENALTY, GAP, audio=True, **kw)
