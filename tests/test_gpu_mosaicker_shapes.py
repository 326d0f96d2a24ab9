"""The mosaicker at every shape its kernels take another path on (the threads' stride loop over G, the partial last wave,
dim 1 ... 64, empty segments anywhere in the dictionary), and the Python layer on top of it (mosaic_long, mosaic_live,
reconstruct_mosaic(mosaic=)): bit for bit against tests/live_mosaic_ref.py and against Engine.dtw_mosaic / SoundDictionary.
mosaic on the same f64 engine."""
import os

import numpy as np
import pytest

import mosaic_ref
import mosaicker_gpu as mg
from soundsym_amd import Engine

pytestmark = pytest.mark.gpu

INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(G, dim, seed, T=24):
    """a dictionary of G frames in three recordings with empty segments at the front, in the middle and at the end, and a
    target that copies a span, doubles one and then wanders"""
    rng = np.random.default_rng(seed)
    a = G // 3
    lens = [0, a, 0, 0, G - a - (G - a) // 2, (G - a) // 2, 0]
    segs = [mosaic_ref._real(rng, (n, dim)) for n in lens]
    assert sum(lens) == G
    big = max(segs, key=lambda s: s.shape[0])
    parts = [big[:8], np.repeat(big[-5:], 2, axis=0), mosaic_ref._real(rng, (T, dim))]
    x = np.concatenate(parts, axis=0)[:T]
    return segs, (x + 0.01 * mosaic_ref._real(rng, x.shape)).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("G,dim", [(1, 13), (63, 1), (64, 13), (65, 64), (1023, 13), (1025, 1), (2100, 13), (2100, 64)])
def test_every_G_and_dim(G, dim):
    segs, x = _case(G, dim, 0x5A0 + G + dim)
    with mg.Dict(segs, dim) as D:
        for penalty, gap in ((1.0, None), (0.5, 1.0)):
            live = mg.Live(D, 2, penalty, gap)
            for a, b in ((0, 1), (1, 8), (8, 24)):
                live.push([x[a:b], x[:0] if a else x[:3]])
            live.flush(0)
            live.flush(1)
            mg.same_as_offline(D, live.emitted[0], x, penalty, gap)
            mg.same_as_offline(D, live.emitted[1], x[:3], penalty, gap)
            live.close()


def test_a_dictionary_of_empty_segments_only():
    x = np.ones((5, 2))
    with mg.Dict([np.zeros((0, 2)), np.zeros((0, 2))], 2) as D:
        for gap in (None, 1.5):
            live = mg.Live(D, 1, 1.0, gap)
            live.push([x])
            live.flush()
            assert len(live.emitted[0]) == (0 if gap is None else 5)
            live.close()


# -- the Python layer ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def spoken():
    """a dictionary of three synthetic recordings and a target of 300 frames that strings spans of them together"""
    from soundsym_amd import Sound, SoundDictionary
    rng = np.random.default_rng(0x10CA1)
    e = Engine(metric="dtw", dtype="f64")
    rate = 16000.0
    t = np.arange(30000) / rate
    recs = [np.sin(2 * np.pi * (200 + 300 * k) * t * (1 + 0.3 * t)) * 0.4 + 0.05 * rng.standard_normal(t.size) for k in range(3)]
    d = SoundDictionary(engine=e)
    d.sounds = [Sound.from_samples(r, rate, engine=e) for r in recs]
    samples = np.concatenate([recs[1][4000:24000], rng.standard_normal(12000) * 0.2, recs[0][1000:22000], recs[2][:25000]])
    samples = samples[:1024 + 299 * 256]                                       # 300 frames
    target = Sound.from_samples(samples, rate, engine=e)
    yield e, d, target, samples, rate
    e.close()


def _same_mosaic(a, b):
    assert np.float64(a.total).tobytes() == np.float64(b.total).tobytes() and a.num_frames == b.num_frames
    assert a.frame_costs.tobytes() == b.frame_costs.tobytes() and len(a.pieces) == len(b.pieces)
    for p, q in zip(a.pieces, b.pieces):
        assert (p.is_gap, p.start_frame, p.end_frame) == (q.is_gap, q.start_frame, q.end_frame)
        assert np.float64(p.cost).tobytes() == np.float64(q.cost).tobytes()
        if not p.is_gap:
            assert (p.source_index, p.frame_map.tolist()) == (q.source_index, q.frame_map.tolist())


@pytest.mark.parametrize("block", [1, 64, 300])
def test_mosaic_long_is_mosaic(spoken, block):
    e, d, t300, samples, rate = spoken
    for penalty, gap in ((2.0, None), (2.0, 30.0)):
        want = d.mosaic([t300], penalty, gap)[0]
        assert want.num_frames == 300 and len(want.pieces) >= 3
        _same_mosaic(d.mosaic_long(t300, penalty, block, gap), want)


def test_mosaic_long_checks_its_arguments_first(spoken):
    e, d, target, _, _ = spoken
    with pytest.raises(ValueError, match="block_frames"):
        d.mosaic_long(target, 1.0, 0)
    with pytest.raises(ValueError, match="one Sound"):
        d.mosaic_long([target], 1.0)
    with pytest.raises(ValueError, match="Mosaic"):
        d.reconstruct_mosaic(target, 1.0, mosaic="no")


def test_mosaic_live_then_reconstruct_is_the_offline_reconstruction(spoken):
    from soundsym_amd import MosaicPiece, Sound, push_sounds
    e, d, target, samples, rate = spoken
    samples = np.asarray(target.samples())
    sounds = [Sound.from_samples(samples[:3000], rate, engine=e)]
    with pytest.raises(ValueError, match="share one stream"):
        d.mosaic_live(sounds)
    push_sounds(sounds, [samples[3000:4000]], e)
    live = d.mosaic_live(sounds, 2.0)
    got = live.poll()
    for lo in range(4000, samples.size, 9000):
        push_sounds(sounds, [samples[lo:lo + 9000]], e)
        new = live.poll()
        assert all(isinstance(p, MosaicPiece) for _, p in new)
        got += new
        src, frame, cost, start = live.committed()[0]
        consumed, covered, committed, total = live.pending()
        assert src.size == int(committed[0]) and got[-1][1].end_frame < src.size if got else True
    before = len(got)
    got += live.flush()
    assert 0 < before < len(got)
    mosaic = live.mosaics()[0]
    want = d.mosaic([sounds[0]], 2.0)[0]
    _same_mosaic(mosaic, want)
    assert [p.start_frame for _, p in got] == [p.start_frame for p in want.pieces]
    live.close()
    a = d.reconstruct_mosaic(sounds[0], 2.0, want_pcm32=True)
    b = d.reconstruct_mosaic(sounds[0], mosaic=mosaic, want_pcm32=True)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and np.abs(a[1]).max() > 0


def test_the_example_prints_the_offline_mosaic_and_writes_its_resynthesis(spoken, tmp_path, capsys):
    import importlib.util
    from soundsym_amd import Sound, SoundDictionary
    from soundsym_amd.io import read_wav, write_wav32
    e, d, target, samples, rate = spoken
    paths = [str(tmp_path / name) for name in ("target.wav", "rec.wav", "out.wav")]
    write_wav32(paths[0], samples[:40000], rate)
    write_wav32(paths[1], np.asarray(d.sounds[1].samples()), rate)
    spec = importlib.util.spec_from_file_location("live_mosaic_example", os.path.join(ROOT, "examples", "live_mosaic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mosaic, out = mod.main(["-s", paths[0], "-d", paths[1], "-o", paths[2], "--block", "5000", "--penalty", "2"])
    lines = [l for l in capsys.readouterr().out.splitlines() if "<- recording" in l]
    one = SoundDictionary(engine=e)
    one.sounds = [Sound.from_path(paths[1], engine=e)]
    want, want_out = one.reconstruct_mosaic(Sound.from_path(paths[0], engine=e), 2.0, search=256)
    _same_mosaic(mosaic, want)
    assert len(lines) == len(want.pieces) >= 2 and out.tobytes() == want_out.tobytes()
    assert read_wav(paths[2])[0].size == out.size
