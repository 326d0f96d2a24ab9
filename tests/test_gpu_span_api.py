"""SoundDictionary.align(spans=), warp(spans=) and reconstruct_spotted on the reference recordings against the cut route
(cut(spots), then the existing calls with indices = arange), bit for bit, for both step patterns and with and without a
WSOLA search; context=True changes only what reaches past a span's end; examples/spot.py writes what the cut route gives."""
import os
import sys

import numpy as np
import pytest

from soundsym_amd import Engine, Sound, SoundDictionary, SoundSequence, Spot
from soundsym_amd import io as sio
from soundsym_amd.api import HOP, frame_features

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "audio")


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class _World:
    def __init__(self):
        self.e = e = Engine(metric="dtw", dtype="f64")
        t_smp, t_rate = sio.read_wav(os.path.join(GOLD, "sample.wav"))
        d_smp, d_rate = sio.read_wav(os.path.join(GOLD, "Section_7_1.wav"))
        whole = Sound(t_smp, t_rate, frame_features(t_smp, t_rate, engine=e))
        seg = 16 * HOP
        cut_up = SoundDictionary.from_segments(whole, [seg] * (t_smp.size // seg), engine=e)
        # six segments of 16 frames across the recording, and one that has samples but no frames: no spot
        self.targets = cut_up.sounds[::48][:6] + [Sound(np.linspace(-0.2, 0.2, 700), t_rate, np.zeros(0))]
        rec = Sound(d_smp, d_rate, frame_features(d_smp, d_rate, engine=e), "Section_7_1")
        # the second recording ends in the middle of a frame, so a span at its end has a short last frame
        part = Sound(d_smp[:300 * HOP - 90], d_rate, rec.mfcc_arrays()[:300].reshape(-1).copy(), "head")
        self.d = SoundDictionary(engine=e)
        self.d.sounds = [part, rec]
        self.spots = {step: self.d.spot(self.targets, step=step) for step in ("symmetric", "paced")}
        # ... and spans chosen by hand: the end of the short recording, a one-frame span, an empty Spot in the middle
        self.by_hand = [Spot(0, 280, 299, 0.0), Spot(1, 1980, 1980, 0.0), Spot.none(), Spot(1, 0, 40, 0.0), Spot(0, 0, 0, 0.0),
                        Spot(1, 1000, 1030, 0.0), Spot(0, 100, 110, 0.0)]
        self.order = np.arange(len(self.targets))

    def close(self):
        self.e.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _spot_sets(world, step):
    return (("spotted", world.spots[step]), ("by hand", world.by_hand))


def test_the_spots_are_what_the_test_needs(world):
    for step in ("symmetric", "paced"):
        spots = world.spots[step]
        assert len(spots) == 7 and all(spots[:6]) and not spots[6]
        assert all(sp.num_frames() >= 1 for sp in spots[:6])


@pytest.mark.parametrize("step", ["symmetric", "paced"])
def test_align_spans_equals_the_cut_route(world, step):
    for what, spots in _spot_sets(world, step):
        got = world.d.align(world.targets, spans=spots, step=step)
        want = world.d.cut(spots).align(world.targets, indices=world.order, step=step)
        for t, (g, w, sp) in enumerate(zip(got, want, spots)):
            assert _bits(g.cost) == _bits(w.cost), (what, t)
            assert np.array_equal(g.path, w.path) and np.array_equal(g.frame_map, w.frame_map), (what, t)
            assert g.source_index == sp.source_index and g.span_start == (sp.start_frame if sp else 0)
            if len(g):
                assert g.frame_map[0] == 0 and g.path[-1][0] == sp.num_frames() - 1
                assert g.span_start + int(g.frame_map.max()) <= sp.end_frame      # frames of the recording
            if what == "spotted" and sp:
                assert _bits(g.cost) == _bits(sp.cost)                              # the spot's bits
        assert len(got[6 if what == "spotted" else 2]) == 0                         # the empty Spot: an empty Alignment
        assert sum(len(g) > 0 for g in got) >= 2


@pytest.mark.parametrize("search", [0, 64])
@pytest.mark.parametrize("step", ["symmetric", "paced"])
def test_warp_spans_equals_the_cut_route(world, step, search):
    for what, spots in _spot_sets(world, step):
        kw = dict(want_pcm32=True, search=search, step=step, want_pos=bool(search))
        got = world.d.warp(world.targets, spans=spots, **kw)
        want = world.d.cut(spots).warp(world.targets, indices=world.order, **kw)
        assert len(got) == len(want) == (4 if search else 2)
        assert np.array_equal(_bits(got[0]), _bits(want[0])), (what, step, search)
        for g, w in zip(got[1:], want[1:]):
            assert np.array_equal(g, w), (what, step, search)
        # an empty Spot: zeros of the target's length (an empty sound's length fit)
        t = 6 if what == "spotted" else 2
        off = np.concatenate([[0], np.cumsum([x.samples().size for x in world.targets])])
        assert not got[0][off[t]:off[t + 1]].any() and got[0].size == off[-1]
        assert got[0].any()


@pytest.mark.parametrize("search", [0, 64])
@pytest.mark.parametrize("step", ["symmetric", "paced"])
def test_reconstruct_spotted_equals_the_cut_route(world, step, search):
    spots, samples, pcm = world.d.reconstruct_spotted(world.targets, step=step, search=search, want_pcm32=True)
    assert [(s.source_index, s.start_frame, s.end_frame, _bits(s.cost)) for s in spots] == \
           [(s.source_index, s.start_frame, s.end_frame, _bits(s.cost)) for s in world.spots[step]]
    assert [s.cost_per_frame for s in spots] == [s.cost_per_frame for s in world.spots[step]]
    want, want_pcm = world.d.cut(spots).warp(world.targets, indices=world.order, want_pcm32=True, search=search, step=step)
    assert np.array_equal(_bits(samples), _bits(want)) and np.array_equal(pcm, want_pcm)
    again = SoundSequence.new(world.targets).reconstruct_spotted_from_dictionary(world.d, step=step, search=search)
    assert len(again) == 2 and np.array_equal(_bits(again[1]), _bits(want))


def test_context_differs_only_where_a_tap_crosses_the_spans_end(world):
    spots = world.by_hand
    plain = world.d.warp(world.targets, spans=spots)
    wide = world.d.warp(world.targets, spans=spots, context=True)
    al = world.d.align(world.targets, spans=spots)
    off = np.concatenate([[0], np.cumsum([x.samples().size for x in world.targets])])
    crossing = np.zeros(plain.size, dtype=bool)
    for t, (a, sp) in enumerate(zip(al, spots)):
        if not len(a):
            continue                                                                # the length fit reads the span alone
        size = world.d.sounds[sp.source_index].samples().size
        first, end = sp.sample_span(size)
        k = np.arange(off[t + 1] - off[t])
        for back in range(4):                                                       # the four taps of an output sample
            j = k // HOP - back
            ok = (j >= 0) & (j < a.frame_map.size)
            p = a.frame_map[np.clip(j, 0, a.frame_map.size - 1)].astype(np.int64) * HOP + (k - j * HOP)
            crossing[off[t]:off[t + 1]] |= ok & (p >= end - first) & (p < size - first)
    same = _bits(plain) == _bits(wide)
    assert same[~crossing].all()                                                    # nothing else changes
    assert crossing.any() and (~same[crossing]).any()                               # ... and the continuation is heard
    # with a search the positions near the span's start stay put as well: their templates and candidates end inside the span
    s_plain, p_plain, m_off = world.d.warp(world.targets, spans=spots, search=64, want_pos=True)
    s_wide, p_wide, _ = world.d.warp(world.targets, spans=spots, search=64, want_pos=True, context=True)
    assert p_plain.shape == p_wide.shape and not np.array_equal(_bits(s_plain), _bits(s_wide))
    at = int(m_off[3])                                                              # frames 0 ... 40 of the long recording
    assert np.array_equal(p_plain[at:at + 3], p_wide[at:at + 3]) and p_plain[at + 2] + 3 * HOP + 1024 + 64 < 41 * HOP

@pytest.mark.parametrize("paced", [False, True])
def test_the_spot_example_writes_what_the_cut_route_gives(world, tmp_path, monkeypatch, capsys, paced):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import spot as example
    finally:
        sys.path.pop(0)
    seen = {}
    real = SoundDictionary.warp

    def warp(self, targets, *a, **kw):
        if "spans" in kw:
            seen["args"] = (self, list(targets), list(kw["spans"]), {k: v for k, v in kw.items() if k != "spans"})
        return real(self, targets, *a, **kw)

    monkeypatch.setattr(SoundDictionary, "warp", warp)
    out = str(tmp_path / "out.wav")
    argv = ["-s", os.path.join(GOLD, "sample.wav"), "-d", os.path.join(GOLD, "Section_7_1.wav"), "-o", out, "--search", "32"]
    samples = example.main(argv + (["--paced"] if paced else []))
    d, targets, spots, kw = seen["args"]
    assert kw["search"] == 32 and kw.get("step", "symmetric") == ("paced" if paced else "symmetric") and len(targets) > 20
    want, want_pcm = d.cut(spots).warp(targets, indices=np.arange(len(targets)), **kw)
    assert np.array_equal(_bits(samples), _bits(want))
    sio.write_wav32(str(tmp_path / "want.wav"), sample_rate=targets[0].sample_rate(), pcm=want_pcm)
    assert open(out, "rb").read() == open(str(tmp_path / "want.wav"), "rb").read()
    printed = capsys.readouterr().out
    assert printed.count("segment ") == len(targets) and ("mean cost_per_frame" in printed) == paced
