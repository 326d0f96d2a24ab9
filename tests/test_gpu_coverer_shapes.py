"""The coverer at the smallest shapes at which each of its mechanisms can go wrong: every W the forward geometry treats
differently, pushes around W, streams that wrap the ring of best values and the ring of back-pointers, slices, a store that
grows, the cover's geometry hooks, empty segments, a long stream, and cover_long against cover.  Everything is compared bit
for bit with tests/live_cover_ref.py (coverer_gpu.Live does that at every call)."""
import numpy as np
import pytest

import coverer_gpu as cg
import live_cover_cases as cases
import live_cover_ref as ref
from soundsym_amd import HOP, Sound, SoundDictionary

pytestmark = pytest.mark.gpu

LENS8 = [3, 1, 8, 2, 5, 4, 7, 1, 6, 8, 2, 3]


def _case(seed, fmax, T, dim=2):
    """A 1-frame segment (every frame has a cover), the longest one and two between; the target is made of them."""
    lens = sorted({1, max(fmax // 3, 1), max(fmax - 1, 1), fmax})
    return cases.random_case(seed, lens, T, dim=dim, noise=0.05)


@pytest.mark.parametrize("fmax", [1, 2, 8, 40, 64, 65, 128])
def test_every_width_with_pushes_around_w(fmax):
    W = 2 * fmax
    sizes = [0, 1, W - 1, W, W + 1, 1, 0, 3]
    segs, x = _case(0x5A0 + fmax, fmax, sum(sizes))
    with cg.Dict(segs, 2) as D:
        live = cg.Live(D, 1, 0.5)
        at = 0
        for m in sizes:
            live.push([x[at:at + m]])
            at += m
        live.flush()
        cg.same_pieces(live.emitted[0], cg.offline(D, x, 0.5)[0])
        assert fmax <= 2 or max(p[2] - p[1] + 1 for p in live.emitted[0]) > 2    # long pieces are in it
        live.close()


def test_one_push_of_600_frames_and_rings_that_wrap():
    segs, x = cases.random_case(0x600, LENS8, 1300)
    with cg.Dict(segs, 3) as D:
        live = cg.Live(D, 2, 0.0)
        live.push([x[:600], x[600:607]])                 # W = 16: one push far beyond the ring of 512 best values
        at = [600, 607]
        while at[1] < 1300:                              # lane 1 passes 512 frames in pushes of 7
            live.push([x[at[0]:min(at[0] + 3, 640)], x[at[1]:at[1] + 7]])
            at = [min(at[0] + 3, 640), min(at[1] + 7, 1300)]
        assert live.cv.counts()[0].tolist() == [640, 700]
        live.flush(0)
        live.flush(1)
        cg.same_pieces(live.emitted[0], cg.offline(D, x[:640], 0.0)[0])
        cg.same_pieces(live.emitted[1], cg.offline(D, x[600:], 0.0)[0])
        live.close()


@pytest.mark.parametrize("slice_frames", [1, 7, 16])
def test_slices_give_what_one_slice_gives(slice_frames):
    segs, x = cases.random_case(0x51C, LENS8, 160)
    cuts = [0, 40, 41, 100, 160]
    with cg.Dict(segs, 3) as D:
        whole = cg.Live(D, 2, 2.0)
        for a, b in zip(cuts[:-1], cuts[1:]):
            whole.push([x[a:b], x[a // 2:b // 2]])
        with cg.hooks(SSYM_COVERER_SLICE=slice_frames):
            sliced = cg.Live(D, 2, 2.0)
            for a, b in zip(cuts[:-1], cuts[1:]):
                got = sliced.push([x[a:b], x[a // 2:b // 2]], slice_frames)
                launches = D.e.timings()["main_launches"]
                assert launches == -(-(b - a) // slice_frames)                   # the call ran that many slices
        assert sliced.emitted == whole.emitted and len(whole.emitted[0]) > 10
        for l in (0, 1):
            sliced.flush(l)
        whole.close()
        sliced.close()


def test_a_small_store_grows_and_wraps():
    segs, x = cases.random_case(0xBAC, LENS8, 300)
    with cg.Dict(segs, 3) as D:
        with cg.hooks(SSYM_COVERER_BACK=8):
            live = cg.Live(D, 2, 20.0)                   # a high penalty: long pieces, long uncommitted stretches
        assert live.cv.counts()[1] == 8
        caps = []
        for a in range(0, 300, 5):
            live.push([x[a:a + 5], x[a:a + 3]])
            caps.append(live.cv.counts()[1])
            assert caps[-1] == ref.capacity(live.needs, 8)
        assert 8 < caps[-1] <= 256 and caps == sorted(caps) and caps[0] < caps[-1]
        live.push([x[:0], x[3:30]])                      # one push larger than the store
        assert live.cv.counts()[1] == ref.capacity(live.needs, 8)
        live.flush(0)
        cg.same_pieces(live.emitted[0], cg.offline(D, x, 20.0)[0])
        live.close()


@pytest.mark.parametrize("knobs", [dict(SSYM_COVER_STARTS=2), dict(SSYM_COVER_STARTS=128, SSYM_COVER_STRIP=1),
                                   dict(SSYM_COVER_STRIP=3, SSYM_COVER_BLOCK=1), dict(SSYM_COVER_BLOCK=5, SSYM_COVERER_SLICE=9)])
def test_the_covers_geometry_hooks(knobs):
    segs, x = cases.random_case(0x6E0, LENS8, 150)
    with cg.Dict(segs, 3) as D:
        with cg.hooks(**knobs):
            live = cg.Live(D, 1, 2.0)
            for a in range(0, 150, 25):
                live.push([x[a:a + 25]], knobs.get("SSYM_COVERER_SLICE", 1 << 40))
            live.flush()
        cg.same_pieces(live.emitted[0], cg.offline(D, x, 2.0)[0])
        live.close()


def test_a_dictionary_with_empty_segments():
    segs, x = cases.random_case(0xE3F, [0, 3, 0, 0, 5, 1, 0], 120)
    with cg.Dict(segs, 3) as D:
        live = cg.Live(D, 1, 0.0)
        for a in range(0, 120, 11):
            live.push([x[a:a + 11]])
        live.flush()
        assert live.emitted[0] and {p[0] for p in live.emitted[0]} <= {1, 4, 5}
        cg.same_pieces(live.emitted[0], cg.offline(D, x, 0.0)[0])
        live.close()
    with cg.Dict([np.zeros((0, 3))] * 3, 3) as D:        # nothing but empty segments: W = 2, no frame has a cover
        live = cg.Live(D, 1, 0.0)
        live.push([x[:5]])
        assert live.flush() == [] and live.cv.best()[0][0] == float("inf")
        live.close()


def test_5000_frames_in_pushes_of_16():
    segs, x = cases.random_case(0x5000, LENS8, 5000)
    with cg.Dict(segs, 3) as D:
        live = cg.Live(D, 1, 2.0)
        for a in range(0, 5000, 16):
            live.push([x[a:a + 16]], check_best=a % 800 == 0)
        cap = live.check_best()
        # consequence 7: the capacity follows from the uncommitted stretches alone, and they stay far below the stream
        assert cap == ref.capacity(live.needs) == 1024 and max(live.needs) < 200
        live.flush()
        pieces, total = cg.offline(D, x, 2.0)
        cg.same_pieces(live.emitted[0], pieces)
        assert live.cv.best()[0].view(np.uint64)[0] == np.array([total]).view(np.uint64)[0] and len(pieces) > 300
        live.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cover_long_is_cover(dtype):
    segs, x = cases.random_case(0x10F6, LENS8, 300, dim=5)
    rng = np.random.default_rng(3)
    x = x + 1e-9 * rng.standard_normal(x.shape)          # not f32 values: an f32 engine rounds them, in both calls alike
    snd = lambda rows: Sound(np.zeros(rows.shape[0] * HOP), 8000.0, rows.reshape(-1), "s", ncoeffs=5)
    from soundsym_amd import Engine
    e = Engine(metric="dtw", dtype=dtype)
    d = SoundDictionary(engine=e)
    d.sounds = [snd(a) for a in segs]
    target = snd(x)
    want = d.cover([target], 2.0)[0]
    for block in (4096, 64, 7):
        got = d.cover_long(target, 2.0, block)
        assert got.num_frames == want.num_frames == 300 and len(got) == len(want) > 20
        assert [(p.source_index, p.start_frame, p.end_frame) for p in got.pieces] == \
               [(p.source_index, p.start_frame, p.end_frame) for p in want.pieces]
        assert np.array([p.cost for p in got.pieces] + [got.total]).tobytes() == \
               np.array([p.cost for p in want.pieces] + [want.total]).tobytes()
    bad = x.copy()
    bad[200, 0] = float("nan")
    assert not d.cover_long(snd(bad), 2.0, 50) and not d.cover([snd(bad)], 2.0)[0]
    e.close()
