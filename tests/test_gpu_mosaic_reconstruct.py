"""SoundDictionary.reconstruct_mosaic on the GPU held to tests/span_ref.py's warp_spans / wsola_spans on the same maps, bit for
bit, on two short synthetic recordings: the Mosaic is the restatement's, every sounding piece is resynthesised from its
span's window along frame_map - source_first, and the gap's stretch is zeros or the target's own samples."""
import numpy as np
import pytest

import mirror_cases as mc
import mosaic_ref as ref
import span_ref
from soundsym_amd import HOP, Engine, Sound, SoundDictionary

pytestmark = pytest.mark.gpu

PLAN = ((1, 2, 6, "copy"), (0, 3, 5, "doubled"))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


@pytest.fixture(scope="module")
def world():
    """Two recordings of 9 and 8 frames x 12 values; the target is frames 2 ... 6 of recording 1, two frames far from
    everything, then frames 3 ... 5 of recording 0 with every frame doubled."""
    class W:
        pass
    w = W()
    rng = np.random.default_rng(0x3051)
    w.recs = [ref._real(rng, (9, 12)), ref._real(rng, (8, 12))]
    parts = [ref._span(w.recs[s], a, b, kind) for s, a, b, kind in PLAN]
    w.x = np.concatenate([parts[0], ref._real(rng, (2, 12)) + 100.0, parts[1]], axis=0)
    w.rec_smp = [rng.standard_normal(a.shape[0] * HOP + 100) * 0.1 for a in w.recs]
    w.tgt_smp = rng.standard_normal(w.x.shape[0] * HOP + 37) * 0.1
    w.e = Engine(metric="dtw", dtype="f64")
    w.D = SoundDictionary(engine=w.e)
    w.D.sounds = [Sound(s, mc.RATE, a.reshape(-1)) for s, a in zip(w.rec_smp, w.recs)]
    w.target = Sound(w.tgt_smp, mc.RATE, w.x.reshape(-1))
    w.want = ref.arrays(w.recs, [w.x], 1.0, 1.5)
    yield w
    w.e.close()


def _expected(w, mosaic, search, gap_fill):
    """The samples by the restatement of the window calls on the Mosaic's own pieces."""
    n = w.tgt_smp.size
    lengths = mosaic.segment_lengths(n)
    sounding = [(p, m) for p, m in zip(mosaic.pieces, lengths) if not p.is_gap]
    idx = [p.source_index for p, _ in sounding]
    first = [p.source_first * HOP for p, _ in sounding]
    length = [min((p.source_last + 1) * HOP, w.rec_smp[p.source_index].size) - p.source_first * HOP for p, _ in sounding]
    o_off = np.concatenate([[0], np.cumsum([m for _, m in sounding])]).astype(np.uint64)
    frames = np.array([p.num_frames() for p, _ in sounding], dtype=np.uint32)
    m_off = np.concatenate([[0], np.cumsum(frames)]).astype(np.uint64)
    maps = np.concatenate([p.frame_map - p.source_first for p, _ in sounding]).astype(np.uint32)
    if search:
        warped, _ = span_ref.wsola_spans(w.rec_smp, idx, first, length, o_off, maps, m_off, frames, None, search)
    else:
        warped = span_ref.warp_spans(w.rec_smp, idx, first, length, o_off, maps, m_off, frames, None)
    out, at, took = np.zeros(n), 0, 0
    for p, m in zip(mosaic.pieces, lengths):
        if not p.is_gap:
            out[at:at + m] = warped[took:took + m]
            took += m
        elif gap_fill == "target":
            out[at:at + m] = w.tgt_smp[at:at + m]
        at += m
    return out


def test_the_mosaic_is_the_restatements(world):
    m = world.D.mosaic([world.target], 1.0, 1.5)[0]
    tiles = [(ref.GAP, p.start_frame, p.end_frame) if p.is_gap else
             (p.source_index, p.source_first, p.source_last, p.start_frame, p.end_frame) for p in m.pieces]
    assert tiles == [(1, 2, 6, 0, 4), (ref.GAP, 5, 6), (0, 3, 5, 7, 12)]
    assert _bits(m.total)[0] == _bits(world.want[1][0])[0] and m.total == 5.0
    assert np.array_equal(_bits(m.frame_costs), _bits(world.want[5]))
    assert m.pieces[2].frame_map.tolist() == [3, 3, 4, 4, 5, 5] and m.gaps[0].cost == 3.0


@pytest.mark.parametrize("search,gap_fill", [(0, "silence"), (0, "target"), (7, "silence")])
def test_reconstruct_mosaic_against_the_window_restatement(world, search, gap_fill):
    m, out, pcm = world.D.reconstruct_mosaic(world.target, 1.0, 1.5, gap_fill, search, want_pcm32=True)
    assert out.size == world.tgt_smp.size == pcm.size and len(m.sounding) == 2
    want = _expected(world, m, search, gap_fill)
    assert np.array_equal(_bits(out), _bits(want))
    a, b = m.gaps[0].sample_span(out.size)
    assert (out[a:b] == (0.0 if gap_fill == "silence" else world.tgt_smp[a:b])).all()
    assert np.abs(out[:a]).max() > 0 and np.abs(out[b:]).max() > 0
    plain = world.D.reconstruct_mosaic(world.target, 1.0, 1.5, gap_fill, search)
    assert len(plain) == 2 and np.array_equal(_bits(plain[1]), _bits(out))


def test_a_target_without_a_mosaic_is_silence(world):
    bad = world.x.copy()
    bad[3, 0] = float("nan")
    m, out = world.D.reconstruct_mosaic(Sound(world.tgt_smp, mc.RATE, bad.reshape(-1)), 1.0)
    assert not m and m.total == float("inf") and out.size == world.tgt_smp.size and not out.any()
