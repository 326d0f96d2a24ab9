"""tests/span_ref.py held to the references it reduces to, on planted cases: a span that is the target itself, spans at both
ends of the paced shape rule, windows whose content is known sample by sample, and the error and limit table."""
import numpy as np
import pytest

import dtw_path_ref
import paced_path_ref
import span_ref
import warp_ref
import wsola_ref

NO = span_ref.NO_MATCH
bits = lambda v: np.asarray(v, dtype=np.float64).view(np.uint64)


def _recording(frames=40, dim=5, seed=0x51A):
    return np.random.default_rng(seed).normal(size=(frames, dim))


@pytest.mark.parametrize("step", ["symmetric", "paced"])
def test_a_span_that_is_the_target_aligns_on_the_diagonal_at_cost_zero(step):
    rec = _recording()
    tgt = rec[11:24].copy()
    cost, path, fmap = span_ref.align_one(rec, tgt, 11, 23, step)
    assert cost == 0.0 and np.array_equal(fmap, np.arange(13))                      # relative to the span: map[0] = 0
    assert np.array_equal(path, np.stack([np.arange(13), np.arange(13)], axis=1))
    # one frame further on each side: the recording's frames 10 and 24 join, the cost is that of the slice
    cost2, path2, fmap2 = span_ref.align_one(rec, tgt, 10, 24, step)
    ref = paced_path_ref.align(rec[10:25], tgt) if step == "paced" else dtw_path_ref.align(rec[10:25], tgt)
    assert bits(cost2) == bits(ref[0]) and np.array_equal(path2, ref[1]) and np.array_equal(fmap2, ref[2])
    assert cost2 > 0.0 and fmap2[0] == 0 and path2[-1][0] == 14


def test_frames_outside_the_span_do_not_count():
    rec = _recording()
    tgt = _recording(9, seed=0x51B)
    want = span_ref.align_one(rec, tgt, 5, 20)
    poisoned = rec.copy()
    poisoned[:5] = np.nan
    poisoned[21:] = np.nan
    got = span_ref.align_one(poisoned, tgt, 5, 20)
    assert bits(got[0]) == bits(want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert not np.isfinite(span_ref.align_one(poisoned, tgt, 4, 20)[0])             # ... and inside it they do


def test_the_band_and_the_squared_option_are_the_existing_calls():
    rec, tgt = _recording(), _recording(12, seed=0x51C)
    for kw in ({"band": 3}, {"squared": True}):
        got = span_ref.align_one(rec, tgt, 7, 20, **kw)
        want = dtw_path_ref.align(rec[7:21], tgt, **kw)
        assert bits(got[0]) == bits(want[0]) and np.array_equal(got[1], want[1])
    assert not np.isfinite(span_ref.align_one(rec, tgt, 0, 30, band=3)[0])          # 31 x 12 with band 3: no path


def test_the_paced_shape_rule_is_applied_to_the_span():
    rec, tgt = _recording(), _recording(9, seed=0x51D)                              # Fb = 9: Fa' in 5 ... 17
    for fa, feasible in ((4, False), (5, True), (17, True), (18, False)):
        assert paced_path_ref.feasible(fa, 9) == feasible
        cost, path, fmap = span_ref.align_one(rec, tgt, 3, 3 + fa - 1, "paced")
        assert np.isfinite(cost) == feasible and len(path) == (9 if feasible else 0)
        if feasible:
            assert fmap[0] == 0 and fmap[-1] == fa - 1 and paced_path_ref.admissible(fmap, fa)


def test_no_span_no_source_and_an_empty_target_give_no_path():
    rec, tgt = _recording(), _recording(9, seed=0x51E)
    for got in (span_ref.align_one(rec, tgt, NO, NO), span_ref.align_one(rec, tgt, 2, 9, src=NO),
                span_ref.align_one(rec, tgt[:0], 2, 9)):
        assert got[0] == np.inf and len(got[1]) == 0 and len(got[2]) == 0
    p_off, m_off = span_ref.sizes([9, 9, 0, 9], [(2, 9), (NO, NO), (2, 9), (NO, 2, 9)])
    assert p_off.tolist() == [0, 8 + 9 - 1, 16, 16, 16] and m_off.tolist() == [0, 9, 9, 9, 9]


def test_the_error_and_limit_table():
    st = span_ref.align_status
    assert st([300], [10], [(17, 80)], 13) == span_ref.OK
    assert st([300], [10], [(81, 80)], 13) == span_ref.E_INVALID                    # first > last
    assert st([300], [10], [(0, 300)], 13) == span_ref.E_INVALID                    # last >= the segment's frames
    assert st([300], [10], [(NO, 5)], 13) == st([300], [10], [(5, NO)], 13) == span_ref.E_INVALID
    assert st([300], [10], [(NO, NO)], 13) == span_ref.OK
    assert st([300], [10], [(NO, 400, 2)], 13) == span_ref.OK                       # no source: its span is not looked at
    assert st([5000], [8], [(0, 4095)], 13) == span_ref.OK                          # the limits hold for the span ...
    assert st([5000], [8], [(0, 4096)], 13) == span_ref.E_UNSUPPORTED
    assert st([5000], [8], [(4135, 4999)], 13) == span_ref.OK                       # ... not for the segment
    assert st([300], [4097], [(0, 9)], 13) == span_ref.E_UNSUPPORTED
    assert st([300], [2049], [(0, 9)], 13, step="paced") == span_ref.E_UNSUPPORTED
    assert st([300], [2049], [(0, 9)], 13) == span_ref.OK
    assert st([300], [10], [(0, 9)], 65) == span_ref.E_UNSUPPORTED
    assert st([300], [10], [(0, 9)], 13, metric="refcos") == span_ref.E_UNSUPPORTED
    assert st([300], [10], [(0, 9)], 13, step="paced", band=4) == span_ref.E_UNSUPPORTED
    assert st([300], [10], [(0, 9)], 13, band=4) == span_ref.OK
    assert st([300, 300], [10, 10], [(0, 4999), (5, 4)], 13) == span_ref.E_INVALID  # a bad span before a long one
    ws = span_ref.window_status
    assert ws([1000, 5], [0, 1, 0], [0, 5, 1000], [1000, 0, 0]) == span_ref.OK
    assert ws([1000, 5], [0], [1], [1000]) == span_ref.E_INVALID
    assert ws([1000, 5], [1], [6], [0]) == span_ref.E_INVALID


def _sounds():
    rng = np.random.default_rng(0x51F)
    return [rng.normal(size=n) * 0.3 for n in (5000, 1023, 1)]


def test_windows_are_the_existing_restatements_on_the_slices():
    sounds = _sounds()
    idx = np.array([0, 0, 1, 2, 0], dtype=np.uint32)
    first = np.array([768, 255, 0, 0, 4999], dtype=np.uint64)
    length = np.array([1280, 257, 1023, 0, 1], dtype=np.uint64)
    frames = np.array([5, 2, 4, 3, 1], dtype=np.uint32)
    moff = np.concatenate([[0], np.cumsum(frames)]).astype(np.uint64)
    maps = np.array([0, 1, 1, 3, 9, 0, 0, 0, 1, 2, 2, 0, 0, 0, 0], dtype=np.uint32)  # repeats, a skip, one past the window
    ooff = np.concatenate([[0], np.cumsum(frames.astype(np.int64) * 256 + 300)]).astype(np.uint64)
    cut = [s[int(a):int(a) + int(n)] for s, a, n in zip([sounds[i] for i in idx], first, length)]
    got = span_ref.warp_spans(sounds, idx, first, length, ooff, maps, moff, frames)
    assert np.array_equal(bits(got), bits(warp_ref.warp(cut, np.arange(5), ooff, maps, moff, frames)))
    got, pos = span_ref.wsola_spans(sounds, idx, first, length, ooff, maps, moff, frames, None, 7)
    want, want_pos = wsola_ref.wsola(cut, np.arange(5), ooff, maps, moff, frames, None, 7)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(pos, want_pos)
    # the content, sample by sample: target 2's map is the diagonal of a window that is the whole sound, so the first hop of
    # its output is the sound itself wherever a tap is valid
    o = int(ooff[2])
    assert np.allclose(span_ref.warp_spans(sounds, idx, first, length, ooff, maps, moff, frames)[o + 1:o + 256],
                       sounds[1][1:256], rtol=1e-12, atol=0)
    # samples outside a window never count: poison them
    poisoned = [s.copy() for s in sounds]
    poisoned[0][:255] = np.nan
    poisoned[0][2048:4999] = np.nan
    keep = (idx != 0) | (first >= 255)
    assert keep.all()
    again = span_ref.warp_spans(poisoned, idx, first, length, ooff, maps, moff, frames)
    assert np.array_equal(bits(again), bits(span_ref.warp_spans(sounds, idx, first, length, ooff, maps, moff, frames)))


def test_the_sample_window_of_a_spot():
    assert span_ref.sample_window(3, 5, 5000) == (768, 768)
    assert span_ref.sample_window(3, 5, 1400) == (768, 632)                         # the recording ends inside the span
    assert span_ref.sample_window(3, 5, 5000, context=True) == (768, 4232)
    assert span_ref.sample_window(30, 31, 5000) == (5000, 0)
