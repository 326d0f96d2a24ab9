"""Span alignment and sample windows restated on the CPU -- TEST INFRASTRUCTURE (include/soundsym_amd.h "Span alignment"
and "Sample windows", DESIGN.md section 2 "Spans").

Both are defined by reduction, and so is this file: slice, then ask the restatement of the existing call.

    align_one / align_spans     frames first ... last of a segment against a target: tests/dtw_path_ref.py for the symmetric
                                pattern (band and squared option included), tests/paced_path_ref.py for the paced one.  Cells
                                and maps count from the span's first frame.
    slices                      samples first ... first + len - 1 of sound idx[t], one array per target
    warp_spans / wsola_spans    tests/warp_ref.py / tests/wsola_ref.py on a store made of the slices, sound t for target t
    align_status / window_status   the error and limit table: what a call answers before any device work

Nothing here looks outside a span or a window: the slices are copies."""
import numpy as np

import dtw_path_ref
import paced_path_ref
import warp_ref
import wsola_ref

NO_MATCH = 0xFFFFFFFF
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -6

MAX_FRAMES = 4096               # frames of a span and of a target
MAX_PACED_TARGET = 2048         # frames of a target under the paced pattern
MAX_DIM = 64
HOP = 256

NO_PATH = (float("inf"), np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64))


def span_kind(first, last, seg_frames, src=0):
    """"none": no path (a spot without a span, or no source); "ok"; "invalid"."""
    if src == NO_MATCH:
        return "none"
    if first == NO_MATCH and last == NO_MATCH:
        return "none"
    if first == NO_MATCH or last == NO_MATCH or first > last or last >= seg_frames:
        return "invalid"
    return "ok"


def align_status(seg_frames, tgt_frames, spans, dim, step="symmetric", metric="dtw", band=-1):
    """What ssym_dtw_align_spans answers for pairs (segment p, target p): spans is a list of (first, last) or
    (src, first, last).  E_INVALID comes first (a bad span), then the limits, which hold for the SPAN."""
    if metric != "dtw" or (step == "paced" and band >= 0):
        return E_UNSUPPORTED
    shapes = []
    for p, sp in enumerate(spans):
        src, first, last = (0,) + tuple(sp) if len(sp) == 2 else sp
        kind = span_kind(first, last, seg_frames[p], src)
        if kind == "invalid":
            return E_INVALID
        if kind == "ok" and tgt_frames[p] > 0:
            shapes.append((last - first + 1, tgt_frames[p]))
    for fa, fb in shapes:
        if fa > MAX_FRAMES or fb > MAX_FRAMES or dim > MAX_DIM or (step == "paced" and fb > MAX_PACED_TARGET):
            return E_UNSUPPORTED
    return OK


def window_status(sound_samples, idx, win_first, win_len):
    """What the two window calls answer for their windows, the existing call's own checks aside."""
    for t, s in enumerate(idx):
        if int(win_first[t]) + int(win_len[t]) > sound_samples[int(s)]:
            return E_INVALID
    return OK


def sizes(tgt_frames, spans):
    """(path offsets, map offsets) of ssym_dtw_align_spans_sizes: Fa' + Fb - 1 cells and Fb map entries per pair with frames."""
    p_off, m_off = [0], [0]
    for p, sp in enumerate(spans):
        src, first, last = (0,) + tuple(sp) if len(sp) == 2 else sp
        has = span_kind(first, last, 1 << 62, src) == "ok" and tgt_frames[p] > 0
        p_off.append(p_off[-1] + (last - first + tgt_frames[p] if has else 0))
        m_off.append(m_off[-1] + (tgt_frames[p] if has else 0))
    return np.array(p_off, dtype=np.uint64), np.array(m_off, dtype=np.uint64)


def align_one(seg, tgt, first, last, step="symmetric", band=-1, squared=False, src=0):
    """(cost, path (L, 2) int64, map (Fb,) int64) of the span against the target, relative to the span."""
    seg, tgt = np.asarray(seg, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    kind = span_kind(first, last, seg.shape[0], src)
    assert kind != "invalid", (first, last, seg.shape[0])
    if kind == "none" or tgt.shape[0] == 0:
        return NO_PATH
    cut = seg[first:last + 1].copy()
    if step == "paced":
        assert band < 0
        return paced_path_ref.align(cut, tgt, squared=squared)
    return dtw_path_ref.align(cut, tgt, band=band, squared=squared)


def align_spans(segs, tgts, spans, step="symmetric", band=-1, squared=False):
    """align_one for pairs (segment p, target p)."""
    out = []
    for p, sp in enumerate(spans):
        src, first, last = (0,) + tuple(sp) if len(sp) == 2 else sp
        out.append(align_one(segs[p], tgts[p], first, last, step, band, squared, src))
    return out


def slices(sounds, idx, win_first, win_len):
    return [np.asarray(sounds[int(s)], dtype=np.float64)[int(a):int(a) + int(n)].copy()
            for s, a, n in zip(idx, win_first, win_len)]


def warp_spans(sounds, idx, win_first, win_len, out_offsets, maps, map_offsets, map_frames, pair_len=None):
    cut = slices(sounds, idx, win_first, win_len)
    return warp_ref.warp(cut, np.arange(len(cut)), out_offsets, maps, map_offsets, map_frames, pair_len)


def wsola_spans(sounds, idx, win_first, win_len, out_offsets, maps, map_offsets, map_frames, pair_len=None, search=0):
    cut = slices(sounds, idx, win_first, win_len)
    return wsola_ref.wsola(cut, np.arange(len(cut)), out_offsets, maps, map_offsets, map_frames, pair_len, search)


def sample_window(start_frame, end_frame, num_samples, context=False):
    """(first, len) of a spot's frames in a recording of num_samples samples: Spot.sample_span's, or with context up to the
    recording's end."""
    a = min(start_frame * HOP, num_samples)
    b = num_samples if context else min((end_frame + 1) * HOP, num_samples)
    return a, max(b - a, 0)
