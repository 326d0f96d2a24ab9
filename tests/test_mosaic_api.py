"""The surface of the mosaic without a device: Mosaic and MosaicPiece assembled from the six arrays of ssym_dtw_mosaic (the
restatement's, tests/mosaic_ref.py), gap frames merged into maximal runs, piece costs as chains of frame_cost, the
ValueErrors that come before any library call, and header, binding, Rust declaration and C++ mirror holding to each other."""
import os
import re

import numpy as np
import pytest

import mosaic_ref as ref
import soundsym_amd
from soundsym_amd import HOP, Gap, Mosaic, MosaicPiece, Sound, SoundDictionary
from soundsym_amd import _native as nat
from soundsym_amd import api as api_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ssym_dtw_mosaic"
INF = float("inf")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


def test_header_binding_rust_and_mirror_name_the_symbol(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    args = ["ctx", "dict", "q", "piece_penalty", "gap_cost", "flags", "out_count", "out_total", "out_start", "out_src",
            "out_frame", "out_frame_cost"]
    assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % NAME, header)
    assert NAME in nat.ABI_SYMBOLS and NAME in soundsym_amd.ABI_SYMBOLS
    assert hasattr(native_lib, NAME) and len(getattr(native_lib, NAME).argtypes) == len(args)
    assert names(header, NAME + "(ssym_ctx") == args
    assert args == re.findall(r"(\w+):", rust[rust.index("pub fn %s" % NAME):].split(";")[0])
    assert NAME + "(ctx_->get()" in mirror
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header       # additions only
    assert "dtw_mosaic.hip" in _read("soundsym_amd", "csrc", "Makefile")


def test_header_states_the_definition():
    header = _read("include", "soundsym_amd.h")
    doc = header[header.index("Mosaic (DESIGN.md"):header.index(NAME + "(ssym_ctx")]
    for line in ("S      = piece_penalty + best(j-1)", "open(g)= not (P(g) <= S)", "H(g,j) = c(g,j) + N(g,j-1)",
                 "vg     = gap_cost + best(j-1)", "a piece never crosses a segment boundary", "Every output may be NULL",
                 "(SSYM_COVER_GAP, SSYM_NO_MATCH, gap_cost)", "SSYM_E_EMPTY_DICT"):
        assert line in doc, line


def test_null_context_is_refused_without_a_device(native_lib):
    u, f = np.full(4, 7, dtype=np.uint32), np.full(4, -1.5)
    for gap in (0.0, -1.0, float("nan"), INF):
        rc = native_lib.ssym_dtw_mosaic(None, None, None, 0.0, gap, 0, u.ctypes.data, f.ctypes.data, u.ctypes.data, u.ctypes.data,
                                        u.ctypes.data, f.ctypes.data)
        assert rc == nat.SSYM_E_INVALID
    assert (u == 7).all() and (f == -1.5).all()


# -- assembly from the six arrays ----------------------------------------------------------------------------------------

def _chain(costs):
    acc = float(costs[0])
    for c in costs[1:]:
        acc = float(c) + acc
    return acc


def test_mosaics_from_the_arrays_of_the_intruder_case():
    recs, x, planted, (first, last) = ref.intruder_case()
    targets = [x, x[:0], x[first:last + 1], x[:3]]
    got = ref.arrays(recs, targets, 1.0, 1.5)
    off = np.concatenate([[0], np.cumsum([t.shape[0] for t in targets])])
    ms = api_mod._mosaics(off, *got)
    assert [bool(m) for m in ms] == [True, False, True, True] and [m.num_frames for m in ms] == [26, 0, 4, 3]
    m = ms[0]
    assert [p.is_gap for p in m.pieces] == [False, True, False] and len(m) == 3
    a, g, b = m.pieces
    assert (a.source_index, a.source_first, a.source_last, a.start_frame, a.end_frame) == planted[0]
    assert (b.source_index, b.source_first, b.source_last, b.start_frame, b.end_frame) == planted[1]
    assert (g.start_frame, g.end_frame, g.cost, g.cost_per_frame) == (first, last, 6.0, 1.5)        # ONE run of four frames
    assert b.frame_map.tolist() == [20, 20, 21, 21, 22, 22, 23, 23, 24, 24, 25, 25] and b.frame_map.dtype == np.int64
    assert m.total == 8.0 and m.total_per_frame == 8.0 / 26 and m.sounding == [a, b] and m.gaps == [g]
    assert np.array_equal(_bits(m.frame_costs), _bits(got[5][:26]))
    assert ms[1].total == INF and ms[1].total_per_frame == INF and not ms[1].pieces and "empty" in repr(ms[1])
    assert [p.is_gap for p in ms[2].pieces] == [True] and ms[2].total == 6.0
    assert "2 pieces, 1 gaps" in repr(m) and "source frames=5...14" in repr(a)


def test_piece_costs_are_chains_of_frame_costs():
    recs, x, _ = ref.planted_case(1e-3)
    got = ref.arrays(recs, [x], 1.0, 0.7)
    m = api_mod._mosaics([0, x.shape[0]], *got)[0]
    assert len(m.sounding) >= 3
    acc = 0.0
    for p in m.pieces:
        fc = m.frame_costs[p.start_frame:p.end_frame + 1]
        if p.is_gap:
            assert (fc == 0.7).all() and p.cost == 0.7 * p.num_frames()
            for c in fc:
                acc = float(c) + acc
            continue
        assert _bits(p.cost)[0] == _bits(_chain(fc))[0] and p.cost_per_frame == p.cost / p.num_frames()
        assert p.frame_map[0] == p.source_first and p.frame_map[-1] == p.source_last and p.frame_map.size == p.num_frames()
        acc = float(fc[0]) + (1.0 + acc)
        for c in fc[1:]:
            acc = float(c) + acc
    assert _bits(acc)[0] == _bits(m.total)[0]                # consequence (2) through the objects


def test_gap_frames_merge_into_maximal_runs():
    start = np.array([0, 1, 2, 4, 5, 6], dtype=np.uint32)
    src = np.array([ref.GAP, ref.GAP, 3, 3, ref.GAP, 0, 0], dtype=np.uint32)
    frame = np.array([ref.NONE, ref.NONE, 7, 9, ref.NONE, 0, 0], dtype=np.uint32)
    cost = np.array([0.5, 0.5, 1.0, 2.0, 0.5, 4.0, 8.0])
    tiles = api_mod._mosaic_tiles(start, src, frame, cost)
    assert [(t.is_gap, t.start_frame, t.end_frame, t.cost) for t in tiles] == [
        (True, 0, 1, 1.0), (False, 2, 3, 3.0), (True, 4, 4, 0.5), (False, 5, 5, 4.0), (False, 6, 6, 8.0)]
    assert tiles[1].frame_map.tolist() == [7, 9] and (tiles[1].source_first, tiles[1].source_last) == (7, 9)
    Mosaic(tiles, 1.0, 7, cost)


def test_mosaic_and_piece_checks():
    p = MosaicPiece(2, 4, 6, 10, 13, 2.0, [4, 4, 5, 6])
    assert p.num_frames() == 4 and p.cost_per_frame == 0.5 and not p.is_gap
    assert p.sample_span(100 * HOP) == (10 * HOP, 14 * HOP) and p.sample_span(14 * HOP - 5) == (10 * HOP, 14 * HOP - 5)
    assert p.source_sample_span(100 * HOP) == (4 * HOP, 7 * HOP) and p.source_sample_span(7 * HOP - 9) == (4 * HOP, 7 * HOP - 9)
    for bad in ([4, 4, 4, 6], [4, 5, 8, 6], [4, 5, 6], [5, 5, 6, 6], [4, 6, 5, 6]):
        with pytest.raises(ValueError):
            MosaicPiece(2, 4, 6, 10, 13, 2.0, bad)
    with pytest.raises(ValueError):
        MosaicPiece(2, 4, 4, 3, 2, 0.0, [4])
    q = MosaicPiece(0, 0, 0, 0, 0, 1.0, [0])
    with pytest.raises(ValueError):
        Mosaic([q, Gap(2, 2, 1.0)], 2.0, 3)                  # a hole
    with pytest.raises(ValueError):
        Mosaic([q, Gap(1, 1, 1.0), Gap(2, 2, 1.0)], 3.0, 3)  # a gap after a gap
    with pytest.raises(ValueError):
        Mosaic([q], 1.0, 2)                                  # does not end with the target
    with pytest.raises(ValueError):
        Mosaic([q], 1.0, 1, [1.0, 2.0])
    m = Mosaic([q, Gap(1, 2, 1.0)], 2.0, 3, [1.0, 0.5, 0.5])
    assert m.segment_lengths(3 * HOP + 11) == [HOP, 2 * HOP + 11] and Mosaic.none(4).segment_lengths(10) == []


def test_value_errors_come_before_any_library_call(monkeypatch):
    calls = []
    monkeypatch.setattr(nat, "lib", lambda: calls.append(1) or pytest.fail("a library call"))
    d = SoundDictionary.__new__(SoundDictionary)
    for penalty, gap in ((-1.0, None), (float("nan"), None), (INF, None), (0.0, -1.0), (0.0, float("nan"))):
        with pytest.raises(ValueError):
            SoundDictionary.reconstruct_mosaic(d, None, penalty, gap)
    with pytest.raises(ValueError):
        SoundDictionary.reconstruct_mosaic(d, None, 1.0, None, "noise")
    with pytest.raises(ValueError):
        SoundDictionary.reconstruct_mosaic(d, [1, 2], 1.0)
    with pytest.raises(ValueError):
        SoundDictionary.reconstruct_mosaic(d, None, 1.0, search=-1)
    assert not calls
