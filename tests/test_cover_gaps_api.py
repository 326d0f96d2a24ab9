"""The surface of the cover with gaps without a device: Gap and Cover arithmetic, the merging of gap frames into runs, the
ValueErrors that come before any library call, and header, binding, Rust declaration and C++ mirror holding to each other."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Cover, Gap, LiveCover, Piece, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat
from soundsym_amd import api as api_mod
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER, CREATE = "ssym_dtw_cover_gaps", "ssym_coverer_create_gaps"
INF = float("inf")
GAP = 0xFFFFFFFE


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbols(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    want = {COVER: ["ctx", "dict", "q", "piece_penalty", "gap_cost", "flags", "out_count", "out_total", "out_src", "out_start",
                    "out_end", "out_cost"],
            CREATE: ["ctx", "dict", "n_lanes", "piece_penalty", "gap_cost", "out"]}
    for name, args in want.items():
        assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % name, header)
        assert name in nat.ABI_SYMBOLS and name in soundsym_amd.ABI_SYMBOLS
        assert hasattr(native_lib, name) and len(getattr(native_lib, name).argtypes) == len(args)
        assert names(header, name + "(ssym_ctx") == args
        assert args == re.findall(r"(\w+):", rust[rust.index("pub fn %s" % name):].split(";")[0])
    assert COVER + "(ctx_->get()" in mirror
    assert "#define SSYM_COVER_GAP 0xFFFFFFFEu" in header and nat.COVER_GAP == GAP != nat.NO_MATCH
    assert re.search(r"pub const SSYM_COVER_GAP: u32 = 0xffff_fffe;", rust)
    assert "kCoverGap = 0xfffffffeu" in _read("soundsym_amd", "csrc", "dtw_cover_chain.hpp")
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header       # additions only


def test_header_states_the_definition():
    header = _read("include", "soundsym_amd.h")
    doc = header[header.index("Cover with gaps (DESIGN.md"):header.index(COVER + "(ssym_ctx")]
    for line in ("vg = gap_cost + best(e-1)", "if vg < v (strict)", "(L = 1, src = SSYM_COVER_GAP, M = gap_cost)",
                 "a gap frame: acc = gap_cost + acc", "FRAME BY FRAME", "a piece wins a tie against a gap",
                 "gap_cost = +inf never wins", "SSYM_E_INVALID before any device work"):
        assert line in doc, line
    live = header[header.index(CREATE + ": a coverer"):header.index(CREATE + "(ssym_ctx")]
    for line in ("(lane, SSYM_COVER_GAP, e, e, gap_cost)", "lastFinite = n - 1", "becomes a gap frame"):
        assert line in live, line
    # one step for both chains: the candidate stands in the shared header and in no kernel file
    step = _read("soundsym_amd", "csrc", "dtw_cover_chain.hpp")
    assert "__dadd_rn(gapCost, ring[e & ringMask])" in step and "if (gapV < bestV)" in step
    for name in ("dtw_cover.hip", "dtw_coverer.hip"):
        assert "kCoverGap" not in _read("soundsym_amd", "csrc", name)


def test_null_context_is_refused_without_a_device(native_lib):
    u = np.full(4, 7, dtype=np.uint32)
    f = np.full(4, -1.5)
    for gap in (0.0, -1.0, float("nan"), INF):
        rc = native_lib.ssym_dtw_cover_gaps(None, None, None, 0.0, gap, 0, u.ctypes.data, f.ctypes.data, u.ctypes.data,
                                            u.ctypes.data, u.ctypes.data, f.ctypes.data)
        assert rc == nat.SSYM_E_INVALID
        assert native_lib.ssym_coverer_create_gaps(None, None, 1, 0.0, gap, None) == nat.SSYM_E_INVALID
    assert (u == 7).all() and (f == -1.5).all()


# -- Gap and Cover -----------------------------------------------------------------------------------------------------------

def test_gap_arithmetic():
    g = Gap(4, 9, 3.0)
    assert (g.start_frame, g.end_frame, g.cost) == (4, 9, 3.0) and g.is_gap and not Piece(0, 0, 0, 0.0).is_gap
    assert g.num_frames() == 6 and g.cost_per_frame == 0.5
    assert g.sample_span(100 * HOP) == (4 * HOP, 10 * HOP) == Piece(0, 4, 9, 0.0).sample_span(100 * HOP)
    assert g.sample_span(10 * HOP - 7) == (4 * HOP, 10 * HOP - 7)
    assert "frames=4...9" in repr(g) and not hasattr(g, "source_index")
    assert Gap(0, 0, 0.0).cost_per_frame == 0.0
    for bad in ((3, 2, 0.0), (-1, 2, 0.0), (0, 1, -1.0), (0, 1, float("nan"))):
        with pytest.raises(ValueError):
            Gap(*bad)


def test_cover_with_gaps():
    tiles = [Piece(1, 0, 2, 3.0), Gap(3, 4, 1.0), Piece(0, 5, 8, 0.5), Gap(9, 9, 0.5)]
    c = Cover(tiles, 5.0, 10)
    assert len(c) == 4 and bool(c) and c.total_per_frame == 0.5
    assert c.gaps == [tiles[1], tiles[3]] and c.sounding == [tiles[0], tiles[2]] and c.covered_frames == 7
    assert c.indices().dtype == np.int64 and c.indices().tolist() == [1, 0]
    assert "2 pieces, 2 gaps" in repr(c)
    n = 10 * HOP + 300
    assert c.segment_lengths(n) == [3 * HOP, 2 * HOP, 4 * HOP, HOP + 300]          # every tile counts, gaps included
    only = Cover([Gap(0, 2, 1.5)], 1.5, 3)
    assert only and only.covered_frames == 0 and only.indices().size == 0 and only.sounding == []
    plain = Cover([Piece(1, 0, 2, 3.0)], 3.0, 3)
    assert plain.gaps == [] and plain.covered_frames == 3 and repr(plain) == "Cover(1 pieces, total=3.0)"
    assert Cover.none(4).gaps == [] and Cover.none(4).covered_frames == 0
    for bad, frames in (([Gap(1, 2, 0.0)], 3), ([Piece(0, 0, 2, 0.0), Gap(4, 5, 0.0)], 6), ([Gap(0, 2, 0.0)], 4)):
        with pytest.raises(ValueError, match="tile the target"):
            Cover(bad, 0.0, frames)
    with pytest.raises(ValueError, match="maximal run"):
        Cover([Gap(0, 1, 0.0), Gap(2, 3, 0.0)], 0.0, 4)


def test_gap_frames_merge_into_runs():
    u = lambda v: np.array(v, dtype=np.uint32)
    src, start, end = u([2, GAP, GAP, GAP, 0, GAP]), u([0, 3, 4, 5, 6, 9]), u([2, 3, 4, 5, 8, 9])
    tiles = api_mod._cover_tiles(src, start, end, np.array([1.0, 0.25, 0.25, 0.25, 2.0, 0.25]))
    assert [(type(t), t.start_frame, t.end_frame, t.cost) for t in tiles] == [
        (Piece, 0, 2, 1.0), (Gap, 3, 5, 0.75), (Piece, 6, 8, 2.0), (Gap, 9, 9, 0.25)]
    assert Cover(tiles, 3.0, 10).covered_frames == 6
    assert api_mod._cover_tiles(u([]), u([]), u([]), np.zeros(0)) == []


def test_cut_sounds_skip_the_gaps():
    rng = np.random.default_rng(2)
    n = 10 * HOP + 300
    sound = Sound(rng.standard_normal(n), 8000.0, rng.standard_normal((10, 5)).reshape(-1), "t", ncoeffs=5)
    c = Cover([Piece(1, 0, 2, 3.0), Gap(3, 4, 1.0), Piece(0, 5, 9, 0.5)], 4.5, 10)
    seq = SoundSequence.from_cover(sound, c).sounds()
    assert [s.num_frames() for s in seq] == [3, 5] and [s.samples().size for s in seq] == [3 * HOP, n - 5 * HOP]
    assert np.array_equal(seq[0].samples(), sound.samples()[:3 * HOP])
    assert np.array_equal(seq[1].samples(), sound.samples()[5 * HOP:])
    assert np.array_equal(seq[1].mfcc_arrays(), sound.mfcc_arrays()[5:10])
    assert SoundSequence.from_cover(sound, Cover([Gap(0, 9, 1.0)], 1.0, 10)).sounds() == []


def test_live_cover_merges_runs_and_sums_frame_by_frame():
    class _Cv:
        n_lanes = 1

        def __init__(self):
            self.batches = [([0, 0, 0], [3, GAP, GAP], [0, 4, 5], [3, 4, 5], [1.0, 0.1, 0.1]), ([0, 0], [GAP, 1], [6, 7], [6, 9], [0.1, 2.0])]

        def follow(self, stream):
            self.now = self.batches.pop(0)

        def pieces(self):
            lane, src, start, end, cost = self.now
            u = lambda v: np.array(v, dtype=np.uint32)
            return u(lane), u(src), u(start), u(end), np.array(cost)

    live = LiveCover(["a"], object(), _Cv(), 2.0, 0.1)
    first = live.poll()
    assert [(l, type(p), p.start_frame, p.end_frame) for l, p in first] == [(0, Piece, 0, 3), (0, Gap, 4, 5)]
    second = live.poll()
    assert [(l, type(p), p.start_frame, p.end_frame) for l, p in second] == [(0, Gap, 6, 6), (0, Piece, 7, 9)]
    cover, = live.covers()
    assert [(type(p), p.start_frame, p.end_frame) for p in cover.pieces] == [(Piece, 0, 3), (Gap, 4, 6), (Piece, 7, 9)]
    assert cover.gaps[0].cost == 0.1 * 3 and cover.num_frames == 10
    assert cover.total == (2.0 + 2.0) + (0.1 + (0.1 + (0.1 + ((1.0 + 2.0) + 0.0))))        # no penalty on a gap frame


# -- the checks before any library call ------------------------------------------------------------------------------------

class _FakeEngine:
    """Enough of an Engine for the checks that come before any library call; anything else fails loudly."""
    np_dtype = np.float64

    def __init__(self, metric="dtw"):
        self.metric = metric

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


def _sounds():
    rng = np.random.default_rng(0xA11)
    return [Sound(rng.standard_normal(frames * HOP), 8000.0 + k, rng.standard_normal((frames, 5)).reshape(-1), "s%d" % k,
                  ncoeffs=5) for k, frames in enumerate((20, 7))]


def test_argument_mistakes_raise_before_any_library_call():
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = _sounds()
    t = _sounds()
    for bad in (-1.0, float("nan"), -INF, -1e-300):
        for call in (lambda: d.cover(t, 0.0, bad), lambda: d.cover(t, gap_cost=bad), lambda: d.cover_live(t, 0.0, bad),
                     lambda: d.cover_long(t[0], 0.0, 64, bad), lambda: d.reconstruct_covered(t[0], gap_cost=bad)):
            with pytest.raises(ValueError, match="gap_cost must not be negative or NaN"):
                call()
    with pytest.raises((ValueError, TypeError)):
        d.cover(t, 0.0, "x")
    for bad in ("hum", None, 0):
        with pytest.raises(ValueError, match='gap_fill must be "silence" or "target"'):
            d.reconstruct_covered(t[0], gap_cost=1.0, gap_fill=bad)
    with pytest.raises(ValueError, match="piece_penalty"):
        d.cover(t, -1.0, 1.0)
    assert d.cover([], 0.0, 1.0) == []


class _Handle:
    ptr, n, dim = None, 2, 5
    offsets = np.array([0, 3, 7], dtype=np.uint64)


class _Lib:
    """Records the entry points an Engine method calls; every call succeeds and writes nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return nat.SSYM_OK
        return call


def test_engine_calls_and_their_gap_cost_check(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    h = _Handle()
    e.dtw_cover(h, h)
    e.dtw_cover(h, h, 2.5, gap_cost=None)
    out = e.dtw_cover(h, h, 2.5, gap_cost=0.0)
    assert [(x.shape, x.dtype) for x in out] == [((2,), np.uint32), ((2,), np.float64), ((7,), np.uint32), ((7,), np.uint32),
                                                 ((7,), np.uint32), ((7,), np.float64)]
    e.dtw_cover(h, h, gap_cost=INF)
    assert lib.calls == [("ssym_dtw_cover", 11)] * 2 + [(COVER, 12)] * 2         # None takes today's entry point
    lib.calls.clear()
    assert e.coverer(h, 2).gap_cost is None and e.coverer(h, 2, 1.0, 0.5).gap_cost == 0.5
    assert lib.calls == [("ssym_coverer_create", 5), (CREATE, 6)]
    lib.calls.clear()
    for bad in (-1.0, float("nan"), -INF):
        with pytest.raises(ValueError):
            e.dtw_cover(h, h, gap_cost=bad)
        with pytest.raises(ValueError):
            e.coverer(h, 1, 0.0, bad)
    assert lib.calls == []
