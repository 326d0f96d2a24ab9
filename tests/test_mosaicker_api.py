"""The mosaicker's surface without a device: header, binding, Rust declarations and C++ mirror holding to each other, the
limits the header names against the kernels' constants, and the ValueErrors of mosaic_live / mosaic_long / Mosaicker that
come before any library call."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Gap, LiveMosaic, Mosaic, MosaicPiece, Mosaicker, Sound, SoundDictionary, SsymError
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
CALLS = {                                                # name -> the header's argument names
    "ssym_mosaicker_create": ["ctx", "dict", "n_lanes", "piece_penalty", "gap_cost", "out"],
    "ssym_mosaicker_destroy": ["ctx", "mk"],
    "ssym_mosaicker_push": ["ctx", "mk", "feats", "frame_offsets", "flags", "out_n_frames"],
    "ssym_mosaicker_follow": ["ctx", "mk", "stream", "flags", "out_n_frames"],
    "ssym_mosaicker_frames": ["ctx", "mk", "out_lane", "out_column", "out_src", "out_frame", "out_cost", "out_start", "flags"],
    "ssym_mosaicker_flush": ["ctx", "mk", "lane", "out_n_frames"],
    "ssym_mosaicker_best": ["ctx", "mk", "out_total", "out_covered", "out_committed", "flags"],
    "ssym_mosaicker_counts": ["mk", "out_frames", "out_capacity"],
    "ssym_mosaicker_reset": ["ctx", "mk", "lane"],
}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbols(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    for name, args in CALLS.items():
        decl = re.search(r"SSYM_API\s+int32_t\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        assert re.findall(r"(\w+)\s*(?:,|$)", decl.group(1).replace("\n", " ")) == args, name
        assert name in nat.ABI_SYMBOLS and name in soundsym_amd.ABI_SYMBOLS
        assert hasattr(native_lib, name) and len(getattr(native_lib, name).argtypes) == len(args), name
        assert getattr(native_lib, name).restype is not None
        rs = re.search(r"pub fn %s\s*\(([^;]*)\)\s*->\s*i32;" % name, rust)
        assert rs and re.findall(r"(\w+):", rs.group(1)) == args, name
        assert name + "(" in mirror, name
    assert "pub struct SsymMosaicker" in rust and "typedef struct ssym_mosaicker ssym_mosaicker;" in header
    assert "class Mosaicker {" in mirror
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header       # additions only


def test_header_states_the_definition_and_the_limits():
    header = _read("include", "soundsym_amd.h")
    mosaic, mosaicker = _read("soundsym_amd", "csrc", "dtw_mosaic.hip"), _read("soundsym_amd", "csrc", "dtw_mosaicker.hip")
    common = _read("soundsym_amd", "csrc", "dtw_mosaic_common.hpp")
    const = lambda src, name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, src).group(1))
    assert const(mosaicker, "kMosaickerMaxLanes") == 65535 and const(common, "kMosaicMaxDim") == 64
    assert (const(mosaicker, "kMosaickerRingMax"), const(mosaicker, "kMosaickerRingMin")) == (1024, 16)
    assert "kMosaickerRingBytes = 64ull << 20" in mosaicker and "kMosaicScratchBytes = 512ull << 20" in common
    assert "kLaneMaxFrames" in mosaicker
    doc = header[header.index("Live mosaic (DESIGN.md"):header.index("ssym_mosaicker_create(ssym_ctx")]
    for line in ("S' = piece_penalty + best(n-1)", "E(g, n-1) finite and <= S'", "N(g, n-1) is finite and <= S'", "NaN is never live",
                 "c(n) = the largest column <= n-1 at which all walks of live(n) hold the same key", "arg(lastFinite) at column lastFinite",
                 "The lane has then ENDED", "total = best(n-1)", "covered = lastFinite + 1, committed = done + 1",
                 "never revised", "and only grows", "rounding is monotone", "dim <= 64", "at most 65535 lanes", "512 MiB", "64 MiB",
                 "2^31 - 1 frames", "SSYM_E_INVALID", "SSYM_E_UNSUPPORTED", "SSYM_E_EMPTY_DICT", "SSYM_OUT_DEVICE",
                 "ordered by (lane, column)", "says to flush", "main_ms = the", "reduce_ms = commit and emission",
                 "A dictionary appended to since: SSYM_E_INVALID", "G + 4 + 8 dim bytes per uncommitted column"):
        assert line in doc, line
    for line in ("live(n)  : S' = piece_penalty + best(n-1)", "flush    : emits the rest of the walk from arg(lastFinite)"):
        assert line in mosaicker, line
    # the three shared pieces exist once, in the header both files include; the offline kernels stayed where they were
    for name in ("mosaic_prep_kernel(", "mosaic_cost(", "mosaic_segment("):
        assert common.count("void " + name) + common.count("double " + name) + common.count("uint32_t " + name) == 1, name
        assert ("void " + name) not in mosaic and ("double " + name) not in mosaic and ("uint32_t " + name) not in mosaic
    assert "mosaic_forward_kernel<<<" in mosaic and "mosaic_backtrace_kernel<<<" in mosaic
    assert '#include "dtw_mosaic_common.hpp"' in mosaic and '#include "dtw_mosaic_common.hpp"' in mosaicker
    assert '#include "lane_feed.hpp"' in mosaicker and "mosaicker (dtw_mosaicker.hip)" in _read("soundsym_amd", "csrc", "lane_feed.hpp")
    make = _read("soundsym_amd", "csrc", "Makefile")
    assert " dtw_mosaicker.hip " in make and re.search(r"\$\(BUILD\)/dtw_mosaicker\.o[^\n]*: lane_feed\.hpp", make)
    assert re.search(r"\$\(BUILD\)/dtw_mosaicker\.o[^\n]*: dtw_mosaic_common\.hpp", make)


def test_null_handles_are_refused_without_a_device(native_lib):
    u = np.full(4, 7, dtype=np.uint32)
    f = np.full(4, -1.5)
    n = np.full(1, 9, dtype=np.uint64)
    p = lambda a: a.ctypes.data
    assert native_lib.ssym_mosaicker_create(None, None, 1, 0.0, INF, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_mosaicker_push(None, None, p(f), p(n), 0, n.ctypes.data_as(native_lib.ssym_mosaicker_push.argtypes[5])) == nat.SSYM_E_INVALID
    assert native_lib.ssym_mosaicker_follow(None, None, None, 0, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_mosaicker_frames(None, None, p(u), p(u), p(u), p(u), p(f), p(u), 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_mosaicker_flush(None, None, 0, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_mosaicker_best(None, None, p(f), p(u), p(u), 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_mosaicker_counts(None, p(n), None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_mosaicker_reset(None, None, 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_mosaicker_destroy(None, None) == nat.SSYM_OK        # destroying nothing is fine
    assert (u == 7).all() and (f == -1.5).all() and n[0] == 9


# -- the checks before any library call ------------------------------------------------------------------------------------

class _FakeEngine:
    """Enough of an Engine for the checks that come before any library call; anything else fails loudly."""
    np_dtype = np.float64

    def __init__(self, metric="dtw"):
        self.metric = metric

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


class _FakeStream:
    ptr, ncoeffs = 1, 5

    def __init__(self, engine, n_lanes):
        self.engine, self.n_lanes = engine, n_lanes


def _sounds(ncoeffs=5):
    rng = np.random.default_rng(0xA12)
    return [Sound(rng.standard_normal(frames * HOP), 8000.0 + k, rng.standard_normal((frames, ncoeffs)).reshape(-1), "s%d" % k,
                  ncoeffs=ncoeffs) for k, frames in enumerate((20, 7))]


def test_mosaic_live_and_mosaic_long_raise_before_any_library_call():
    e = _FakeEngine()
    d = SoundDictionary(engine=e)
    d.sounds = _sounds()
    t = _sounds()
    for bad in (-1.0, float("nan"), INF, -INF, -1e-300):
        with pytest.raises(ValueError, match="piece_penalty must be finite and not negative"):
            d.mosaic_live(t, bad)
        with pytest.raises(ValueError, match="piece_penalty must be finite and not negative"):
            d.mosaic_long(t[0], bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="gap_cost"):
            d.mosaic_live(t, 1.0, bad)
        with pytest.raises(ValueError, match="gap_cost"):
            d.mosaic_long(t[0], 1.0, 8, bad)
    with pytest.raises(ValueError, match="mosaic_live: the sounds must share one stream"):
        d.mosaic_live(t)
    with pytest.raises(ValueError, match="share one stream"):
        d.mosaic_live([])
    st = _FakeStream(e, 2)
    t[0]._stream, t[1]._stream = (st, 0), (st, 0)
    with pytest.raises(ValueError, match="share one stream"):
        d.mosaic_live(t)                                 # sound 1 is not in lane 1
    t[1]._stream = (st, 1)
    other = SoundDictionary(engine=_FakeEngine())
    other.sounds = _sounds()
    with pytest.raises(ValueError, match="engine must be the one that holds the sounds' stream"):
        other.mosaic_live(t)
    wide = SoundDictionary(engine=e)
    wide.sounds = _sounds(7)
    with pytest.raises(ValueError, match="ncoeffs"):
        wide.mosaic_live(t)
    with pytest.raises(ValueError, match="ncoeffs"):
        wide.mosaic_long(t[0])
    for bad in (0, -4, 2.5):
        with pytest.raises(ValueError, match="block_frames"):
            d.mosaic_long(t[0], 0.0, bad)
    with pytest.raises(ValueError, match="takes one Sound"):
        d.mosaic_long(t)
    with pytest.raises(ValueError, match="must be a Mosaic"):
        d.reconstruct_mosaic(t[0], 1.0, mosaic=object())
    with pytest.raises(soundsym_amd.EmptyDictionaryError):
        SoundDictionary(engine=e).mosaic_live(t)
    with pytest.raises(soundsym_amd.EmptyDictionaryError):
        SoundDictionary(engine=e).mosaic_long(t[0])
    refcos = SoundDictionary(engine=_FakeEngine("refcos"))
    refcos.sounds = _sounds()
    for call in (lambda: refcos.mosaic_live(t), lambda: refcos.mosaic_long(t[0])):
        with pytest.raises(SsymError) as err:
            call()
        assert err.value.code == nat.SSYM_E_UNSUPPORTED


class _Handle:
    ptr, n, dim = None, 2, 3


class _Lib:
    """Records the entry points a call makes; every call succeeds and writes nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return nat.SSYM_OK
        return call


def test_mosaicker_calls_and_their_checks(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    h = _Handle()
    for bad in (-1.0, float("nan"), INF):
        with pytest.raises(ValueError):
            e.mosaicker(h, 1, bad)
    with pytest.raises(ValueError, match="gap_cost"):
        e.mosaicker(h, 1, 1.0, -0.5)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="n_lanes"):
            e.mosaicker(h, bad)
    assert lib.calls == []
    mk = e.mosaicker(h, 2, 2.5, 4.0)
    assert isinstance(mk, Mosaicker) and mk.d is h and (mk.n_lanes, mk.dim, mk.piece_penalty, mk.gap_cost) == (2, 3, 2.5, 4.0)
    x = np.zeros((4, 3))
    for call in (lambda: mk.push(x), lambda: mk.push(x, [0, 4]), lambda: mk.push(x, [0, 3, 2]), lambda: mk.push(x, [0, 2, 5]),
                 lambda: mk.push(np.zeros(7), [0, 1, 2]), lambda: mk.flush(2), lambda: mk.flush(-1), lambda: mk.reset(2)):
        with pytest.raises(ValueError):
            call()

    class _St:
        n_lanes, ncoeffs, ptr = 3, 3, None
    with pytest.raises(ValueError, match="follow"):
        mk.follow(_St())
    assert lib.calls == [("ssym_mosaicker_create", 6)]
    lib.calls.clear()
    assert mk.push(x, [0, 1, 4]) == 0 and mk.flush(1) == 0
    out = mk.frames()
    assert [(a.shape, a.dtype) for a in out] == [((0,), np.uint32)] * 4 + [((0,), np.float64), ((0,), np.uint32)]     # no frames: no call
    best = mk.best()
    assert [(a.shape, a.dtype) for a in best] == [((2,), np.float64), ((2,), np.uint32), ((2,), np.uint32)]
    frames, cap = mk.counts()
    assert frames.shape == (2,) and frames.dtype == np.uint64 and cap == 0
    mk.reset(1)
    mk.close()
    mk.close()
    assert lib.calls == [("ssym_mosaicker_push", 6), ("ssym_mosaicker_flush", 4), ("ssym_mosaicker_best", 6),
                         ("ssym_mosaicker_counts", 3), ("ssym_mosaicker_reset", 3)]      # (ctx is None: nothing to destroy)


def test_live_mosaic_closes_a_piece_when_the_next_start_is_committed():
    G = nat.COVER_GAP

    class _Mk:
        n_lanes = 2

        def __init__(self):
            # (lane, column, src, frame, cost, start)
            self.batches = [([0, 0, 0, 1], [0, 1, 2, 0], [3, 3, 1, G], [5, 6, 0, nat.NO_MATCH], [1.0, 0.5, 2.0, 4.0], [1, 0, 1, 1]),
                            ([0, 1, 1], [3, 1, 2], [1, G, 2], [2, nat.NO_MATCH, 9], [0.25, 4.0, 1.5], [0, 1, 1]),
                            ([0], [4], [1], [3], [0.125], [0]), ([1], [3], [2], [9], [0.5], [0])]

        def follow(self, stream):
            self.now = self.batches.pop(0)

        def flush(self, lane):
            self.now = self.batches.pop(0)

        def frames(self):
            lane, col, src, frame, cost, start = self.now
            u = lambda v: np.array(v, dtype=np.uint32)
            return u(lane), u(col), u(src), u(frame), np.array(cost), u(start)

    live = LiveMosaic(["a", "b"], object(), _Mk(), 2.0, 4.0)
    first = live.poll()                                   # sound 0: the piece 0-1 is closed by the start at 2; sound 1: nothing yet
    assert [(l, p.is_gap, p.start_frame, p.end_frame) for l, p in first] == [(0, False, 0, 1)]
    assert first[0][1].frame_map.tolist() == [5, 6] and first[0][1].cost == 0.5 + 1.0
    second = live.poll()                                  # sound 1: gap 0, then gap 1 closed by the start at 2: one Gap per call
    assert [(l, p.is_gap, p.start_frame, p.end_frame) for l, p in second] == [(1, True, 0, 1)]
    assert [a.size for a in live.committed()[0]] == [4] * 4 and live.committed()[1][3].tolist() == [True, True, True]
    rest = live.flush()
    assert [(l, p.is_gap, p.start_frame, p.end_frame) for l, p in rest] == [(0, False, 2, 4), (1, False, 2, 3)]
    a, b = live.mosaics()
    assert isinstance(a, Mosaic) and a.num_frames == 5 and [type(p) for p in a.pieces] == [MosaicPiece, MosaicPiece]
    assert a.total == 0.125 + (0.25 + (2.0 + (2.0 + (0.5 + (1.0 + (2.0 + 0.0))))))
    assert [type(p) for p in b.pieces] == [Gap, MosaicPiece] and b.pieces[0].cost == 8.0 and b.total == 0.5 + (1.5 + (2.0 + (4.0 + (4.0 + 0.0))))
    assert LiveMosaic(["a"], object(), _Mk(), 0.0).mosaics()[0].total == INF
