"""The coverer's surface without a device: header, binding, Rust declarations and C++ mirror holding to each other, the limits
the header names against the kernels' constants, and the ValueErrors of cover_live / cover_long / Coverer that come before
any library call."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Cover, Coverer, LiveCover, Piece, Sound, SoundDictionary, SsymError
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
CALLS = {                                                # name -> the header's argument names
    "ssym_coverer_create": ["ctx", "dict", "n_lanes", "piece_penalty", "out"],
    "ssym_coverer_destroy": ["ctx", "cv"],
    "ssym_coverer_push": ["ctx", "cv", "feats", "frame_offsets", "flags", "out_n_pieces"],
    "ssym_coverer_follow": ["ctx", "cv", "stream", "flags", "out_n_pieces"],
    "ssym_coverer_pieces": ["ctx", "cv", "out_lane", "out_src", "out_start", "out_end", "out_cost", "flags"],
    "ssym_coverer_flush": ["ctx", "cv", "lane", "out_n_pieces"],
    "ssym_coverer_best": ["ctx", "cv", "out_total", "out_covered", "out_committed", "flags"],
    "ssym_coverer_counts": ["cv", "out_frames", "out_capacity"],
    "ssym_coverer_reset": ["ctx", "cv", "lane"],
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
    assert "pub struct SsymCoverer" in rust and "typedef struct ssym_coverer ssym_coverer;" in header
    assert "class Coverer {" in mirror
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header       # additions only


def test_header_states_the_definition_and_the_limits():
    header = _read("include", "soundsym_amd.h")
    cover, coverer = _read("soundsym_amd", "csrc", "dtw_cover.hip"), _read("soundsym_amd", "csrc", "dtw_coverer.hip")
    const = lambda src, name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, src).group(1))
    frames, ring = const(cover, "kCoverMaxSourceFrames"), const(cover, "kCoverRing")
    assert const(coverer, "kCovererBackMin") == 1024 and const(coverer, "kCovererMaxLanes") == 65535
    # the lane limit is the lane feed's, shared with the spotter
    assert "kLaneMaxFrames" in coverer and "kLaneMaxFrames = %d;" % 0x7fffffff in _read("soundsym_amd", "csrc", "lane_feed.hpp")
    assert ring > 2 * frames and ring & (ring - 1) == 0     # the ring holds best(e) of the W ends of the horizon and best(-1)
    doc = header[header.index("Live cover (DESIGN.md"):header.index("ssym_coverer_create(ssym_ctx")]
    for line in ("H(n) = { e : max(-1, n-W) <= e <= n-1, best(e) finite }", "C(n) = the longest common prefix of walk(e) over e in H(n)",
                 "walk(lastFinite)", "The lane has then ENDED", "total = best(n-1)", "covered = lastFinite + 1, committed = done + 1",
                 "W = 2 max(Fmax, 1)", "never revised", "a power of two, 1024 at least", "dim <= 64",
                 "at most %d frames (kCoverMaxSourceFrames)" % frames, "at most 65535 lanes",
                 "lanes x 2 Fmax x 2 Fmax x 12 bytes <= 512 MiB", "lanes x (W - 1 + new frames) x W x 12 bytes", "2^31 - 1 frames",
                 "SSYM_E_INVALID", "SSYM_E_UNSUPPORTED", "SSYM_E_EMPTY_DICT", "SSYM_OUT_DEVICE", "ordered by (lane, start)",
                 "main_ms = the forward pass", "reduce_ms = chain, commit and emission",
                 "n_pairs = n_sources x the frames the call consumed", "A dictionary appended to since: SSYM_E_INVALID"):
        assert line in doc, line
    # the definition in the kernel file's header comment is the header's
    for line in ("horizon  : H(n) = { e : max(-1, n-W) <= e <= n-1, best(e) finite }", "flush    : emits the pieces of walk(lastFinite)"):
        assert line in coverer, line
    # one chain step for both kernels, one forward launch for both callers
    chain = _read("soundsym_amd", "csrc", "dtw_cover_chain.hpp")
    assert "cover_chain_step(" in chain and cover.count("cover_chain_step(") == 1 and coverer.count("cover_chain_step(") == 1
    assert "cover_forward_kernel<<<" in cover and "cover_forward_kernel" not in coverer.replace("cover_forward_kernel and", "")
    assert "cover_forward(ctx," in coverer and "cover_forward(ctx," in cover
    make = _read("soundsym_amd", "csrc", "Makefile")
    assert " dtw_coverer.hip " in make and re.search(r"\$\(BUILD\)/dtw_coverer\.o[^\n]*: dtw_cover_chain\.hpp", make)


def test_null_handles_are_refused_without_a_device(native_lib):
    u = np.full(4, 7, dtype=np.uint32)
    f = np.full(4, -1.5)
    n = np.full(1, 9, dtype=np.uint64)
    p = lambda a: a.ctypes.data
    assert native_lib.ssym_coverer_create(None, None, 1, 0.0, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_coverer_push(None, None, p(f), p(n), 0, n.ctypes.data_as(native_lib.ssym_coverer_push.argtypes[5])) == nat.SSYM_E_INVALID
    assert native_lib.ssym_coverer_follow(None, None, None, 0, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_coverer_pieces(None, None, p(u), p(u), p(u), p(u), p(f), 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_coverer_flush(None, None, 0, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_coverer_best(None, None, p(f), p(u), p(u), 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_coverer_counts(None, p(n), None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_coverer_reset(None, None, 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_coverer_destroy(None, None) == nat.SSYM_OK          # destroying nothing is fine
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
    rng = np.random.default_rng(0xA11)
    return [Sound(rng.standard_normal(frames * HOP), 8000.0 + k, rng.standard_normal((frames, ncoeffs)).reshape(-1), "s%d" % k,
                  ncoeffs=ncoeffs) for k, frames in enumerate((20, 7))]


def test_cover_live_and_cover_long_raise_before_any_library_call():
    e = _FakeEngine()
    d = SoundDictionary(engine=e)
    d.sounds = _sounds()
    t = _sounds()
    for bad in (-1.0, float("nan"), INF, -INF, -1e-300):
        with pytest.raises(ValueError, match="piece_penalty must be finite and not negative"):
            d.cover_live(t, bad)
        with pytest.raises(ValueError, match="piece_penalty must be finite and not negative"):
            d.cover_long(t[0], bad)
    # the sounds must share one stream, sound i in lane i: watch's check
    with pytest.raises(ValueError, match="cover_live: the sounds must share one stream"):
        d.cover_live(t)
    with pytest.raises(ValueError, match="share one stream"):
        d.cover_live([])
    st = _FakeStream(e, 2)
    t[0]._stream, t[1]._stream = (st, 0), (_FakeStream(e, 2), 1)
    with pytest.raises(ValueError, match="share one stream"):
        d.cover_live(t)
    t[1]._stream = (st, 0)
    with pytest.raises(ValueError, match="share one stream"):
        d.cover_live(t)                                  # sound 1 is not in lane 1
    t[1]._stream = (st, 1)
    with pytest.raises(ValueError, match="share one stream"):
        d.cover_live(t[:1])                              # not every lane of the stream
    other = SoundDictionary(engine=_FakeEngine())
    other.sounds = _sounds()
    with pytest.raises(ValueError, match="engine must be the one that holds the sounds' stream"):
        other.cover_live(t)
    wide = SoundDictionary(engine=e)
    wide.sounds = _sounds(7)
    with pytest.raises(ValueError, match="ncoeffs"):
        wide.cover_live(t)
    with pytest.raises(ValueError, match="ncoeffs"):
        wide.cover_long(t[0])
    for bad in (0, -4, 2.5):
        with pytest.raises(ValueError, match="block_frames"):
            d.cover_long(t[0], 0.0, bad)
    with pytest.raises(ValueError, match="takes one Sound"):
        d.cover_long(t)
    with pytest.raises(soundsym_amd.EmptyDictionaryError):
        SoundDictionary(engine=e).cover_live(t)
    with pytest.raises(soundsym_amd.EmptyDictionaryError):
        SoundDictionary(engine=e).cover_long(t[0])
    refcos = SoundDictionary(engine=_FakeEngine("refcos"))
    refcos.sounds = _sounds()
    for call in (lambda: refcos.cover_live(t), lambda: refcos.cover_long(t[0])):
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


def test_coverer_calls_and_their_checks(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    h = _Handle()
    for bad in (-1.0, float("nan"), INF):
        with pytest.raises(ValueError):
            e.coverer(h, 1, bad)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="n_lanes"):
            e.coverer(h, bad)
    assert lib.calls == []
    cv = e.coverer(h, 2, 2.5)
    assert isinstance(cv, Coverer) and cv.d is h and (cv.n_lanes, cv.dim, cv.piece_penalty) == (2, 3, 2.5)
    x = np.zeros((4, 3))
    for call in (lambda: cv.push(x), lambda: cv.push(x, [0, 4]), lambda: cv.push(x, [0, 3, 2]), lambda: cv.push(x, [0, 2, 5]),
                 lambda: cv.push(np.zeros(7), [0, 1, 2]), lambda: cv.flush(2), lambda: cv.flush(-1), lambda: cv.reset(2)):
        with pytest.raises(ValueError):
            call()

    class _St:
        n_lanes, ncoeffs, ptr = 3, 3, None
    with pytest.raises(ValueError, match="follow"):
        cv.follow(_St())
    assert lib.calls == [("ssym_coverer_create", 5)]
    lib.calls.clear()
    assert cv.push(x, [0, 1, 4]) == 0 and cv.flush(1) == 0
    out = cv.pieces()
    assert [(a.shape, a.dtype) for a in out] == [((0,), np.uint32)] * 4 + [((0,), np.float64)]     # no pieces: no call
    best = cv.best()
    assert [(a.shape, a.dtype) for a in best] == [((2,), np.float64), ((2,), np.uint32), ((2,), np.uint32)]
    frames, cap = cv.counts()
    assert frames.shape == (2,) and frames.dtype == np.uint64 and cap == 0
    cv.reset(1)
    cv.close()
    cv.close()
    assert lib.calls == [("ssym_coverer_push", 6), ("ssym_coverer_flush", 4), ("ssym_coverer_best", 6), ("ssym_coverer_counts", 3),
                         ("ssym_coverer_reset", 3)]                      # (ctx is None: nothing to destroy)


def test_live_cover_collects_what_it_returns():
    class _Cv:
        n_lanes = 2

        def __init__(self):
            self.batches = [([0, 0, 1], [3, 1, 2], [0, 4, 0], [3, 9, 5], [1.0, 2.0, 0.5]), ([1], [0], [6], [6], [0.25])]

        def follow(self, stream):
            self.now = self.batches.pop(0)

        def pieces(self):
            lane, src, start, end, cost = self.now
            u = lambda v: np.array(v, dtype=np.uint32)
            return u(lane), u(src), u(start), u(end), np.array(cost)

    live = LiveCover(["a", "b"], object(), _Cv(), 2.0)
    first = live.poll()
    assert [(l, p.source_index, p.start_frame, p.end_frame, p.cost) for l, p in first] == [(0, 3, 0, 3, 1.0), (0, 1, 4, 9, 2.0),
                                                                                           (1, 2, 0, 5, 0.5)]
    assert all(isinstance(p, Piece) for _, p in first)
    live.poll()
    a, b = live.covers()
    assert isinstance(a, Cover) and a.num_frames == 10 and len(a) == 2 and a.total == (2.0 + 2.0) + ((1.0 + 2.0) + 0.0)
    assert b.num_frames == 7 and b.total == (0.25 + 2.0) + ((0.5 + 2.0) + 0.0)
    assert LiveCover(["a"], object(), _Cv(), 0.0).covers()[0].total == INF
