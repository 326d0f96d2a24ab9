"""The resynthesiser's surface without a device: header, binding, Rust declarations and C++ mirror holding to each other, the
definition the header carries against the kernels' constants, the shared search step, and the ValueErrors of Engine.resynth /
Resynth / mosaic_live(audio=True) / LiveMosaic.audio that come before any library call."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, LiveMosaic, Resynth, SoundDictionary
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {                                                # name -> the header's argument names
    "ssym_resynth_create": ["ctx", "store", "n_lanes", "search", "out"],
    "ssym_resynth_destroy": ["ctx", "rs"],
    "ssym_resynth_push": ["ctx", "rs", "lane", "column", "src", "frame", "start", "n_frames", "out_n_samples"],
    "ssym_resynth_take": ["ctx", "rs", "mk", "out_n_samples"],
    "ssym_resynth_samples": ["ctx", "rs", "out_lane_offsets", "out_samples", "out_pcm32", "flags"],
    "ssym_resynth_flush": ["ctx", "rs", "lane", "total_samples", "out_n_samples"],
    "ssym_resynth_counts": ["rs", "out_frames", "out_samples"],
    "ssym_resynth_reset": ["ctx", "rs", "lane"],
}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbols(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    integration = _read("INTEGRATION.md")
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
        assert name in integration, name
    assert "pub struct SsymResynth" in rust and "typedef struct ssym_resynth ssym_resynth;" in header
    assert "class Resynth {" in mirror and "Resynth" in soundsym_amd.__all__
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header       # additions only
    assert "pub const SSYM_ABI_VERSION: i32 = 3;" in rust


def test_header_states_the_definition_and_the_kernels_hold_to_it():
    header = _read("include", "soundsym_amd.h")
    resynth, common, wsola = (_read("soundsym_amd", "csrc", f) for f in ("resynth.hip", "warp_common.hpp", "wsola.hip"))
    const = lambda src, name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, src).group(1))
    assert const(resynth, "kResynthMaxLanes") == 65535 and const(resynth, "kResynthRing") == 16 and const(resynth, "kResynthHops") == 16
    assert const(common, "kWsolaMaxSearch") == 512
    assert "rs->reach = search ? (search + 1279) / 256 : 2;" in resynth
    doc = header[header.index("Live resynthesis (DESIGN.md"):header.index("ssym_resynth_create(ssym_ctx")]
    for line in ("src = SSYM_COVER_GAP is a gap frame", "starts at every frame with start = 1", "never by 0 twice in a row",
                 "the last tile N - a * HOP", "min((last + 1) * HOP,", "pos[0] = 0 at the tile's first frame", "A gap tile is +0.0",
                 "max(a, j - 3) ... j of its own tile only", "map[j] + R <= L", "R = floor((search + 1279) / 256)",
                 "at once when it is a gap frame", "window end (L + 1) * HOP", "at most map[j] + 2", "map[j] * HOP + search + 1279",
                 "a later `last` cannot change it", "at most 2 R hops", "not on how they were cut into pushes", "ring of 16",
                 "The lane has then ENDED", "at most 512", "1 ... 65535", "SSYM_E_EMPTY_DICT", "ordered by (lane, column)",
                 "nothing\n *   consumed", "no frame goes through the host", "Taking the same log twice", "SSYM_OUT_DEVICE",
                 "One synchronisation per call", "main_ms = the search, reduce_ms = staging and synthesis", "2^31 - 1 frames"):
        assert line in doc, line
    # the kernels: three of them here, the search step shared with wsola_search_kernel through the header both include
    assert re.findall(r"__global__[^\n]*void (\w+)\(", resynth) == ["resynth_init_kernel", "resynth_feed_kernel", "resynth_search_kernel",
                                                                   "resynth_synth_kernel"]
    assert common.count("int wsola_step(") == 1 and "wsola_step(" in wsola and "wsola_step(" in resynth
    for name in ("wsola_sums(", "wsola_beats("):
        assert name in common and name not in wsola and name not in resynth
    assert '#include "lane_feed.hpp"' in resynth and '#include "warp_common.hpp"' in resynth
    assert "check_handle(" in resynth and "check_lane_room(" in resynth and "LaneLog out{1}" in resynth
    assert "resynthesiser (resynth.hip)" in _read("soundsym_amd", "csrc", "lane_feed.hpp")
    for word in ("__dadd_rn", "__dmul_rn", "__ddiv_rn", "warp_pcm32", "p < wlen"):
        assert word in resynth, word
    kernels = resynth[resynth.index("__global__"):resynth.index("void resynth_free")]
    for word in ("atomic", "asm", "while (true)", "cooperative"):
        assert word not in kernels, word
    make = _read("soundsym_amd", "csrc", "Makefile")
    assert " resynth.hip " in make and re.search(r"\$\(BUILD\)/resynth\.o[^\n]*: warp_common\.hpp", make)
    assert re.search(r"\$\(BUILD\)/resynth\.o[^\n]*: lane_feed\.hpp", make)
    assert "resynth.mk" in _read("__graft_entry__.py")


def test_null_handles_are_refused_without_a_device(native_lib):
    u = np.full(4, 7, dtype=np.uint32)
    f = np.full(4, -1.5)
    n = np.full(1, 9, dtype=np.uint64)
    p = lambda a: a.ctypes.data
    count = n.ctypes.data_as(native_lib.ssym_resynth_push.argtypes[8])
    assert native_lib.ssym_resynth_create(None, None, 1, 0, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_resynth_push(None, None, p(u), p(u), p(u), p(u), p(u), 4, count) == nat.SSYM_E_INVALID
    assert native_lib.ssym_resynth_take(None, None, None, count) == nat.SSYM_E_INVALID
    assert native_lib.ssym_resynth_samples(None, None, p(n), p(f), p(u), 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_resynth_flush(None, None, 0, 0, count) == nat.SSYM_E_INVALID
    assert native_lib.ssym_resynth_counts(None, p(n), p(n)) == nat.SSYM_E_INVALID
    assert native_lib.ssym_resynth_reset(None, None, 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_resynth_destroy(None, None) == nat.SSYM_OK         # destroying nothing is fine
    assert (u == 7).all() and (f == -1.5).all() and n[0] == 9


class _Lib:
    """Records the entry points a call makes; every call succeeds and writes nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return nat.SSYM_OK
        return call


class _Store:
    ptr = None


def test_resynth_calls_and_their_checks(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    store = _Store()
    for bad in (513, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="search"):
            e.resynth(store, 1, bad)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="n_lanes"):
            e.resynth(store, bad)
    assert lib.calls == []
    rs = e.resynth(store, 2, 300)
    assert isinstance(rs, Resynth) and rs.store is store and (rs.n_lanes, rs.search, rs.n_samples) == (2, 300, 0)
    for call in (lambda: rs.push([0], [0, 1], [0], [0], [1]), lambda: rs.flush(2, 0), lambda: rs.flush(-1, 0), lambda: rs.flush(0, -1),
                 lambda: rs.flush(0, 2.5), lambda: rs.reset(2)):
        with pytest.raises(ValueError):
            call()

    class _Mk:
        n_lanes, ptr = 3, None
    with pytest.raises(ValueError, match="take"):
        rs.take(_Mk())
    assert lib.calls == [("ssym_resynth_create", 5)]
    lib.calls.clear()
    assert rs.push([0, 1], [0, 0], [0, 0], [3, 4], [1, 1]) == 0 and rs.flush(1, 700) == 0
    _Mk.n_lanes = 2
    assert rs.take(_Mk()) == 0
    off, smp, pcm = rs.samples(want_pcm32=True)
    assert (off.shape, off.dtype, smp.shape, smp.dtype, pcm.shape, pcm.dtype) == ((3,), np.uint64, (0,), np.float64, (0,), np.int32)
    assert len(rs.samples()) == 2
    frames, released = rs.counts()
    assert frames.shape == released.shape == (2,) and frames.dtype == released.dtype == np.uint64
    rs.reset(1)
    rs.close()
    rs.close()
    assert lib.calls == [("ssym_resynth_push", 9), ("ssym_resynth_flush", 5), ("ssym_resynth_take", 4), ("ssym_resynth_samples", 6),
                         ("ssym_resynth_samples", 6), ("ssym_resynth_counts", 3), ("ssym_resynth_reset", 3)]     # (ctx is None: nothing to destroy)


class _FakeEngine:
    """Enough of an Engine for the checks that come before any library call; anything else fails loudly."""
    np_dtype = np.float64
    metric = "dtw"

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


def test_mosaic_live_checks_the_audio_arguments_before_any_library_call():
    from soundsym_amd import Sound
    rng = np.random.default_rng(0xA13)
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = [Sound(rng.standard_normal(20 * HOP), 8000.0, rng.standard_normal(20 * 5), "s", ncoeffs=5)]
    for kw in ({"search": 513}, {"search": -1}, {"search": 1.5}, {"gap_fill": "noise"}):
        with pytest.raises(ValueError, match="search|gap_fill"):
            d.mosaic_live(d.sounds, 1.0, None, audio=True, **kw)
    with pytest.raises(ValueError, match="share one stream"):
        d.mosaic_live(d.sounds, 1.0, None, audio=True, search=8, gap_fill="target")
    with pytest.raises(ValueError, match="share one stream"):
        d.mosaic_live(d.sounds, 1.0, None, search=9999, gap_fill="unused")       # without audio they are not looked at


def test_live_mosaic_audio_gathers_per_sound_and_fills_gaps_on_the_host():
    G = nat.COVER_GAP

    class _Mk:
        n_lanes = 2

        def __init__(self):
            # (lane, column, src, frame, cost, start)
            self.batches = [([0, 0, 1], [0, 1, 0], [3, G, G], [5, nat.NO_MATCH, nat.NO_MATCH], [1.0, 4.0, 4.0], [1, 1, 1]),
                            ([0], [2], [1], [2], [0.25], [1]), ([], [], [], [], [], [])]

        def follow(self, stream):
            self.now = self.batches.pop(0)

        def flush(self, lane):
            self.now = self.batches.pop(0)

        def frames(self):
            lane, col, src, frame, cost, start = self.now
            u = lambda v: np.array(v, dtype=np.uint32)
            return u(lane), u(col), u(src), u(frame), np.array(cost, dtype=np.float64), u(start)

        def close(self):
            pass

    class _Rs:
        """Releases one hop per frame taken, valued 0.5 (pcm 7), and the tail at the flush."""
        n_samples = 0

        def __init__(self, mk):
            self.mk, self.log = mk, []

        def take(self, mk):
            lane = np.array(mk.now[0], dtype=np.int64)
            self.sizes = [int((lane == l).sum()) * HOP for l in range(2)]
            self.n_samples = sum(self.sizes)
            self.log.append("take")

        def flush(self, lane, total):
            self.sizes = [total - 3 * HOP if l == lane == 0 else (total - HOP if l == lane else 0) for l in range(2)]
            self.n_samples = sum(self.sizes)
            self.log.append(("flush", lane, total))

        def samples(self, want_pcm32=False):
            off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.uint64)
            return off, np.full(self.n_samples, 0.5), np.full(self.n_samples, 7, dtype=np.int32)

        def close(self):
            self.log.append("close")

    class _Snd:
        def __init__(self, n):
            self.x = np.arange(n, dtype=np.float64) / 4096.0

        def samples(self):
            return self.x

    sounds = [_Snd(3 * HOP + 10), _Snd(HOP + 5)]
    mk = _Mk()
    live = LiveMosaic(sounds, object(), mk, 2.0, 4.0, _Rs(mk), "target")
    live.poll()
    a, b = live.audio(want_pcm32=True)
    assert a[0].size == 2 * HOP and (a[0][:HOP] == 0.5).all() and (a[1][:HOP] == 7).all()
    assert np.array_equal(a[0][HOP:], sounds[0].x[HOP:2 * HOP])          # the gap frame: the sound's own samples
    assert np.array_equal(a[1][HOP:], np.trunc(2147483647.0 * sounds[0].x[HOP:2 * HOP]).astype(np.int32))
    assert np.array_equal(b[0], sounds[1].x[:HOP])
    assert [x.size for x in live.audio()] == [0, 0]                      # nothing comes twice
    live.flush()
    a, b = live.audio()
    assert a.size == HOP + 10 and (a == 0.5).all()                       # lane 0 ends in a sounding tile
    assert np.array_equal(b, sounds[1].x[HOP:])                          # lane 1 ends in a gap: filled to the end
    assert live.resynth.log == ["take", "take", ("flush", 0, 3 * HOP + 10), "take", ("flush", 1, HOP + 5)]
    silent = LiveMosaic(sounds, object(), _Mk(), 2.0, 4.0)
    with pytest.raises(ValueError, match="without audio"):
        silent.audio()
    live.close()
    assert live.resynth.log[-1] == "close"
