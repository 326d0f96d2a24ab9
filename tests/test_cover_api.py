"""The cover's surface without a device: Piece / Cover arithmetic, segment_lengths, the ValueErrors that come before any
library call, and header, binding, Rust declaration and C++ mirror holding to each other."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Cover, Piece, Sound, SoundDictionary, SoundSequence, SsymError
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = "ssym_dtw_cover"
INF = float("inf")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbol(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % COVER, header)
    assert COVER in nat.ABI_SYMBOLS and COVER in soundsym_amd.ABI_SYMBOLS
    assert re.search(r"pub fn %s\s*\(" % COVER, rust) and COVER + "(ctx_->get()" in mirror
    assert hasattr(native_lib, COVER) and len(getattr(native_lib, COVER).argtypes) == 11
    c_names = names(header, COVER + "(ssym_ctx")
    assert c_names == ["ctx", "dict", "q", "piece_penalty", "flags", "out_count", "out_total", "out_src", "out_start",
                       "out_end", "out_cost"]
    assert c_names == re.findall(r"(\w+):", rust[rust.index("pub fn %s" % COVER):].split(";")[0])
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header       # additions only


def test_header_states_the_definition_and_the_kernels_limits():
    src, header = _read("soundsym_amd", "csrc", "dtw_cover.hip"), _read("include", "soundsym_amd.h")
    const = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, src).group(1))
    frames, dim = const("kCoverMaxSourceFrames"), const("kCoverMaxDim")
    assert frames >= 128 and dim == 64 and const("kCoverScratchBytes") == 512 and "512ull << 20" in src
    assert const("kCoverRing") > 2 * frames and const("kCoverRing") & (const("kCoverRing") - 1) == 0
    doc = header[header.index("Cover (DESIGN.md"):header.index(COVER + "(ssym_ctx")]
    for line in ("at most %d frames (kCoverMaxSourceFrames)" % frames, "dim <= %d" % dim,
                 "frames x 2 Fmax x 12 + frames x 16 bytes <= 512 MiB", "ceil((Fa+1)/2) ... 2 Fa", "best(-1)  = 0",
                 "v = (M(e-L+1, L) + piece_penalty) + best(e-L)", "(SSYM_NO_MATCH,\n *               SSYM_NO_MATCH, SSYM_NO_MATCH, +inf)",
                 "SSYM_E_INVALID", "SSYM_E_UNSUPPORTED", "SSYM_E_EMPTY_DICT", "main_ms = the forward pass",
                 "reduce_ms = the chain", "SSYM_OUT_DEVICE"):
        assert line in doc, line
    # LDS at the limit: E, N and a c tile of at least 8 columns for one start fit a workgroup; 2 Fmax chain candidates fit
    # four per lane
    assert frames * 8 * (3 + 8) <= 160 * 1024 and 2 * frames <= const("kCoverRing")
    make = _read("soundsym_amd", "csrc", "Makefile")
    assert " dtw_cover.hip " in make and re.search(r"\$\(BUILD\)/dtw_cover\.o[^\n]*: dtw_wave\.hpp", make)


def test_null_context_is_refused_without_a_device(native_lib):
    u = np.full(4, 7, dtype=np.uint32)
    f = np.full(4, -1.5)
    for penalty in (0.0, -1.0, float("nan")):
        rc = native_lib.ssym_dtw_cover(None, None, None, penalty, 0, u.ctypes.data, f.ctypes.data, u.ctypes.data, u.ctypes.data,
                                       u.ctypes.data, f.ctypes.data)
        assert rc == nat.SSYM_E_INVALID
    assert (u == 7).all() and (f == -1.5).all()


# -- Piece and Cover ---------------------------------------------------------------------------------------------------------

def test_piece_arithmetic():
    p = Piece(3, 4, 9, 1.5)
    assert (p.source_index, p.start_frame, p.end_frame, p.cost) == (3, 4, 9, 1.5)
    assert p.num_frames() == 6 and p.cost_per_frame == 0.25
    assert p.sample_span(100 * HOP) == (4 * HOP, 10 * HOP)
    assert p.sample_span(10 * HOP - 7) == (4 * HOP, 10 * HOP - 7)          # the last frame ends with the sound
    assert Piece(0, 0, 0, 2.0).cost_per_frame == 2.0 and Piece(0, 0, 0, 2.0).sample_span(5) == (0, 5)
    assert "frames=4...9" in repr(p)
    for bad in ((0, 3, 2, 0.0), (0, -1, 2, 0.0), (-1, 0, 0, 0.0)):
        with pytest.raises(ValueError):
            Piece(*bad)


def test_cover_arithmetic():
    c = Cover([Piece(1, 0, 2, 3.0), Piece(0, 3, 4, 1.0), Piece(1, 5, 9, 0.5)], 4.5, 10)
    assert len(c) == 3 and bool(c) and c.total == 4.5 and c.total_per_frame == 0.45
    assert c.indices().dtype == np.int64 and c.indices().tolist() == [1, 0, 1]
    none = Cover.none(7)
    assert len(none) == 0 and not none and none.total == INF and none.total_per_frame == INF and none.num_frames == 7
    assert none.indices().size == 0 and none.segment_lengths(123) == [] and repr(none) == "Cover(empty)"
    # the pieces tile the target
    for pieces, frames in (([Piece(0, 1, 2, 0.0)], 3), ([Piece(0, 0, 2, 0.0), Piece(0, 4, 5, 0.0)], 6),
                           ([Piece(0, 0, 2, 0.0), Piece(0, 2, 5, 0.0)], 6), ([Piece(0, 0, 2, 0.0)], 4), ([(0, 0, 2, 0.0)], 3)):
        with pytest.raises(ValueError, match="tile the target"):
            Cover(pieces, 0.0, frames)
    with pytest.raises(ValueError):
        Cover([], INF, -1)


def test_segment_lengths_are_what_from_segments_takes():
    c = Cover([Piece(1, 0, 2, 3.0), Piece(0, 3, 4, 1.0), Piece(1, 5, 9, 0.5)], 4.5, 10)
    n = 10 * HOP + 300                                               # samples behind the last whole frame go to the last piece
    lens = c.segment_lengths(n)
    assert lens == [3 * HOP, 2 * HOP, n - 5 * HOP] and sum(lens) == n and all(isinstance(x, int) for x in lens)
    assert c.segment_lengths(5 * HOP) == [3 * HOP, 2 * HOP, 0]
    with pytest.raises(ValueError, match="longer sound"):
        c.segment_lengths(5 * HOP - 1)
    with pytest.raises(ValueError):
        c.segment_lengths(-1)
    rng = np.random.default_rng(1)
    sound = Sound(rng.standard_normal(n), 8000.0, rng.standard_normal((10, 5)).reshape(-1), "t", ncoeffs=5)
    cut = SoundDictionary.from_segments(sound, lens, engine=_FakeEngine()).sounds
    seq = SoundSequence.from_cover(sound, c).sounds()
    assert [s.samples().size for s in cut] == lens == [s.samples().size for s in seq]
    assert [s.num_frames() for s in seq] == [3, 2, 5]
    for a, b, p in zip(cut, seq, c.pieces):
        assert np.array_equal(a.samples(), b.samples())
        assert np.array_equal(b.mfcc_arrays(), sound.mfcc_arrays()[p.start_frame:p.end_frame + 1])
        assert np.array_equal(a.mfccs()[:b.mfccs().size], b.mfccs()[:a.mfccs().size])      # from_segments takes seg / HOP rows
    assert np.array_equal(np.concatenate([s.samples() for s in seq]), sound.samples())
    assert SoundSequence.from_cover(sound, Cover.none(10)).sounds() == []
    with pytest.raises(ValueError, match="another number of frames"):
        SoundSequence.from_cover(sound, Cover([Piece(0, 0, 3, 0.0)], 0.0, 4))
    with pytest.raises(ValueError, match="a Cover is needed"):
        SoundSequence.from_cover(sound, [Piece(0, 0, 9, 0.0)])


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
    for bad in (-1.0, float("nan"), INF, -INF, -1e-300):
        with pytest.raises(ValueError, match="piece_penalty must be finite and not negative"):
            d.cover(t, bad)
        with pytest.raises(ValueError, match="piece_penalty must be finite and not negative"):
            d.reconstruct_covered(t[0], bad)
    for bad in ("x", None):
        with pytest.raises((ValueError, TypeError)):
            d.cover(t, bad)
    for bad in (-1, 513, 1.5):
        with pytest.raises(ValueError):
            d.reconstruct_covered(t[0], 0.0, search=bad)
    with pytest.raises(ValueError, match="takes one Sound"):
        d.reconstruct_covered(t)
    assert d.cover([]) == []
    with pytest.raises(soundsym_amd.EmptyDictionaryError):
        SoundDictionary(engine=_FakeEngine()).cover(t)
    refcos = SoundDictionary(engine=_FakeEngine("refcos"))
    refcos.sounds = _sounds()
    with pytest.raises(SsymError) as err:
        refcos.cover(t)
    assert err.value.code == nat.SSYM_E_UNSUPPORTED
    with pytest.raises(SsymError) as err:
        refcos.reconstruct_covered(t[0])
    assert err.value.code == nat.SSYM_E_UNSUPPORTED


class _Handle:
    ptr, n = None, 2
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


def test_engine_call_and_its_penalty_check(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    h = _Handle()
    out = e.dtw_cover(h, h)
    assert [(x.shape, x.dtype) for x in out] == [((2,), np.uint32), ((2,), np.float64), ((7,), np.uint32), ((7,), np.uint32),
                                                 ((7,), np.uint32), ((7,), np.float64)]
    e.dtw_cover(h, h, 2.5)
    assert lib.calls == [(COVER, 11)] * 2
    lib.calls.clear()
    for bad in (-1.0, float("nan"), INF):
        with pytest.raises(ValueError):
            e.dtw_cover(h, h, bad)
    assert lib.calls == []
