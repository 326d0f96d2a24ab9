"""The spotting interface without a device: the header, the ctypes binding, the Rust declarations and the C++ mirror name
the new entry points; the limits the header states are the kernel's constants; Spot, SoundDictionary.cut and the Python
argument checks."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Sound, SoundDictionary, SoundSequence, Spot
from soundsym_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ssym_dtw_spot", "ssym_spot_queries"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


class _FakeEngine:
    """Enough of an Engine for the checks that come before any device work; anything else fails loudly."""
    np_dtype = np.float64

    def __init__(self, metric="dtw"):
        self.metric = metric

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


def test_header_binding_rust_and_mirror_name_the_new_symbols(native_lib):
    header, rust = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs")
    for name in NEW:
        assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % name, header), name
        assert name in nat.ABI_SYMBOLS and name in soundsym_amd.ABI_SYMBOLS
        assert re.search(r"pub fn %s\s*\(" % name, rust), name
        assert hasattr(native_lib, name)
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header      # additions only
    mirror = _read("include", "soundsym.hpp")
    assert "spot(" in mirror and "ssym_dtw_spot(" in mirror and "ssym_spot_queries(" in mirror
    assert len(native_lib.ssym_dtw_spot.argtypes) == 11 and len(native_lib.ssym_spot_queries.argtypes) == 9


def test_header_states_the_kernels_limits():
    src, header = _read("soundsym_amd", "csrc", "dtw_spot.hip"), _read("include", "soundsym_amd.h")
    frames = int(re.search(r"kSpotMaxTargetFrames\s*=\s*(\d+);", src).group(1))
    dim = int(re.search(r"kSpotMaxDim\s*=\s*(\d+);", src).group(1))
    assert (frames, dim) == (4096, 64)
    doc = header[header.index("DTW spotting"):header.index("ssym_dtw_spot(ssym_ctx")]
    assert "targets of at most %d frames" % frames in doc and "dim <= %d" % dim in doc
    assert "2^31 - 1 frames" in doc and "NOT normalised" in doc
    assert "dtw_spot.hip" in _read("soundsym_amd", "csrc", "Makefile")


def test_null_context_is_refused_without_a_device(native_lib):
    idx = np.zeros(1, dtype=np.uint32)
    cost = np.full(1, -1.5)
    word = np.full(3, 7, dtype=np.uint32)
    assert native_lib.ssym_dtw_spot(None, None, None, idx.ctypes.data, None, 1, 0, cost.ctypes.data, word.ctypes.data,
                                    word[1:].ctypes.data, 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_spot_queries(None, None, None, 0, word.ctypes.data, cost.ctypes.data, word[1:].ctypes.data,
                                        word[2:].ctypes.data, 0) == nat.SSYM_E_INVALID
    assert cost[0] == -1.5 and (word == 7).all()


def test_spot_value_class():
    s = Spot(3, 10, 14, 2.5)
    assert (s.source_index, s.start_frame, s.end_frame, s.cost) == (3, 10, 14, 2.5)
    assert s and not s.empty() and s.num_frames() == 5
    assert s.sample_span(100 * HOP) == (10 * HOP, 15 * HOP)
    assert s.sample_span(15 * HOP - 7) == (10 * HOP, 15 * HOP - 7)        # the last frame ends with the recording
    assert Spot(0, 4, 4, 0.0).num_frames() == 1 and Spot(0, 0, 0, 0.0)
    assert "frames=10...14" in repr(s)
    for e in (Spot.none(), Spot(nat.NO_MATCH, nat.NO_MATCH, nat.NO_MATCH, float("inf")), Spot(2, nat.NO_MATCH, nat.NO_MATCH, 1.0)):
        assert not e and e.empty() and e.num_frames() == 0 and e.sample_span(5000) == (0, 0)
    assert Spot.none().cost == float("inf") and "empty" in repr(Spot.none())
    with pytest.raises(ValueError):
        Spot(0, 5, 4, 0.0)
    with pytest.raises(ValueError):
        Spot(0, -1, 4, 0.0)


def _recordings():
    rng = np.random.default_rng(0xC07)
    out = []
    for k, (n_samples, frames) in enumerate([(20 * HOP + 100, 20), (7 * HOP, 7)]):
        out.append(Sound(rng.standard_normal(n_samples), 8000.0 + k, rng.standard_normal((frames, 5)).reshape(-1),
                         "rec%d" % k, ncoeffs=5))
    return out


def test_cut_takes_samples_and_frames_of_every_spot():
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = _recordings()
    spots = [Spot(0, 2, 4, 1.0), Spot(1, 0, 6, 2.0), Spot.none(), Spot(0, 19, 19, 0.5), Spot(1, 6, 6, 0.0), Spot(0, 2, 4, 1.0)]
    c = d.cut(spots)
    assert isinstance(c, SoundDictionary) and len(c.sounds) == len(spots) and c._engine is d._engine
    for sp, got in zip(spots, c.sounds):
        if not sp:
            assert got.samples().size == 0 and got.num_frames() == 0 and got.ncoeffs == 5
            continue
        rec = d.sounds[sp.source_index]
        a, b = sp.sample_span(rec.samples().size)
        assert np.array_equal(got.samples(), rec.samples()[a:b])
        assert np.array_equal(got.mfcc_arrays(), rec.mfcc_arrays()[sp.start_frame:sp.end_frame + 1])
        assert got.num_frames() == sp.num_frames() and got.sample_rate() == rec.sample_rate() and got.ncoeffs == 5
    # the tail of a sound: recording 0 has 100 samples beyond its last whole hop, recording 1 ends on a hop
    assert c.sounds[3].samples().size == HOP and c.sounds[4].samples().size == HOP
    assert c.sounds[0].samples().size == 3 * HOP and c.sounds[1].samples().size == 7 * HOP
    short = Sound(d.sounds[0].samples()[:19 * HOP + 9], 8000.0, d.sounds[0].mfccs(), None, 5)
    d.sounds = [short]
    assert d.cut([Spot(0, 18, 19, 0.0)]).sounds[0].samples().size == HOP + 9
    # the copy is the dictionary's own
    c.sounds[0].samples()[:] = 0.0
    assert d.sounds[0].samples()[2 * HOP:5 * HOP].any()
    assert d.cut([]).sounds == []
    with pytest.raises(ValueError):
        d.cut([Spot(1, 0, 1, 0.0)])                   # a sound the dictionary does not hold
    with pytest.raises(ValueError):
        d.cut([Spot(0, 3, 20, 0.0)])                  # beyond the sound's frames


def test_argument_errors_come_before_any_device_work():
    with pytest.raises(soundsym_amd.EmptyDictionaryError):
        SoundDictionary(engine=_FakeEngine()).spot([])
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = _recordings()
    t = _recordings()
    assert d.spot([]) == [] and d.spot([], indices=[]) == []
    with pytest.raises(ValueError):
        d.spot(t, indices=[0])                        # one index per target
    with pytest.raises(ValueError):
        d.spot(t, indices=[0, 2])                     # outside the dictionary
    with pytest.raises(ValueError):
        d.spot(t, indices=[-1, 0])
    r = SoundDictionary(engine=_FakeEngine("refcos"))
    r.sounds = _recordings()
    with pytest.raises(soundsym_amd.SsymError) as err:
        r.spot(t)
    assert err.value.code == nat.SSYM_E_UNSUPPORTED
    assert SoundSequence.new([]).spot_in_dictionary(d) == []
    with pytest.raises(ValueError):
        soundsym_amd.Engine.dtw_spot(None, None, None, [0, 1], [0])       # the pair list, before the library is asked


def test_new_names_are_exported():
    assert "Spot" in soundsym_amd.__all__
    for name in ("dtw_spot", "dtw_spot_device", "spot_queries"):
        assert hasattr(soundsym_amd.Engine, name), name
    assert hasattr(SoundDictionary, "spot") and hasattr(SoundDictionary, "cut")
    assert hasattr(SoundSequence, "spot_in_dictionary")
