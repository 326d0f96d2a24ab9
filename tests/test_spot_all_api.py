"""The occurrences interface without a device: the header, the ctypes binding, the Rust declarations and the C++ mirror
name ssym_dtw_spot_all; the limits the header states are the kernel's constants; the Python argument checks come before
any device work."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ssym_dtw_spot_all"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


class _FakeEngine:
    """Enough of an Engine for the checks that come before any device work; anything else fails loudly."""
    np_dtype = np.float64

    def __init__(self, metric="dtw"):
        self.metric = metric

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


def test_header_binding_rust_and_mirror_name_the_symbol(native_lib):
    header, rust = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs")
    assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % NAME, header)
    assert NAME in nat.ABI_SYMBOLS and NAME in soundsym_amd.ABI_SYMBOLS
    assert re.search(r"pub fn %s\s*\(" % NAME, rust)
    assert hasattr(native_lib, NAME)
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header      # additions only
    mirror = _read("include", "soundsym.hpp")
    assert "spot_all(" in mirror and "ssym_dtw_spot_all(" in mirror
    assert len(native_lib.ssym_dtw_spot_all.argtypes) == 14
    # the declaration follows ssym_spot_queries': the spotting comment keeps its place
    assert header.index("ssym_spot_queries(ssym_ctx") < header.index("ssym_dtw_spot_all(ssym_ctx")
    # the same parameters in the same order in the header and in the Rust declaration
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    rust_names = re.findall(r"(\w+):", rust[rust.index("pub fn %s" % NAME):].split(";")[0])
    assert names(header, "ssym_dtw_spot_all(ssym_ctx") == rust_names and len(rust_names) == 14


def test_header_states_the_kernels_limits():
    src, header = _read("soundsym_amd", "csrc", "dtw_spot.hip"), _read("include", "soundsym_amd.h")
    spots = int(re.search(r"kSpotAllMaxSpots\s*=\s*(\d+);", src).group(1))
    frames = int(re.search(r"kSpotAllMaxSourceFrames\s*=\s*(\d+);", src).group(1))
    assert (spots, frames) == (64, 2 ** 24)
    doc = header[header.index("Occurrences (DESIGN.md"):header.index("ssym_dtw_spot_all(ssym_ctx")]
    assert "1 ... %d" % spots in doc and "max_spots 0 or > %d" % spots in doc
    assert "2^24 = %d frames" % frames in doc and "12 bytes per source frame" in doc
    assert "targets of at most 4096 frames" in doc and "dim <= 64" in doc
    assert "NOT normalised" in doc and "SSYM_OUT_DEVICE" in doc


def test_null_context_is_refused_without_a_device(native_lib):
    idx = np.zeros(1, dtype=np.uint32)
    cost = np.full(2, -1.5)
    word = np.full(5, 7, dtype=np.uint32)
    limit = np.zeros(1)
    rc = native_lib.ssym_dtw_spot_all(None, None, None, idx.ctypes.data, None, 1, 0, 2, limit.ctypes.data, word.ctypes.data,
                                      cost.ctypes.data, word[1:].ctypes.data, word[3:].ctypes.data, 0)
    assert rc == nat.SSYM_E_INVALID
    assert (cost == -1.5).all() and (word == 7).all()


def _recordings():
    rng = np.random.default_rng(0xC07)
    out = []
    for k, (n_samples, frames) in enumerate([(20 * HOP + 100, 20), (7 * HOP, 7)]):
        out.append(Sound(rng.standard_normal(n_samples), 8000.0 + k, rng.standard_normal((frames, 5)).reshape(-1),
                         "rec%d" % k, ncoeffs=5))
    return out


def test_argument_errors_come_before_any_device_work():
    with pytest.raises(soundsym_amd.EmptyDictionaryError):
        SoundDictionary(engine=_FakeEngine()).spot_all([])
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = _recordings()
    t = _recordings()
    assert d.spot_all([]) == [] and d.spot_all([], indices=[]) == []
    with pytest.raises(ValueError):
        d.spot_all(t, indices=[0])                    # one index per target
    with pytest.raises(ValueError):
        d.spot_all(t, indices=[0, 2])                 # outside the dictionary
    with pytest.raises(ValueError):
        d.spot_all(t, indices=[-1, 0])
    for k in (0, 65, -1):
        with pytest.raises(ValueError):
            d.spot_all(t, max_spots=k)
    with pytest.raises(ValueError):
        d.spot_all(t, max_cost=float("nan"))
    with pytest.raises(ValueError):
        d.spot_all(t, indices=[0, 1], max_cost=[1.0])             # one threshold per target
    with pytest.raises(ValueError):
        d.spot_all(t, max_cost=[1.0, 2.0])                        # per-target thresholds need indices
    r = SoundDictionary(engine=_FakeEngine("refcos"))
    r.sounds = _recordings()
    with pytest.raises(soundsym_amd.SsymError) as err:
        r.spot_all(t)
    assert err.value.code == nat.SSYM_E_UNSUPPORTED
    assert SoundSequence.new([]).spot_all_in_dictionary(d) == []
    # Engine: the pair list, K and the thresholds, before the library is asked
    E = soundsym_amd.Engine
    for call in (E.dtw_spot_all, E.dtw_spot_all_device):
        with pytest.raises(ValueError):
            call(None, None, None, [0, 1], [0])
        for k in (0, 65):
            with pytest.raises(ValueError):
                call(None, None, None, [0, 1], max_spots=k)
        with pytest.raises(ValueError):
            call(None, None, None, [0, 1], max_cost=[1.0, 2.0, 3.0])
        with pytest.raises(ValueError):
            call(None, None, None, [0, 1], max_cost=[1.0, float("nan")])


def test_new_names_are_exported():
    for name in ("dtw_spot_all", "dtw_spot_all_device"):
        assert hasattr(soundsym_amd.Engine, name), name
    assert hasattr(SoundDictionary, "spot_all") and hasattr(SoundSequence, "spot_all_in_dictionary")
    assert NAME in soundsym_amd.ABI_SYMBOLS
