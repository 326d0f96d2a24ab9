"""The watching interface without a device: the header, the ctypes binding, the Rust declarations and the C++ mirror name
the ssym_spotter_* symbols; the header states the kernel's limits; a NULL context is refused; the Python argument checks come
before any device work; the new names are exported."""
import ctypes
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import Sound
from soundsym_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ssym_spotter_create": 5, "ssym_spotter_destroy": 2, "ssym_spotter_push": 8, "ssym_spotter_follow": 7,
         "ssym_spotter_events": 8, "ssym_spotter_flush": 4, "ssym_spotter_best": 6, "ssym_spotter_counts": 2,
         "ssym_spotter_reset": 3}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


class _FakeEngine:
    """Enough of an Engine for the checks that come before any device work; anything else fails loudly."""
    np_dtype = np.float64

    def __init__(self, metric="dtw"):
        self.metric = metric

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


class _FakeStream:
    ptr = 1

    def __init__(self, engine, n_lanes, ncoeffs=5):
        self.engine, self.n_lanes, self.ncoeffs = engine, n_lanes, ncoeffs


def test_header_binding_rust_and_mirror_name_the_symbols(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    for name, n_args in NAMES.items():
        assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % name, header), name
        assert name in nat.ABI_SYMBOLS and name in soundsym_amd.ABI_SYMBOLS
        assert re.search(r"pub fn %s\s*\(" % name, rust), name
        assert hasattr(native_lib, name) and len(getattr(native_lib, name).argtypes) == n_args
        assert name + "(" in mirror, name
        rust_names = re.findall(r"(\w+):", rust[rust.index("pub fn %s" % name):].split(";")[0])
        assert names(header, name + "(") == rust_names and len(rust_names) == n_args, name
    assert "typedef struct ssym_spotter ssym_spotter;" in header and "pub struct SsymSpotter" in rust
    assert "class Spotter" in mirror
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header      # additions only


def test_header_states_the_limits_and_what_the_rule_is_not():
    src, header = _read("soundsym_amd", "csrc", "dtw_spotter.hip"), _read("include", "soundsym_amd.h")
    frames = int(re.search(r"kSpotterMaxTargetFrames\s*=\s*(\d+);", src).group(1))
    dim = int(re.search(r"kSpotterMaxDim\s*=\s*(\d+);", src).group(1))
    assert "kLaneMaxFrames" in src                      # the lane limit is the lane feed's, shared with the coverer
    lane = int(re.search(r"kLaneMaxFrames\s*=\s*(\d+);", _read("soundsym_amd", "csrc", "lane_feed.hpp")).group(1))
    assert (frames, dim, lane) == (4096, 64, 2 ** 31 - 1)
    assert "kSpotterScratchBytes = (size_t)512 << 20" in src
    doc = header[header.index("Watching (DESIGN.md"):header.index("ssym_spotter_create(ssym_ctx")]
    assert "targets of at most %d frames" % frames in doc and "dim <= %d" % dim in doc
    assert "2^31 - 1 = %d frames" % lane in doc and "512 MiB" in doc and "12 bytes per (pair, new row)" in doc
    assert "NOT ssym_dtw_spot_all's greedy" in doc and "NOT normalised" in doc and "SSYM_OUT_DEVICE" in doc
    assert "FOR AS LONG AS IT LIVES" in doc and "ssym_spotter_reset" in doc
    design = _read("DESIGN.md")
    assert '"Watching"' in design and "### 5.17" in design and "not `ssym_dtw_spot_all`'s greedy" in design


def test_null_context_is_refused_without_a_device(native_lib):
    L = native_lib
    n, out = ctypes.c_uint64(77), ctypes.c_void_p(5)
    x, off = np.full(4, -1.5), np.array([0, 1], dtype=np.uint64)
    word = np.full(6, 7, dtype=np.uint32)
    inv = nat.SSYM_E_INVALID
    assert L.ssym_spotter_create(None, None, 1, None, ctypes.byref(out)) == inv and out.value == 5
    assert L.ssym_spotter_push(None, None, x.ctypes.data, off.ctypes.data, 0, ctypes.byref(n), x.ctypes.data, word.ctypes.data) == inv
    assert L.ssym_spotter_follow(None, None, None, 0, ctypes.byref(n), x.ctypes.data, word.ctypes.data) == inv
    assert L.ssym_spotter_events(None, None, word.ctypes.data, word.ctypes.data, x.ctypes.data, word.ctypes.data, word.ctypes.data, 0) == inv
    assert L.ssym_spotter_flush(None, None, 0, ctypes.byref(n)) == inv
    assert L.ssym_spotter_best(None, None, x.ctypes.data, word.ctypes.data, word.ctypes.data, 0) == inv
    assert L.ssym_spotter_reset(None, None, 0) == inv
    assert L.ssym_spotter_counts(None, off.ctypes.data) == inv
    assert L.ssym_spotter_destroy(None, None) == nat.SSYM_OK                     # nothing to destroy
    assert n.value == 77 and (x == -1.5).all() and (word == 7).all() and off.tolist() == [0, 1]


def _sounds(n, stream=None, ncoeffs=5):
    rng = np.random.default_rng(0xA7)
    out = [Sound(rng.standard_normal(2000), 8000.0, rng.standard_normal((4, ncoeffs)).reshape(-1), "s%d" % k, ncoeffs=ncoeffs)
           for k in range(n)]
    for i, s in enumerate(out):
        s._stream = None if stream is None else (stream, i)
    return out


def test_python_argument_errors_come_before_any_device_work():
    e = _FakeEngine()
    targets = _sounds(2)
    with pytest.raises(ValueError):
        soundsym_amd.watch([], targets, engine=e)
    with pytest.raises(ValueError):
        soundsym_amd.watch(_sounds(2), targets, engine=e)                       # not resident: no stream
    st = _FakeStream(e, 2)
    mixed = _sounds(2, st)
    mixed[1]._stream = (_FakeStream(e, 2), 1)
    with pytest.raises(ValueError):
        soundsym_amd.watch(mixed, targets, engine=e)                            # two streams
    with pytest.raises(ValueError):
        soundsym_amd.watch(_sounds(2, st)[::-1], targets, engine=e)             # lanes out of order
    with pytest.raises(ValueError):
        soundsym_amd.watch(_sounds(1, st), targets, engine=e)                   # not every lane of the stream
    with pytest.raises(ValueError):
        soundsym_amd.watch(_sounds(2, st), targets, engine=_FakeEngine())       # another engine than the stream's
    with pytest.raises(ValueError):
        soundsym_amd.watch(_sounds(2, st), _sounds(2, ncoeffs=7), engine=e)
    with pytest.raises(ValueError):
        soundsym_amd.watch(_sounds(2, st), targets, max_cost=float("nan"), engine=e)
    with pytest.raises(ValueError):
        soundsym_amd.watch(_sounds(2, st), targets, max_cost=[1.0, 2.0, 3.0], engine=e)
    r = _FakeEngine("refcos")
    with pytest.raises(soundsym_amd.SsymError) as err:
        soundsym_amd.watch(_sounds(2, _FakeStream(r, 2)), targets, engine=r)
    assert err.value.code == nat.SSYM_E_UNSUPPORTED

    class Q:
        n, dim, ptr = 3, 5, None
    E = soundsym_amd.Engine
    for kw in (dict(n_lanes=0), dict(n_lanes=-2), dict(max_cost=[1.0, 2.0]), dict(max_cost=[1.0, float("nan"), 2.0]),
               dict(max_cost=float("nan"))):
        with pytest.raises(ValueError):
            E.spotter(None, Q, **kw)
    sp = soundsym_amd.Spotter(e, None, Q, 2)
    with pytest.raises(ValueError):
        sp.push(np.zeros(7))                                                   # not whole frames
    with pytest.raises(ValueError):
        sp.push(np.zeros(10))                                                  # two lanes need offsets
    with pytest.raises(ValueError):
        sp.push(np.zeros(10), [0, 2, 1])
    with pytest.raises(ValueError):
        sp.push(np.zeros(10), [0, 1, 3])                                       # beyond feats
    for call in (sp.flush, sp.reset):
        with pytest.raises(ValueError):
            call(2)
    with pytest.raises(ValueError):
        sp.follow(_FakeStream(e, 3))


def test_new_names_are_exported():
    for name in ("Spotter", "Watch", "watch"):
        assert hasattr(soundsym_amd, name) and name in soundsym_amd.__all__, name
    assert hasattr(soundsym_amd.Engine, "spotter")
    for name in ("push", "follow", "events", "flush", "best", "counts", "reset", "close"):
        assert hasattr(soundsym_amd.Spotter, name), name
    for name in ("poll", "flush", "best"):
        assert hasattr(soundsym_amd.Watch, name), name
    assert os.path.exists(os.path.join(ROOT, "examples", "watch.py"))
