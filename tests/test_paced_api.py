"""The paced spotting interface without a device: the header, the ctypes binding, the Rust declarations and the C++
mirror name the three _step symbols and the two constants; the limits the header states are the kernel's constants; the
Python argument checks come before any device work; the default step calls the existing entry points."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Sound, SoundDictionary, SoundSequence, Spot
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ssym_dtw_spot_step": 12, "ssym_spot_queries_step": 10, "ssym_dtw_spot_all_step": 15}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbols_and_constants(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    for name, nargs in NEW.items():
        assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % name, header), name
        assert name in nat.ABI_SYMBOLS and name in soundsym_amd.ABI_SYMBOLS
        assert re.search(r"pub fn %s\s*\(" % name, rust), name
        assert name + "(" in mirror
        assert hasattr(native_lib, name) and len(getattr(native_lib, name).argtypes) == nargs
        # the same parameters in the same order in the header and in the Rust declaration, `step` behind index_base
        rust_names = re.findall(r"(\w+):", rust[rust.index("pub fn %s" % name):].split(";")[0])
        c_names = names(header, name + "(ssym_ctx")
        assert c_names == rust_names and len(c_names) == nargs
        assert c_names[c_names.index("index_base") + 1] == "step"
        # the existing call's parameters with `step` taken out
        assert [x for x in c_names if x != "step"] == names(header, name[:-len("_step")] + "(ssym_ctx")
    assert "#define SSYM_STEP_SYMMETRIC 0u" in header and "#define SSYM_STEP_PACED 1u" in header
    assert (nat.STEP_SYMMETRIC, nat.STEP_PACED) == (0, 1)
    assert "pub const SSYM_STEP_SYMMETRIC: u32 = 0;" in rust and "pub const SSYM_STEP_PACED: u32 = 1;" in rust
    assert "SSYM_STEP_SYMMETRIC" in mirror
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header      # additions only
    # the declarations follow ssym_dtw_spot_all's: the comments above keep their places
    assert header.index("ssym_dtw_spot_all(ssym_ctx") < header.index("Paced spotting (DESIGN.md") < header.index("ssym_dtw_spot_step(ssym_ctx")


def test_header_states_the_definition_and_the_kernels_limits():
    src, header = _read("soundsym_amd", "csrc", "dtw_spot.hip"), _read("include", "soundsym_amd.h")
    frames = int(re.search(r"kPacedMaxTargetFrames\s*=\s*(\d+);", src).group(1))
    assert frames == 2048
    doc = header[header.index("Paced spotting (DESIGN.md"):header.index("ssym_dtw_spot_step(ssym_ctx")]
    assert "targets of at most %d frames" % frames in doc and "dim <= 64" in doc and "24 bytes of LDS per target frame" in doc
    for line in ("N(i,0) = c(i,0), sN(i,0) = i", "H(i,0) = +inf", "if H(i,j) < N(i,j): (H, sH)", "if E(i-2,j-1) < P: E(i-2,j-1)",
                 "N(i,j) = c(i,j) + P.value", "H(i,j) = c(i,j) + N(i,j-1)", "floor((Fb-1)/2) + 1", "2 Fb - 1"):
        assert line in doc, line
    assert "SSYM_E_INVALID" in doc and "SSYM_E_UNSUPPORTED" in doc and "unnormalised" in doc
    # two hand-off rows and the ring stay inside the 160 KiB of LDS at the limit, and would not at 4096 frames
    ring = 128 * 66 * 8
    assert frames * 24 + ring <= 160 * 1024 < 4096 * 24 + ring


def test_null_context_and_unknown_step_are_refused_without_a_device(native_lib):
    idx = np.zeros(1, dtype=np.uint32)
    cost = np.full(2, -1.5)
    word = np.full(5, 7, dtype=np.uint32)
    for step in (nat.STEP_SYMMETRIC, nat.STEP_PACED, 7):
        assert native_lib.ssym_dtw_spot_step(None, None, None, idx.ctypes.data, None, 1, 0, step, cost.ctypes.data,
                                             word.ctypes.data, word[1:].ctypes.data, 0) == nat.SSYM_E_INVALID
        assert native_lib.ssym_spot_queries_step(None, None, None, 0, step, word.ctypes.data, cost.ctypes.data,
                                                 word[1:].ctypes.data, word[2:].ctypes.data, 0) == nat.SSYM_E_INVALID
        assert native_lib.ssym_dtw_spot_all_step(None, None, None, idx.ctypes.data, None, 1, 0, step, 2, None, word.ctypes.data,
                                                 cost.ctypes.data, word[1:].ctypes.data, word[3:].ctypes.data,
                                                 0) == nat.SSYM_E_INVALID
    assert (cost == -1.5).all() and (word == 7).all()


class _Handle:
    ptr, n = None, 2


class _Lib:
    """Records the entry points an Engine method calls; every call succeeds and writes nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return nat.SSYM_OK
        return call


def _engine(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    return e, lib


def test_the_default_step_calls_the_existing_symbols(monkeypatch):
    e, lib = _engine(monkeypatch)
    h = _Handle()
    for kw in ({}, {"step": "symmetric"}):
        lib.calls.clear()
        e.dtw_spot(h, h, [0, 1], **kw)
        e.spot_queries(h, h, **kw)
        e.dtw_spot_all(h, h, [0, 1], max_spots=3, **kw)
        assert lib.calls == [("ssym_dtw_spot", 11), ("ssym_spot_queries", 9), ("ssym_dtw_spot_all", 14)]
    lib.calls.clear()
    e.dtw_spot(h, h, [0, 1], step="paced")
    e.spot_queries(h, h, step="paced")
    e.dtw_spot_all(h, h, [0, 1], max_spots=3, step="paced")
    assert lib.calls == [("ssym_dtw_spot_step", 12), ("ssym_spot_queries_step", 10), ("ssym_dtw_spot_all_step", 15)]
    lib.calls.clear()
    for call in (e.dtw_spot, e.dtw_spot_device, e.dtw_spot_all, e.dtw_spot_all_device):
        with pytest.raises(ValueError):
            call(h, h, [0, 1], step="itakura")
    with pytest.raises(ValueError):
        e.spot_queries(h, h, step="")
    assert lib.calls == []                                       # an unknown step is refused before the library is asked


class _FakeEngine:
    """Enough of an Engine for the checks that come before any device work; anything else fails loudly."""
    np_dtype = np.float64

    def __init__(self, metric="dtw"):
        self.metric = metric

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


def _recordings():
    rng = np.random.default_rng(0xC08)
    return [Sound(rng.standard_normal(frames * HOP), 8000.0 + k, rng.standard_normal((frames, 5)).reshape(-1), "rec%d" % k,
                  ncoeffs=5) for k, frames in enumerate((20, 7))]


def test_argument_errors_come_before_any_device_work():
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = _recordings()
    t = _recordings()
    for call in (d.spot, d.spot_all):
        with pytest.raises(ValueError):
            call(t, step="itakura")
        with pytest.raises(ValueError):
            call(t, step=1)
    with pytest.raises(ValueError):
        d.spot_all(t, step="paced", max_cost=1.0, max_cost_per_frame=1.0)          # exclusive
    with pytest.raises(ValueError):
        d.spot_all(t, max_cost_per_frame=1.0)                                      # paced only
    with pytest.raises(ValueError):
        d.spot_all(t, step="symmetric", max_cost_per_frame=1.0)
    with pytest.raises(ValueError):
        d.spot_all(t, step="paced", max_cost_per_frame=float("nan"))
    with pytest.raises(ValueError):
        d.spot_all(t, step="paced", max_cost_per_frame=[1.0, 2.0])                 # per-target thresholds need indices
    with pytest.raises(ValueError):
        d.spot_all(t, step="paced", indices=[0, 1], max_cost_per_frame=[1.0])      # one threshold per target
    seq = SoundSequence.new(t)
    with pytest.raises(ValueError):
        seq.spot_all_in_dictionary(d, max_cost_per_frame=1.0)
    with pytest.raises(ValueError):
        seq.spot_in_dictionary(d, step="itakura")
    assert d.spot_all([], step="paced", max_cost_per_frame=1.0) == [] and d.spot([], step="paced") == []


class _RecordingEngine:
    """An engine that answers dtw_spot_all with one occurrence per pair and keeps what it was asked."""
    np_dtype = np.float64
    metric = "dtw"

    class _Q:
        def close(self):
            pass

    def dictionary(self, *a):
        return object()

    def queries(self, *a):
        return self._Q()

    def dtw_spot_all(self, d, q, src, tgt, max_spots, max_cost, **kw):
        self.asked = (np.asarray(src), np.asarray(tgt), max_cost, kw)
        n = len(src)
        return (np.ones(n, dtype=np.uint32), np.full((n, max_spots), 3.0), np.zeros((n, max_spots), dtype=np.uint32),
                np.ones((n, max_spots), dtype=np.uint32))


def test_max_cost_per_frame_becomes_a_sum_per_pair_and_spots_carry_the_mean():
    e = _RecordingEngine()
    d = SoundDictionary(engine=e)
    d.sounds = _recordings()
    t = _recordings()                                                             # targets of 20 and of 7 frames
    out = d.spot_all(t, max_spots=2, step="paced", max_cost_per_frame=0.3)
    src, tgt, max_cost, kw = e.asked
    assert kw == {"step": "paced"} and tgt.tolist() == [0, 1, 0, 1]
    assert np.array_equal(max_cost, np.float64(0.3) * np.array([20.0, 7.0, 20.0, 7.0]))        # x * Fb[p] in f64
    assert [sp.cost_per_frame for sp in out[0]] == [3.0 / 20, 3.0 / 20] and [sp.cost_per_frame for sp in out[1]] == [3.0 / 7] * 2
    d.spot_all(t, indices=[1, 0], max_spots=2, step="paced", max_cost_per_frame=[0.5, 2.0])
    assert np.array_equal(e.asked[2], np.array([0.5 * 20.0, 2.0 * 7.0]))
    out = d.spot_all(t, max_spots=2, max_cost=4.0)                                # the default: the call as it was
    assert e.asked[3] == {} and float(e.asked[2]) == 4.0 and out[0][0].cost_per_frame is None


def test_spot_value_class_keeps_its_four_arguments():
    s = Spot(3, 10, 14, 2.5)
    assert s.cost_per_frame is None and s.num_frames() == 5
    assert Spot(3, 10, 14, 2.5, 0.5).cost_per_frame == 0.5 and Spot.none().cost_per_frame is None


def test_example_and_tool_take_the_new_options():
    ex = _read("examples", "occurrences.py")
    assert "--paced" in ex and "--max-cost-per-frame" in ex
    tool = _read("tools", "paced_timing.py")
    assert 'step="paced"' in tool and "dtw_spot_all" in tool
