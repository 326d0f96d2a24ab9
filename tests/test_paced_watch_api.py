"""The paced watching interface without a device: the header, the ctypes binding, the Rust declarations and the C++ mirror
name ssym_spotter_create_step; the header states the definition and the kernel's limit; NULL handles are refused; the Python
argument checks come before any device work; the default step calls the existing entry point; a per-frame threshold
becomes a sum per target on the host."""
import ctypes
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import Sound, Spot
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ssym_spotter_create_step"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbol(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % NAME, header)
    assert NAME in nat.ABI_SYMBOLS and NAME in soundsym_amd.ABI_SYMBOLS
    assert re.search(r"pub fn %s\s*\(" % NAME, rust) and NAME + "(" in mirror
    assert hasattr(native_lib, NAME) and len(getattr(native_lib, NAME).argtypes) == 6
    c_names = names(header, NAME + "(ssym_ctx")
    rust_names = re.findall(r"(\w+):", rust[rust.index("pub fn %s" % NAME):].split(";")[0])
    assert c_names == rust_names and len(c_names) == 6
    # ssym_spotter_create's parameters with `step` behind max_cost
    assert c_names[c_names.index("max_cost") + 1] == "step"
    assert [x for x in c_names if x != "step"] == names(header, "ssym_spotter_create(ssym_ctx")
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header      # additions only
    # the declaration follows ssym_spotter_reset's: the comments above keep their places
    assert header.index("ssym_spotter_reset(ssym_ctx") < header.index("Paced watching (DESIGN.md") < header.index(NAME + "(ssym_ctx")


def test_header_and_design_state_the_definition_and_the_kernels_limit():
    src, spot, header = _read("soundsym_amd", "csrc", "dtw_spotter.hip"), _read("soundsym_amd", "csrc", "dtw_spot.hip"), _read("include", "soundsym_amd.h")
    frames = int(re.search(r"kSpotterPacedMaxTargetFrames\s*=\s*(\d+);", src).group(1))
    assert frames == int(re.search(r"kPacedMaxTargetFrames\s*=\s*(\d+);", spot).group(1)) == 2048
    doc = header[header.index("Paced watching (DESIGN.md"):header.index(NAME + "(ssym_ctx")]
    assert "targets of at most %d frames" % frames in doc and "24 bytes of LDS per target frame" in doc
    for line in ("rows n-1 and n-2 of E", "ssym_dtw_spot_step(SSYM_STEP_PACED)", "ssym_dtw_align_step(SSYM_STEP_PACED)",
                 "floor((Fb-1)/2) + 1", "2 Fb - 1", "WITHOUT ssym_spotter_reset", "SSYM_E_INVALID", "SSYM_E_UNSUPPORTED",
                 "24 bytes x (frames of all targets) x n_lanes", "max_cost[t] = x * Fb[t]"):
        assert line in doc, line
    # two hand-off rows and the ring at the limit and DIMR = 64: the LDS of the largest paced launch
    assert 2 * frames * 12 + 128 * 66 * 8 == 116736 <= 160 * 1024
    design = _read("DESIGN.md")
    assert '"Paced watching"' in design and "### 5.20" in design
    assert "Out of scope: the spotter under the paced pattern" not in design
    assert "dtw_watch_paced_kernel" in src and "dtw_watch_paced_kernel" in design


def test_null_handles_are_refused_without_a_device(native_lib):
    out = ctypes.c_void_p(5)
    limit = np.full(2, -1.5)
    for step in (nat.STEP_SYMMETRIC, nat.STEP_PACED, 7):
        assert native_lib.ssym_spotter_create_step(None, None, 1, None, step, ctypes.byref(out)) == nat.SSYM_E_INVALID
        assert native_lib.ssym_spotter_create_step(None, None, 1, limit.ctypes.data, step, None) == nat.SSYM_E_INVALID
    assert out.value == 5 and (limit == -1.5).all()


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


def _sounds(n, stream=None, frames=4, ncoeffs=5):
    rng = np.random.default_rng(0xA7)
    fr = [frames] * n if np.isscalar(frames) else frames
    out = [Sound(rng.standard_normal(2000), 8000.0, rng.standard_normal((fr[k], ncoeffs)).reshape(-1), "s%d" % k, ncoeffs=ncoeffs)
           for k in range(n)]
    for i, s in enumerate(out):
        s._stream = None if stream is None else (stream, i)
    return out


def test_python_argument_errors_come_before_any_device_work():
    e = _FakeEngine()
    st = _FakeStream(e, 2)
    targets = _sounds(2)
    watch = soundsym_amd.watch
    with pytest.raises(ValueError, match="needs step"):
        watch(_sounds(2, st), targets, engine=e, max_cost_per_frame=1.0)                       # paced only
    with pytest.raises(ValueError, match="needs step"):
        watch(_sounds(2, st), targets, engine=e, step="symmetric", max_cost_per_frame=1.0)
    with pytest.raises(ValueError, match="exclude each other"):
        watch(_sounds(2, st), targets, engine=e, step="paced", max_cost=1.0, max_cost_per_frame=1.0)
    for step in ("itakura", "", 1, None):
        with pytest.raises(ValueError, match="step must be"):
            watch(_sounds(2, st), targets, engine=e, step=step)
    with pytest.raises(ValueError):
        watch(_sounds(2, st), targets, engine=e, step="paced", max_cost_per_frame=float("nan"))
    with pytest.raises(ValueError):
        watch(_sounds(2, st), targets, engine=e, step="paced", max_cost_per_frame=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        watch(_sounds(2), targets, engine=e, step="paced")                                     # not resident, as ever

    class Q:
        n, dim, ptr = 3, 5, None
    for step in ("itakura", 0):
        with pytest.raises(ValueError):
            soundsym_amd.Engine.spotter(None, Q, step=step)
    assert soundsym_amd.Spotter(e, None, Q, 2).step == "symmetric" and soundsym_amd.Spotter(e, None, Q, 2, "paced").step == "paced"


class _Lib:
    """Records the entry points an Engine method calls; every call succeeds and writes nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return nat.SSYM_OK
        return call


def test_the_default_step_calls_the_existing_symbol(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0

    class Q:
        n, dim, ptr = 2, 5, None
    for kw in ({}, {"step": "symmetric"}):
        sp = e.spotter(Q, 3, **kw)
        assert sp.step == "symmetric"
        sp.ptr = None
    sp = e.spotter(Q, 3, max_cost=[1.0, 2.0], step="paced")
    assert sp.step == "paced" and sp.n_lanes == 3
    sp.ptr = None
    assert lib.calls == [("ssym_spotter_create", 5), ("ssym_spotter_create", 5), ("ssym_spotter_create_step", 6)]


class _RecordingEngine:
    """An engine that keeps what its spotter was asked for."""
    np_dtype = np.float64
    metric = "dtw"

    class _Q:
        def close(self):
            pass

    class _Sp:
        n_lanes = 1

        def __init__(self, step):
            self.step = step

        def events(self):
            u = lambda *v: np.array(v, dtype=np.uint32)
            return u(0, 0), u(0, 2), np.array([3.0, 1.5]), u(4, 9), u(8, 12)

        def best(self):
            return (np.array([[3.0, np.inf, 1.5]]), np.array([[4, nat.NO_MATCH, 9]], dtype=np.uint32),
                    np.array([[8, nat.NO_MATCH, 12]], dtype=np.uint32))

    def queries(self, *a):
        return self._Q()

    def spotter(self, q, n_lanes, max_cost, **kw):
        self.asked = (n_lanes, max_cost, kw)
        return self._Sp(kw.get("step", "symmetric"))


def test_max_cost_per_frame_becomes_a_sum_per_target_and_spots_carry_the_mean():
    e = _RecordingEngine()
    st = _FakeStream(e, 1)
    targets = _sounds(3, frames=[20, 0, 7])                                   # a target without frames among them
    w = soundsym_amd.watch(_sounds(1, st), targets, engine=e, step="paced", max_cost_per_frame=0.3)
    lanes, max_cost, kw = e.asked
    assert lanes == 1 and kw == {"step": "paced"}
    assert np.array_equal(max_cost, np.array([np.float64(0.3) * 20.0, np.inf, np.float64(0.3) * 7.0]))     # x * Fb[t] in f64; never NaN
    ev = w._events()
    assert [(l, t) for l, t, _ in ev] == [(0, 0), (0, 2)]
    assert [sp.cost_per_frame for _, _, sp in ev] == [3.0 / 20, 1.5 / 7] and ev[0][2].num_frames() == 5
    best = w.best()[0]
    assert best[0].cost_per_frame == 3.0 / 20 and not best[1] and best[2].cost_per_frame == 1.5 / 7
    soundsym_amd.watch(_sounds(1, st), targets, engine=e, step="paced", max_cost_per_frame=[0.5, 1.0, 2.0])
    assert np.array_equal(e.asked[1], np.array([10.0, np.inf, 14.0]))
    soundsym_amd.watch(_sounds(1, st), targets, engine=e, step="paced", max_cost=4.0)
    assert e.asked[1] == 4.0 and e.asked[2] == {"step": "paced"}               # a sum stays a sum
    w = soundsym_amd.watch(_sounds(1, st), targets, engine=e, max_cost=4.0)    # the default: the call as it was
    assert e.asked[1:] == (4.0, {}) and all(sp.cost_per_frame is None for _, _, sp in w._events())
    assert isinstance(w.best()[0][0], Spot) and w.best()[0][0].cost_per_frame is None


def test_example_and_tool_take_the_new_options():
    ex = _read("examples", "watch.py")
    assert "--paced" in ex and "--max-cost-per-frame" in ex and 'step="paced"' in ex
    tool = _read("tools", "spotter_timing.py")
    assert "--paced" in tool and "spotter(q, 1, **kw)" in tool
