"""The paced alignment interface without a device: the header, the ctypes binding, the Rust declaration and the C++
mirror name ssym_dtw_align_step with `step` behind index_base; the definition and the limits the header states are the
kernel's constants; the refusals that need no device; the Python `step` checks come before any device work; the default
step calls ssym_dtw_align."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "ssym_dtw_align_step", 15


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbol(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % NAME, header)
    assert NAME in nat.ABI_SYMBOLS and NAME in soundsym_amd.ABI_SYMBOLS
    assert re.search(r"pub fn %s\s*\(" % NAME, rust) and NAME + "(" in mirror
    assert hasattr(native_lib, NAME) and len(getattr(native_lib, NAME).argtypes) == NARGS
    rust_names = re.findall(r"(\w+):", rust[rust.index("pub fn %s" % NAME):].split(";")[0])
    c_names = names(header, NAME + "(ssym_ctx")
    assert c_names == rust_names and len(c_names) == NARGS
    assert c_names[c_names.index("index_base") + 1] == "step"
    assert [x for x in c_names if x != "step"] == names(header, "ssym_dtw_align(ssym_ctx")      # ssym_dtw_align's, step put in
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header         # additions only
    assert header.index("ssym_dtw_spot_all_step(ssym_ctx") < header.index("Paced alignment (DESIGN.md") < header.index(NAME + "(ssym_ctx")
    # the mirror's align takes the step and keeps the plain call for the default
    body = mirror[mirror.index("std::vector<Alignment> align("):mirror.index("std::vector<double> warp(")]
    assert "uint32_t step = SSYM_STEP_SYMMETRIC" in body and "ssym_dtw_align(ctx_->get()" in body and NAME + "(ctx_->get()" in body


def test_header_states_the_definition_and_the_kernels_limits():
    src, spot, header = _read("soundsym_amd", "csrc", "dtw_align.hip"), _read("soundsym_amd", "csrc", "dtw_spot.hip"), _read("include", "soundsym_amd.h")
    const = lambda text, name: int(re.search(r"\b%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    tgt, frames, dim, dirs = (const(src, k) for k in ("kAlignPacedMaxTargetFrames", "kAlignMaxFrames", "kAlignMaxDim", "kAlignDirLdsBytes"))
    assert (tgt, frames, dim) == (2048, 4096, 64)
    assert tgt == const(spot, "kPacedMaxTargetFrames")                  # every span paced spotting reports can be aligned
    doc = header[header.index("Paced alignment (DESIGN.md"):header.index(NAME + "(ssym_ctx")]
    assert "targets of at most %d frames" % tgt in doc and "sources of at most %d frames" % frames in doc and "dim <= %d" % dim in doc
    for line in ("floor((Fb-1)/2) + 1 ... 2 Fb - 1", "N(0,0) = c(0,0);  N(i,0) = +inf for i >= 1;  H(i,0) = +inf",
                 "E(i,j) = N(i,j); if H(i,j) < N(i,j): H(i,j)", "P = E(i-1,j-1); if E(i-2,j-1) < P: E(i-2,j-1)",
                 "N(i,j) = c(i,j) + P;   H(i,j) = c(i,j) + N(i,j-1)", "cost    = E(Fa-1,Fb-1);  L = Fb if the cost is finite, else 0",
                 "state H at (i,j): the cell before is (i, j-1), in state N.", "path[j] = (i_j, j);  map[j] = i_j"):
        assert line in doc, line
    assert "SSYM_E_INVALID" in doc and "SSYM_E_UNSUPPORTED" in doc and "ssym_dtw_align_sizes leaves at least that" in doc
    # LDS at the limits: two f64 hand-off rows, the ring at DIMR = 64, one word per target frame, the directions
    lds = 2 * tgt * 8 + 128 * 66 * 8 + tgt * 4 + dirs
    assert lds == 124928 and lds <= 160 * 1024


def test_null_context_and_unknown_step_are_refused_without_a_device(native_lib):
    idx = np.zeros(1, dtype=np.uint32)
    off = np.array([0, 4], dtype=np.uint64)
    cost = np.full(2, -1.5)
    word = np.full(12, 7, dtype=np.uint32)
    for step in (nat.STEP_SYMMETRIC, nat.STEP_PACED, 7):
        assert native_lib.ssym_dtw_align_step(None, None, None, idx.ctypes.data, None, 1, 0, step, cost.ctypes.data,
                                              word.ctypes.data, off.ctypes.data, word[1:].ctypes.data, off.ctypes.data,
                                              word[9:].ctypes.data, 0) == nat.SSYM_E_INVALID
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
    monkeypatch.setattr(engine_mod, "_output", lambda device, shape, t: (np.zeros(shape, dtype=t), 0))
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    return e, lib


def test_the_default_step_calls_the_existing_symbol(monkeypatch):
    e, lib = _engine(monkeypatch)
    h = _Handle()
    for kw in ({}, {"step": "symmetric"}):
        lib.calls.clear()
        e.dtw_align(h, h, [0, 1], **kw)
        e.dtw_align_device(h, h, [0, 1], **kw)
        assert lib.calls == [("ssym_dtw_align_sizes", 8), ("ssym_dtw_align", 14)] * 2
    lib.calls.clear()
    e.dtw_align(h, h, [0, 1], step="paced")
    e.dtw_align_device(h, h, [0, 1], step="paced")
    assert lib.calls == [("ssym_dtw_align_sizes", 8), (NAME, NARGS)] * 2
    lib.calls.clear()
    for call in (e.dtw_align, e.dtw_align_device):
        with pytest.raises(ValueError):
            call(h, h, [0, 1], step="itakura")
        with pytest.raises(ValueError):
            call(h, h, [0, 1], step=1)
    assert lib.calls == []                                       # an unknown step is refused before the library is asked


class _FakeEngine:
    """Enough of an Engine for the checks that come before any device work; anything else fails loudly."""
    np_dtype = np.float64

    def __init__(self, metric="dtw"):
        self.metric = metric

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


def _sounds():
    rng = np.random.default_rng(0xA11)
    return [Sound(rng.standard_normal(frames * HOP), 8000.0 + k, rng.standard_normal((frames, 5)).reshape(-1), "s%d" % k,
                  ncoeffs=5) for k, frames in enumerate((20, 7))]


def test_step_errors_come_before_any_device_work():
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = _sounds()
    t = _sounds()
    seq = SoundSequence.new(t)
    for call in (lambda **kw: d.align(t, [0, 1], **kw), lambda **kw: d.warp(t, [0, 1], **kw),
                 lambda **kw: seq.align_to_dictionary(d, **kw), lambda **kw: seq.reconstruct_warped_from_dictionary(d, **kw)):
        for bad in ("itakura", "", 1, None):
            with pytest.raises(ValueError):
                call(step=bad)
    assert d.align([], step="paced") == [] and SoundSequence.new([]).align_to_dictionary(d, step="paced") == []


class _RecordingEngine:
    """An engine that answers the alignment calls with nothing found and keeps the keywords it was given."""
    np_dtype = np.float64
    metric = "dtw"

    class _Q:
        n = 2

        def close(self):
            pass

    def __init__(self):
        self.asked = []

    def dictionary(self, *a):
        return self._Q()

    def samples(self, *a):
        return self._Q()

    def queries(self, *a):
        return self._Q()

    def dtw_align(self, d, q, indices, **kw):
        self.asked.append(("dtw_align", kw))
        n = len(indices)
        return np.full(n, np.inf), np.zeros(n, np.uint32), [np.zeros((0, 2), np.uint32)] * n, [np.zeros(0, np.uint32)] * n

    def dtw_align_device(self, d, q, indices, **kw):
        self.asked.append(("dtw_align_device", kw))
        n = len(indices)
        return None, np.zeros(n, np.uint32), None, np.zeros(27, np.uint32), None, np.array([0, 20, 27], np.uint64)

    def reconstruct_warped(self, *a):
        return np.zeros(3)


def test_the_default_passes_no_keyword_on_and_paced_passes_the_step():
    e = _RecordingEngine()
    d = SoundDictionary(engine=e)
    d.sounds = _sounds()
    t = _sounds()
    seq = SoundSequence.new(t)
    d.align(t, [0, 1])
    d.align(t, [0, 1], step="symmetric")
    d.warp(t, [0, 1])
    assert e.asked == [("dtw_align", {}), ("dtw_align", {}), ("dtw_align_device", {})]
    e.asked.clear()
    out = d.align(t, [0, 1], step="paced")
    d.warp(t, [1, 0], step="paced")
    assert e.asked == [("dtw_align", {"step": "paced"}), ("dtw_align_device", {"step": "paced"})]
    assert [len(a) for a in out] == [0, 0] and all(np.isposinf(a.cost) for a in out)
    e.asked.clear()
    e.match = lambda d_, q: (np.array([1, 0]), np.zeros(2))
    seq.align_to_dictionary(d, step="paced")
    seq.reconstruct_warped_from_dictionary(d, step="paced")
    seq.align_to_dictionary(d)
    assert e.asked == [("dtw_align", {"step": "paced"}), ("dtw_align_device", {"step": "paced"}), ("dtw_align", {})]
