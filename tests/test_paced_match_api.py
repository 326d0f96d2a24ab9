"""The paced matching interface without a device: the header, the ctypes binding, the Rust declaration and the C++ mirror
name the two calls; the header states the definition and the kernel's limits; the refusals that need no device; the Python
checks of `step`, `match_step` and `per_frame` come before any library call; every default calls what it called before."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH, MATRIX = "ssym_match_queries_step", "ssym_pair_matrix_step"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbols(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    for name, nargs, plain in ((MATCH, 9, "ssym_match_queries"), (MATRIX, 5, "ssym_pair_matrix")):
        assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % name, header)
        assert name in nat.ABI_SYMBOLS and name in soundsym_amd.ABI_SYMBOLS
        assert re.search(r"pub fn %s\s*\(" % name, rust) and name + "(ctx_->get()" in mirror
        assert hasattr(native_lib, name) and len(getattr(native_lib, name).argtypes) == nargs
        c_names = names(header, name + "(ssym_ctx")
        assert c_names == re.findall(r"(\w+):", rust[rust.index("pub fn %s" % name):].split(";")[0]) and len(c_names) == nargs
        assert "step" in c_names
        theirs = names(header, plain + "(ssym_ctx")
        assert [x for x in c_names if x != "step"] == [x for x in theirs if x != "exact"]      # the plain call's, step put in
    assert names(header, MATCH + "(ssym_ctx")[5] == "step"                                     # behind index_base
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header       # additions only


def test_header_states_the_definition_and_the_kernels_limits():
    src, align, header = (_read("soundsym_amd", "csrc", "dtw_match_paced.hip"), _read("soundsym_amd", "csrc", "dtw_align.hip"),
                          _read("include", "soundsym_amd.h"))
    const = lambda text, name: int(re.search(r"\b%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    fa, fb, dim = (const(src, k) for k in ("kMatchPacedMaxSrcFrames", "kMatchPacedMaxTgtFrames", "kMatchPacedMaxDim"))
    # ssym_dtw_align_step's, so that every reported match can be aligned
    assert (fa, fb, dim) == (const(align, "kAlignMaxFrames"), const(align, "kAlignPacedMaxTargetFrames"), const(align, "kAlignMaxDim"))
    doc = header[header.index("Paced matching (DESIGN.md"):header.index(MATCH + "(ssym_ctx")]
    assert "every target of at most %d and every source of at\n * most %d frames" % (fb, fa) in doc and "dim <= %d" % dim in doc
    for line in ("floor((Fb-1)/2) + 1 ... 2 Fb - 1", "argmin_s |cost(s,t) - distance[t]|", "the fold starts at (0, +inf)",
                 "a NaN or +inf key never wins", "0 + index_base and +inf", "SSYM_DTW_FORCE_EXACT and SSYM_DTW_PRUNE mean nothing",
                 "SSYM_E_INVALID", "SSYM_E_UNSUPPORTED", "SSYM_E_EMPTY_DICT", "main_ms = the forward kernel, reduce_ms = the fold"):
        assert line in doc, line
    # LDS at the limits: two f64 hand-off rows and the ring at DIMR = 64
    assert 2 * fb * 8 + 128 * 66 * 8 <= 160 * 1024
    # the kernel is in the build, with its dependence on the shared header
    make = _read("soundsym_amd", "csrc", "Makefile")
    assert " dtw_match_paced.hip " in make and re.search(r"\$\(BUILD\)/dtw_match_paced\.o[^\n]*: dtw_wave\.hpp", make)


def test_null_context_and_unknown_step_are_refused_without_a_device(native_lib):
    idx = np.full(2, 7, dtype=np.uint32)
    cost = np.full(2, -1.5)
    for step in (nat.STEP_SYMMETRIC, nat.STEP_PACED, 7):
        assert native_lib.ssym_match_queries_step(None, None, None, None, 0, step, idx.ctypes.data, cost.ctypes.data, 0) == nat.SSYM_E_INVALID
        assert native_lib.ssym_pair_matrix_step(None, None, None, step, cost.ctypes.data) == nat.SSYM_E_INVALID
    assert (cost == -1.5).all() and (idx == 7).all()


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


def test_the_default_step_calls_the_existing_symbols(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    h = _Handle()
    for kw in ({}, {"step": "symmetric"}):
        lib.calls.clear()
        e.match(h, h, **kw)
        e.match(h, h, [1.0, 2.0], index_base=4, force_exact=True, **kw)
        e.pair_matrix(h, h, **kw)
        e.pair_matrix(h, h, exact=True, **kw)
        assert lib.calls == [("ssym_match_queries", 8)] * 2 + [("ssym_pair_matrix", 5)] * 2
    lib.calls.clear()
    e.match(h, h, step="paced")
    e.match(h, h, [1.0, 2.0], index_base=4, step="paced")
    e.pair_matrix(h, h, step="paced")
    assert lib.calls == [(MATCH, 9)] * 2 + [(MATRIX, 5)]
    lib.calls.clear()
    for call in (e.match, e.pair_matrix):
        for bad in ("itakura", "", 1, None):
            with pytest.raises(ValueError):
                call(h, h, step=bad)
    assert lib.calls == []                                       # an unknown step is refused before the library is asked


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


def test_step_errors_come_before_any_library_call():
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = _sounds()
    t = _sounds()
    seq = SoundSequence.new(t)
    stepped = (lambda **kw: d.match_indices(t, **kw), lambda **kw: seq.clone_from_dictionary(d, **kw),
               lambda **kw: seq.morph_to([1.0, 2.0], d, **kw))
    for call in stepped:
        for bad in ("itakura", "", 1, None):
            with pytest.raises(ValueError, match="step must be"):
                call(step=bad)
    # per_frame without step="paced": a symmetric cost is no sum over the target's frames
    for call in stepped[0::2]:
        for kw in ({}, {"step": "symmetric"}):
            with pytest.raises(ValueError, match="per_frame needs"):
                call(per_frame=True, **kw)
    matched = (lambda **kw: d.align(t, **kw), lambda **kw: d.warp(t, **kw), lambda **kw: seq.align_to_dictionary(d, **kw),
               lambda **kw: seq.reconstruct_warped_from_dictionary(d, **kw))
    for call in matched:
        for kw in ({}, {"step": "symmetric"}):
            with pytest.raises(ValueError, match='match_step="paced" needs step="paced"'):
                call(match_step="paced", **kw)
        for bad in ("itakura", "", 1):
            with pytest.raises(ValueError, match="step must be"):
                call(step="paced", match_step=bad)
    assert d.align([], step="paced", match_step="paced") == []
    assert SoundSequence.new([]).align_to_dictionary(d, step="paced", match_step="paced") == []
    assert SoundSequence.new([]).clone_from_dictionary(d, step="paced").sounds() == []


class _RecordingEngine:
    """An engine that answers the calls of a match and an alignment and keeps the keywords it was given."""
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

    def match(self, d, q, distance=None, **kw):
        self.asked.append(("match", None if distance is None else np.asarray(distance).tolist(), kw))
        return np.array([1, 0], dtype=np.uint32), np.array([40.0, 21.0])

    def match_batch(self, d, flat, off, distance=None):
        self.asked.append(("match_batch", None if distance is None else np.asarray(distance).tolist(), {}))
        return np.array([1, 0], dtype=np.uint32), np.array([40.0, 21.0])

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


def test_the_defaults_pass_no_keyword_on_and_paced_passes_the_step():
    e = _RecordingEngine()
    d = SoundDictionary(engine=e)
    d.sounds = _sounds()
    t = _sounds()
    seq = SoundSequence.new(t)
    # the symmetric search stays ssym_match_batch, whatever spelling asks for it
    d.match_indices(t)
    d.match_indices(t, [3.0, 4.0], step="symmetric")
    seq.clone_from_dictionary(d)
    seq.morph_to([3.0, 4.0], d)
    assert e.asked == [("match_batch", None, {}), ("match_batch", [3.0, 4.0], {}), ("match_batch", None, {}),
                       ("match_batch", [3.0, 4.0], {})]
    e.asked.clear()
    # paced: one resident query set, the step passed on; per_frame multiplies the distances by the targets' frames (20 and 7)
    # and divides the costs by them
    idx, cost = d.match_indices(t, [3.0, 4.0], step="paced")
    assert cost.tolist() == [40.0, 21.0]
    idx, cost = d.match_indices(t, [3.0, 4.0], step="paced", per_frame=True)
    assert idx.tolist() == [1, 0] and cost.tolist() == [40.0 / 20.0, 21.0 / 7.0]
    seq.clone_from_dictionary(d, step="paced")
    seq.morph_to([0.5, 1.5], d, step="paced", per_frame=True)
    assert e.asked == [("match", [3.0, 4.0], {"step": "paced"}), ("match", [60.0, 28.0], {"step": "paced"}),
                       ("match", None, {"step": "paced"}), ("match", [10.0, 10.5], {"step": "paced"})]
    e.asked.clear()
    # match_step: None and "symmetric" are the calls as they were; "paced" reaches the match, the step the alignment
    d.align(t)
    d.align(t, step="paced")
    d.align(t, step="paced", match_step="symmetric")
    d.warp(t, step="paced")
    assert e.asked == [("match", None, {}), ("dtw_align", {}), ("match", None, {}), ("dtw_align", {"step": "paced"}),
                       ("match", None, {}), ("dtw_align", {"step": "paced"}), ("match", None, {}), ("dtw_align_device", {"step": "paced"})]
    e.asked.clear()
    d.align(t, step="paced", match_step="paced")
    d.warp(t, step="paced", match_step="paced")
    seq.align_to_dictionary(d, step="paced", match_step="paced")
    seq.reconstruct_warped_from_dictionary(d, step="paced", match_step="paced")
    assert e.asked == [("match", None, {"step": "paced"}), ("dtw_align", {"step": "paced"}),
                       ("match", None, {"step": "paced"}), ("dtw_align_device", {"step": "paced"})] * 2
    e.asked.clear()
    d.align(t, [0, 1], step="paced", match_step="paced")            # with indices nothing is searched
    assert e.asked == [("dtw_align", {"step": "paced"})]
