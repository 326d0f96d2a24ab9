"""The span interface without a device: the header, the ctypes binding, the Rust declaration and the C++ mirror name the four
calls; without spans / windows every Engine method calls the symbol it called before, with the arguments it passed before;
spans exclude indices and match_step before any library call; an empty Spot becomes a pair without a source and an empty
window; context=True changes the windows' lengths and nothing else; a NULL context is refused without a device."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import HOP, Alignment, Sound, SoundDictionary, SoundSequence, Spot
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, ALIGN, WARPED, WSOLA = ("ssym_dtw_align_spans_sizes", "ssym_dtw_align_spans", "ssym_reconstruct_warped_spans",
                               "ssym_reconstruct_wsola_spans")
NO = nat.NO_MATCH


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_symbols(native_lib):
    header, rust, mirror = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs"), _read("include", "soundsym.hpp")
    names = lambda text, start: re.findall(r"(\w+)\s*[,)]", text[text.index(start):].split(";")[0])
    plain = {SIZES: ("ssym_dtw_align_sizes", ("span_first", "span_last")),
             ALIGN: ("ssym_dtw_align_step", ("span_first", "span_last")),
             WARPED: ("ssym_reconstruct_warped", ("win_first", "win_len")),
             WSOLA: ("ssym_reconstruct_wsola", ("win_first", "win_len"))}
    for name, nargs in ((SIZES, 10), (ALIGN, 17), (WARPED, 14), (WSOLA, 16)):
        assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % name, header)
        assert name in nat.ABI_SYMBOLS and name in soundsym_amd.ABI_SYMBOLS
        assert re.search(r"pub fn %s\s*\(" % name, rust)
        assert name + ("(resident()" if name == SIZES else "(ctx_->get()") in mirror
        assert hasattr(native_lib, name) and len(getattr(native_lib, name).argtypes) == nargs
        c_names = names(header, "SSYM_API int32_t %s(" % name)
        assert c_names == re.findall(r"(\w+):", rust[rust.index("pub fn %s(" % name):].split(";")[0]) and len(c_names) == nargs
        # the existing call's arguments in its order, the two new ones put in behind the indices
        theirs, added = plain[name]
        assert [x for x in c_names if x not in added] == names(header, "SSYM_API int32_t %s(" % theirs)
        at = c_names.index(added[0])
        assert tuple(c_names[at:at + 2]) == added and c_names[at - 1] in ("tgt_idx", "idx")
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header       # additions only


def test_header_states_the_semantics_and_the_kernels_are_the_existing_ones():
    header, align = _read("include", "soundsym_amd.h"), _read("soundsym_amd", "csrc", "dtw_align.hip")
    const = lambda text, name: int(re.search(r"\b%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    doc = header[header.index("Span alignment (DESIGN.md"):header.index("SSYM_API int32_t " + SIZES)]
    for line in ("RELATIVE TO THE SPAN", "map[0] = 0", "Fa' + Fb - 1 cells and Fb map entries", "SSYM_E_INVALID", "SSYM_E_UNSUPPORTED",
                 "Fa' <= %d" % const(align, "kAlignMaxFrames"), "<= %d under SSYM_STEP_PACED" % const(align, "kAlignPacedMaxTargetFrames"),
                 "dim <= %d" % const(align, "kAlignMaxDim"), "span_first[p] == span_last[p] == SSYM_NO_MATCH", "before any device work"):
        assert line in doc, line
    doc = header[header.index("Sample windows (DESIGN.md"):header.index("SSYM_API int32_t " + WARPED)]
    for line in ("win_len[t] = 0 is allowed", "0 <= nom + d < sLen", "relative to the window", "never influence an output",
                 "SSYM_E_INVALID", "before any device work"):
        assert line in doc, line
    # one kernel text for segments and spans: no kernel of the three files was added, none takes a span argument
    for path, kernels in (("dtw_align.hip", ["dtw_align_kernel", "dtw_align_paced_kernel"]), ("warp.hip", ["warp_kernel"]),
                          ("wsola.hip", ["wsola_search_kernel", "wsola_synth_kernel"])):
        src = _read("soundsym_amd", "csrc", path)
        assert re.findall(r"__global__[^\n]*void (\w+)\(", src) == kernels
    # (the two resynthesis files take their common arguments, WarpArgs, from warp_common.hpp, which holds no kernel)
    src = "".join(_read("soundsym_amd", "csrc", path) for path in ("dtw_align.hip", "warp_common.hpp", "warp.hip", "wsola.hip"))
    assert "__global__" not in _read("soundsym_amd", "csrc", "warp_common.hpp")
    structs = re.findall(r"struct (AlignArgs|WarpArgs|WsolaArgs)( : WarpArgs)? \{(.*?)\n\};", src, re.S)
    assert [(name, base) for name, base, _ in structs] == [("AlignArgs", ""), ("WarpArgs", ""), ("WsolaArgs", " : WarpArgs")]
    for _, _, struct in structs:
        assert "span" not in struct.lower() and "win_" not in struct and "window table" not in struct


def test_null_context_is_refused_without_a_device(native_lib):
    u32 = np.full(4, 7, dtype=np.uint32)
    u64 = np.full(4, 7, dtype=np.uint64)
    f64 = np.full(4, -1.5)
    p = lambda a: a.ctypes.data
    for step in (nat.STEP_SYMMETRIC, nat.STEP_PACED, 7):
        assert native_lib.ssym_dtw_align_spans(None, None, None, p(u32), None, p(u32), p(u32), 1, 0, step, p(f64), p(u32),
                                               p(u64), p(u32), p(u64), p(u32), 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_dtw_align_spans_sizes(None, None, p(u32), None, p(u32), p(u32), 1, 0, p(u64), p(u64)) == nat.SSYM_E_INVALID
    assert native_lib.ssym_reconstruct_warped_spans(None, None, p(u32), p(u64), p(u64), p(u64), 1, p(u32), p(u64), p(u32), None,
                                                    0, p(f64), None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_reconstruct_wsola_spans(None, None, p(u32), p(u64), p(u64), p(u64), 1, p(u32), p(u64), p(u32), None,
                                                   7, 0, None, p(f64), None) == nat.SSYM_E_INVALID
    assert (u32 == 7).all() and (u64 == 7).all() and (f64 == -1.5).all()


class _Handle:
    ptr, n = None, 2


class _Lib:
    """Records the entry points an Engine method calls and their arguments; every call succeeds and writes nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return nat.SSYM_OK
        return call

    def names(self):
        return [(name, len(args)) for name, args in self.calls]


def _engine(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device, e.metric = None, 0, "dtw"
    return e, lib


def test_without_spans_the_existing_symbols_are_called_with_unchanged_arguments(monkeypatch):
    e, lib = _engine(monkeypatch)
    h = _Handle()
    for kw in ({}, {"spans": None}):
        lib.calls.clear()
        e.dtw_align(h, h, [0, 1], **kw)
        e.dtw_align(h, h, [0, 1], step="paced", **kw)
        e.dtw_align_sizes(h, h, [0, 1], **kw)
        assert lib.names() == [("ssym_dtw_align_sizes", 8), ("ssym_dtw_align", 14), ("ssym_dtw_align_sizes", 8),
                               ("ssym_dtw_align_step", 15), ("ssym_dtw_align_sizes", 8)]
        assert lib.calls[3][1][7] == nat.STEP_PACED and lib.calls[1][1][5:7] == (2, 0)
    one = np.zeros(1, dtype=np.uint32)
    off = np.array([0, 300], dtype=np.uint64)
    moff = np.array([0, 1], dtype=np.uint64)
    for kw in ({}, {"windows": None}):
        lib.calls.clear()
        e.reconstruct_warped(h, one, off, one, moff, [1], **kw)
        e.reconstruct_wsola(h, one, off, one, moff, [1], search=9, **kw)
        assert lib.names() == [("ssym_reconstruct_warped", 12), ("ssym_reconstruct_wsola", 14)]
        warped, wsola = lib.calls[0][1], lib.calls[1][1]
        assert warped[4] == 1 and warped[9] == 0 and wsola[4] == 1 and wsola[9:11] == (9, 0)


def test_spans_and_windows_reach_the_new_symbols(monkeypatch):
    e, lib = _engine(monkeypatch)
    h = _Handle()
    first, last = np.array([3, NO], dtype=np.uint32), np.array([9, NO], dtype=np.uint32)
    e.dtw_align(h, h, [0, NO], spans=(first, last))
    e.dtw_align(h, h, [0, NO], spans=(first, last), step="paced", index_base=5)
    assert lib.names() == [(SIZES, 10), (ALIGN, 17)] * 2
    args = lib.calls[3][1]
    assert args[5:10] == (first.ctypes.data, last.ctypes.data, 2, 5, nat.STEP_PACED) and args[16] == 0
    assert lib.calls[2][1][4:8] == (first.ctypes.data, last.ctypes.data, 2, 5)
    lib.calls.clear()
    one = np.zeros(1, dtype=np.uint32)
    off, moff = np.array([0, 300], dtype=np.uint64), np.array([0, 1], dtype=np.uint64)
    wf, wl = np.array([768], dtype=np.uint64), np.array([512], dtype=np.uint64)
    e.reconstruct_warped(h, one, off, one, moff, [1], windows=(wf, wl))
    e.reconstruct_wsola(h, one, off, one, moff, [1], search=9, windows=(wf, wl))
    assert lib.names() == [(WARPED, 14), (WSOLA, 16)]
    assert lib.calls[0][1][3:5] == (wf.ctypes.data, wl.ctypes.data) and lib.calls[0][1][6] == 1
    assert lib.calls[1][1][3:5] == (wf.ctypes.data, wl.ctypes.data) and lib.calls[1][1][11:13] == (9, 0)
    lib.calls.clear()
    for bad in ((first,), (first, last[:1]), (first[:1], last[:1])):
        with pytest.raises(ValueError):
            e.dtw_align(h, h, [0, 1], spans=bad)
    with pytest.raises(ValueError):
        e.reconstruct_warped(h, one, off, one, moff, [1], windows=(wf, np.zeros(2, dtype=np.uint64)))
    assert lib.calls == []


class _FakeEngine:
    """Enough of an Engine for the checks that come before any library call; anything else fails loudly."""
    np_dtype = np.float64
    metric = "dtw"

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


def _sounds():
    rng = np.random.default_rng(0xA12)
    return [Sound(rng.standard_normal(n), 8000.0, rng.standard_normal((frames, 5)).reshape(-1), "s%d" % k, ncoeffs=5)
            for k, (frames, n) in enumerate(((20, 20 * HOP + 100), (7, 7 * HOP - 60)))]


def test_spans_exclude_indices_and_match_step_before_any_library_call():
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = _sounds()
    t = _sounds()
    spots = [Spot(0, 2, 9, 1.0), Spot(1, 0, 6, 2.0)]
    for call in (d.align, d.warp):
        with pytest.raises(ValueError, match="indices and match_step do not go with them"):
            call(t, [0, 1], spans=spots)
        with pytest.raises(ValueError, match="indices and match_step do not go with them"):
            call(t, spans=spots, step="paced", match_step="paced")
        with pytest.raises(ValueError, match="indices and match_step do not go with them"):
            call(t, spans=spots, match_step="symmetric")
        with pytest.raises(ValueError, match="one Spot per target"):
            call(t, spans=spots[:1])
        with pytest.raises(ValueError, match="one Spot per target"):
            call(t, spans=[(0, 2, 9), (1, 0, 6)])
        with pytest.raises(ValueError, match="outside the dictionary"):
            call(t, spans=[Spot(2, 0, 1, 0.0), spots[1]])
        with pytest.raises(ValueError, match="beyond its sound's frames"):
            call(t, spans=[spots[0], Spot(1, 0, 7, 0.0)])
        with pytest.raises(ValueError, match="step must be"):
            call(t, spans=spots, step="itakura")
    with pytest.raises(ValueError, match="context"):
        d.warp(t, context=True)
    assert d.align([], spans=[]) == []
    assert d.warp([], spans=[]).size == 0


class _RecordingEngine:
    """An engine that answers an alignment and a reconstruction and keeps what it was given."""
    np_dtype = np.float64
    metric = "dtw"

    class _Q:
        n = 3

        def close(self):
            pass

    def __init__(self):
        self.asked = []

    def dictionary(self, *a):
        return self._Q()

    samples = queries = dictionary

    def spot_queries(self, d, q, **kw):
        self.asked.append(("spot_queries", kw))
        return (np.array([1, 0, NO], dtype=np.uint32), np.array([3.0, 4.0, np.inf]), np.array([1, 2, NO], dtype=np.uint32),
                np.array([5, 9, NO], dtype=np.uint32))

    def dtw_align(self, d, q, src, **kw):
        self.asked.append(("dtw_align", np.asarray(src).tolist(), kw))
        n = len(src)
        return np.full(n, np.inf), np.zeros(n, np.uint32), [np.zeros((0, 2), np.uint32)] * n, [np.zeros(0, np.uint32)] * n

    def dtw_align_device(self, d, q, src, **kw):
        self.asked.append(("dtw_align_device", np.asarray(src).tolist(), kw))
        return None, "lengths", None, "maps", None, np.array([0, 20, 27, 27], np.uint64)

    def reconstruct_warped(self, smp, idx, out_off, maps, m_off, frames, lengths, want_pcm32, **kw):
        self.asked.append(("reconstruct_warped", np.asarray(idx).tolist(), maps, lengths, kw))
        return np.zeros(int(out_off[-1]))

    def reconstruct_wsola(self, smp, idx, out_off, maps, m_off, frames, lengths, search, want_pcm32, want_pos, **kw):
        self.asked.append(("reconstruct_wsola", np.asarray(idx).tolist(), search, kw))
        return np.zeros(int(out_off[-1]))


def _dict(e):
    d = SoundDictionary(engine=e)
    d.sounds = _sounds()
    rng = np.random.default_rng(0xA13)
    targets = [Sound(rng.standard_normal(n), 8000.0, rng.standard_normal((f, 5)).reshape(-1), None, ncoeffs=5)
               for f, n in ((20, 5000), (7, 1800), (4, 1000))]
    return d, targets


def test_an_empty_spot_is_a_pair_without_a_source_and_an_empty_window():
    e = _RecordingEngine()
    d, targets = _dict(e)
    spots = [Spot(1, 1, 5, 3.0), Spot(0, 2, 9, 4.0), Spot.none()]
    al = d.align(targets, spans=spots)
    name, src, kw = e.asked[0]
    assert (name, src) == ("dtw_align", [1, 0, NO]) and set(kw) == {"spans"}       # the default step passes no keyword on
    assert kw["spans"][0].tolist() == [1, 2, NO] and kw["spans"][1].tolist() == [5, 9, NO]
    assert [a.source_index for a in al] == [1, 0, NO] and [a.span_start for a in al] == [1, 2, 0]
    assert all(isinstance(a, Alignment) and len(a) == 0 for a in al)
    assert Alignment(0.0, np.zeros((0, 2)), np.zeros(0), 4).span_start == 0
    e.asked.clear()
    d.align(targets, spans=spots, step="paced")
    assert set(e.asked[0][2]) == {"spans", "step"} and e.asked[0][2]["step"] == "paced"
    e.asked.clear()
    out = d.warp(targets, spans=spots)
    assert out.size == 7800
    (a_name, a_src, a_kw), (w_name, w_idx, maps, lengths, w_kw) = e.asked
    assert (a_name, a_src, w_name) == ("dtw_align_device", [1, 0, NO], "reconstruct_warped")
    assert (maps, lengths) == ("maps", "lengths")                                  # the device outputs pass straight through
    assert w_idx == [1, 0, 0] and set(w_kw) == {"windows"}
    # sound 1 has 7 * 256 - 60 samples: frames 1 ... 5 end at 6 * 256; sound 0 is long enough; the empty spot: (0, 0)
    assert w_kw["windows"][0].tolist() == [256, 512, 0] and w_kw["windows"][1].tolist() == [5 * 256, 8 * 256, 0]
    assert w_kw["windows"][0].dtype == np.uint64 and w_kw["windows"][1].dtype == np.uint64
    e.asked.clear()
    d.warp(targets, spans=[Spot(1, 1, 6, 3.0)] + spots[1:], search=64)
    assert e.asked[1][0] == "reconstruct_wsola" and e.asked[1][2] == 64
    assert e.asked[1][3]["windows"][1].tolist() == [7 * 256 - 60 - 256, 8 * 256, 0]     # the recording ends inside the span


def test_context_changes_only_the_windows_lengths():
    e = _RecordingEngine()
    d, targets = _dict(e)
    spots = [Spot(1, 1, 5, 3.0), Spot(0, 2, 9, 4.0), Spot.none()]
    d.warp(targets, spans=spots)
    d.warp(targets, spans=spots, context=True)
    plain, wide = e.asked[:2], e.asked[2:]
    assert plain[0][:2] == wide[0][:2]
    for k in (0, 1):
        assert np.array_equal(plain[0][2]["spans"][k], wide[0][2]["spans"][k])
    assert plain[1][:4] == wide[1][:4]
    assert np.array_equal(plain[1][4]["windows"][0], wide[1][4]["windows"][0])
    assert wide[1][4]["windows"][1].tolist() == [7 * 256 - 60 - 256, 20 * 256 + 100 - 512, 0]      # to each recording's end


def test_reconstruct_spotted_is_three_calls_on_one_query_set():
    e = _RecordingEngine()
    made = []
    e.queries = lambda *a: made.append(1) or e._Q()
    d, targets = _dict(e)
    spots, out = d.reconstruct_spotted(targets)
    assert [c[0] for c in e.asked] == ["spot_queries", "dtw_align_device", "reconstruct_warped"] and len(made) == 1
    assert [bool(s) for s in spots] == [True, True, False] and (spots[0].source_index, spots[0].start_frame, spots[0].end_frame) == (1, 1, 5)
    assert out.size == 7800 and e.asked[1][1] == [1, 0, NO] and e.asked[2][1] == [1, 0, 0]
    e.asked.clear()
    spots, out = SoundSequence.new(targets).reconstruct_spotted_from_dictionary(d, step="paced", search=64)
    assert [c[0] for c in e.asked] == ["spot_queries", "dtw_align_device", "reconstruct_wsola"]
    assert e.asked[0][1] == {"step": "paced"} and e.asked[1][2]["step"] == "paced" and spots[0].cost_per_frame == 3.0 / 20
    with pytest.raises(ValueError, match="step must be"):
        d.reconstruct_spotted(targets, step="itakura")
    assert d.reconstruct_spotted([])[0] == []
