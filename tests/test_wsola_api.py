"""The WSOLA-reconstruction interface without a device: the header, the ctypes binding and the Rust declarations name the
new entry point, a null context is refused, the Python argument checks come before any device work, and search = 0 keeps
to the plain warp's entry point."""
import os
import re
import types

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import Engine, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat
from soundsym_amd.engine import DeviceFrames, _wsola_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ssym_reconstruct_wsola"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_and_rust_name_the_call(native_lib):
    header, rust = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs")
    assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % NAME, header)
    assert NAME in nat.ABI_SYMBOLS and NAME in soundsym_amd.ABI_SYMBOLS
    assert re.search(r"pub fn %s\s*\(" % NAME, rust)
    assert hasattr(native_lib, NAME) and len(getattr(native_lib, NAME).argtypes) == 14
    assert "search" in _read("include", "soundsym.hpp")
    assert "wsola.hip" in _read("soundsym_amd", "csrc", "Makefile")


def test_the_header_carries_the_definition():
    header = _read("include", "soundsym_amd.h")
    doc = header[header.index("WSOLA reconstruction"):header.index("ssym_reconstruct_wsola(ssym_ctx")]
    for phrase in ("pos[0] = map[0] * HOP", "pos[j-1] + HOP + n", "0 <= nom + d < sLen", "ascending n", "c / sqrt(e)",
                   "0 when e = 0", "smaller |d|", "negative d", "NaN score never wins", "at most 512", "out_pos",
                   "One synchronisation", "bit for bit"):
        assert phrase in doc, phrase
    kernel = _read("soundsym_amd", "csrc", "wsola.hip")
    assert "warp_synth(" in kernel                                 # the synthesis kernel's text is the shared header's
    kernel += _read("soundsym_amd", "csrc", "warp_common.hpp")
    for word in ("__dadd_rn", "__dmul_rn", "__ddiv_rn", "__dsqrt_rn", "wsola_search_kernel", "wsola_synth_kernel"):
        assert word in kernel
    assert "atomic" not in kernel


def test_a_null_context_is_refused_without_a_device(native_lib):
    one = np.zeros(2, dtype=np.uint64)
    assert native_lib.ssym_reconstruct_wsola(None, None, None, one.ctypes.data, 1, None, one.ctypes.data, None, None, 16,
                                             0, None, None, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_reconstruct_wsola(None, None, None, one.ctypes.data, 1, None, one.ctypes.data, None, None, 513,
                                             0, None, None, None) == nat.SSYM_E_INVALID


class _NoDevice:
    """An engine whose every attribute but the metric is a failure: what touches it has reached for the device."""
    metric = "dtw"

    def __getattr__(self, name):
        raise AssertionError("device work before the argument checks: " + name)


def test_python_argument_errors_come_before_any_device_work():
    for good in (0, 1, 512, np.int64(7), np.uint32(512)):
        assert _wsola_search(good) == int(good)
    for bad in (-1, 513, 1 << 40, 2.0, "4", None, True, np.float64(3)):
        with pytest.raises(ValueError):
            _wsola_search(bad)
    e = _NoDevice()
    idx, off = [0, 1], [0, 300, 900]
    maps, m_off, frames = np.arange(6, dtype=np.uint32), [0, 2, 6], [2, 4]
    for search in (-1, 513, 1.5):
        with pytest.raises(ValueError):
            Engine.reconstruct_wsola(e, None, idx, off, maps, m_off, frames, search=search)
    bad = [
        dict(out_offsets=[0, 300]),
        dict(out_offsets=[1, 300, 900]),
        dict(out_offsets=[0, 900, 300]),
        dict(map_offsets=[0, 2]),
        dict(map_offsets=[0, 6, 2]),
        dict(map_offsets=[0, 1, 6]),
        dict(map_frames=[2]),
        dict(maps=np.arange(5, dtype=np.uint32)),
        dict(maps=None),
        dict(pair_len=[1]),
        dict(pair_len=DeviceFrames(4096, 2, 1)),
        dict(maps=DeviceFrames(4096, 6, 1), pair_len=[1, 1]),
        dict(maps=DeviceFrames(4096, 5, 1)),
    ]
    for change in bad:
        args = dict(idx=idx, out_offsets=off, maps=maps, map_offsets=m_off, map_frames=frames, pair_len=None)
        args.update(change)
        with pytest.raises(ValueError):
            Engine.reconstruct_wsola(e, None, search=64, **args)
    # the dictionary and the sequence: the width is checked before a query is packed or a sound is matched
    d = SoundDictionary(engine=e)
    d.sounds.append(object())
    for search in (-1, 513, 0.5):
        with pytest.raises(ValueError):
            d.warp([object()], search=search)
        with pytest.raises(ValueError):
            SoundSequence.new([object()]).reconstruct_warped_from_dictionary(d, search=search)
        with pytest.raises(ValueError):
            SoundSequence.new([]).reconstruct_warped_from_dictionary(d, search=search)
    with pytest.raises(ValueError):
        d.warp([object()], want_pos=True)                     # positions without a search
    out, pcm, pos, m_off = d.warp([], want_pcm32=True, search=8, want_pos=True)
    assert out.size == 0 and pcm.dtype == np.int32 and pos.dtype == np.uint64 and m_off.tolist() == [0]


def test_a_refcos_engine_is_refused_in_python():
    refcos = types.SimpleNamespace(metric="refcos")
    with pytest.raises(nat.SsymError) as err:
        Engine.reconstruct_wsola(refcos, None, [0], [0, 10], None, [0, 0], [0], search=4)
    assert err.value.code == nat.SSYM_E_UNSUPPORTED
    d = SoundDictionary(engine=refcos)
    d.sounds.append(object())
    with pytest.raises(nat.SsymError) as err:
        d.warp([], search=4)
    assert err.value.code == nat.SSYM_E_UNSUPPORTED
    for cls, name in ((Engine, "reconstruct_wsola"), (SoundDictionary, "warp"),
                      (SoundSequence, "reconstruct_warped_from_dictionary")):
        assert hasattr(cls, name)


class _Recorder:
    """Stands in for an engine: records which reconstruction the dictionary asks for."""
    metric, np_dtype = "dtw", np.float64

    def __init__(self):
        self.calls = []

    def queries(self, flat, off, dim):
        return types.SimpleNamespace(close=lambda: None)

    def dictionary(self, flat, off, dim):
        return types.SimpleNamespace(close=lambda: None, n=1)

    def samples(self, smp, off):
        return types.SimpleNamespace(close=lambda: None)

    def dtw_align_device(self, d, q, indices):
        return None, "lengths", None, "maps", None, np.array([0, 3], dtype=np.uint64)

    def reconstruct_warped(self, *args):
        self.calls.append(("warped", args))
        return np.zeros(5)

    def reconstruct_wsola(self, *args):
        self.calls.append(("wsola", args))
        return np.zeros(5)


def test_search_zero_does_not_reach_the_new_entry_point():
    rng = np.random.default_rng(3)
    e = _Recorder()
    d = SoundDictionary(engine=e)
    d.sounds = [Sound(rng.uniform(-1, 1, size=900), 44100.0, rng.standard_normal(3 * 12))]
    target = Sound(rng.uniform(-1, 1, size=800), 44100.0, rng.standard_normal(3 * 12))
    d.warp([target], indices=[0])
    d.warp([target], indices=[0], search=0)
    assert [c[0] for c in e.calls] == ["warped", "warped"]
    d.warp([target], indices=[0], search=96)
    assert e.calls[-1][0] == "wsola" and e.calls[-1][1][7] == 96 and e.calls[-1][1][3] == "maps"
    # the sequence passes its width on (no indices: it matches first)
    e.match = lambda d_, q_: (np.zeros(1, dtype=np.uint32), np.zeros(1))
    SoundSequence.new([target]).reconstruct_warped_from_dictionary(d)
    SoundSequence.new([target]).reconstruct_warped_from_dictionary(d, search=5)
    assert [c[0] for c in e.calls[-2:]] == ["warped", "wsola"] and e.calls[-1][1][7] == 5
