"""The envelope-following interface without a device: the header, the ctypes binding, the Rust declaration and the C++ mirror
name the call; the header carries the definition; a null context is refused; the Python layer's ValueErrors come before
any device work; dynamics=None makes no call into follow_envelope and dynamics="target" makes exactly one, against the
targets' own samples."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import Engine, Sound, SoundDictionary, SoundSequence, follow_envelope
from soundsym_amd import _native as nat
from soundsym_amd.engine import DeviceFrames, follow_boundaries, follow_dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ssym_follow_envelope"
METHODS = ((SoundDictionary, "warp"), (SoundDictionary, "reconstruct_spotted"), (SoundDictionary, "reconstruct_covered"),
           (SoundDictionary, "reconstruct_mosaic"), (SoundSequence, "reconstruct_from_dictionary"),
           (SoundSequence, "reconstruct_warped_from_dictionary"), (SoundSequence, "reconstruct_spotted_from_dictionary"))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_rust_and_mirror_name_the_call(native_lib):
    header, rust = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs")
    decl = re.search(r"SSYM_API\s+int32_t\s+%s\s*\(([^;]*)\);" % NAME, header)
    assert decl and decl.group(1).count(",") + 1 == 11
    assert NAME in nat.ABI_SYMBOLS and NAME in soundsym_amd.ABI_SYMBOLS
    assert re.search(r"pub fn %s\s*\(" % NAME, rust)
    assert hasattr(native_lib, NAME) and len(getattr(native_lib, NAME).argtypes) == 11
    assert "#define SSYM_FOLLOW_SAMPLES_DEVICE 64u" in header and "#define SSYM_FOLLOW_REF_DEVICE 128u" in header
    assert (nat.FOLLOW_SAMPLES_DEVICE, nat.FOLLOW_REF_DEVICE) == (64, 128)
    values = [int(v.rstrip("u"), 0) for v in re.findall(r"#define SSYM_\w+_DEVICE (\w+)", header)] + [nat.OUT_DEVICE]
    assert len(values) == len(set(values)) == 4                    # no other call's device flag has these values
    mirror = _read("include", "soundsym.hpp")
    assert "follow_envelope(" in mirror and "dynamics" in mirror
    assert "follow.hip" in _read("soundsym_amd", "csrc", "Makefile")
    assert "follow_envelope" in soundsym_amd.__all__


def test_the_header_carries_the_definition():
    header = _read("include", "soundsym_amd.h")
    doc = header[header.index("Envelope following (DESIGN.md"):header.index("ssym_follow_envelope(ssym_ctx")]
    for phrase in ("x[k] reads +0.0 for k >= nx", "x[k] for k >= n is never read", "J = ceil(n / HOP)", "B = J + 1 boundaries",
                   "k = (b-2)*HOP + m", "three roundings, no contraction", "g(b) = sqrt(E_x(b) / E_y(b))", "g(b) = 1.0",
                   "g(b) = max_gain", "f = (k - j*HOP) / 256.0", "out[k] = y[k]*(a + c)", "two hops of look-ahead",
                   "SSYM_FOLLOW_SAMPLES_DEVICE", "SSYM_FOLLOW_REF_DEVICE", "SSYM_OUT_DEVICE", "One synchronisation",
                   "refcos included", "ssym_match_begin", "SSYM_E_UNSUPPORTED", "before any device work"):
        assert phrase in doc, phrase
    design = _read("DESIGN.md")
    for phrase in ("Envelope following", "5.28", "follow_gain_kernel", "follow_apply_kernel"):
        assert phrase in design, phrase
    kernel = _read("soundsym_amd", "csrc", "follow.hip")
    for word in ("__dadd_rn", "__dmul_rn", "__ddiv_rn", "__dsqrt_rn", "follow_gain_kernel", "follow_apply_kernel", "warp_pcm32"):
        assert word in kernel
    assert "atomic" not in kernel and "asm" not in kernel


def test_a_null_context_is_refused_without_a_device(native_lib):
    off = np.array([0, 10], dtype=np.uint64)
    y = np.zeros(10)
    assert native_lib.ssym_follow_envelope(None, y.ctypes.data, off.ctypes.data, 1, y.ctypes.data, off.ctypes.data, 8.0, 0,
                                           None, None, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_follow_envelope(None, None, None, 0, None, None, 8.0, 0, None, None, None) == nat.SSYM_E_INVALID


class _NoDevice:
    """An engine whose every attribute but the metric is a failure: what touches it has reached for the device."""
    metric = "dtw"

    def __getattr__(self, name):
        raise AssertionError("device work before the argument checks: " + name)


BAD_GAINS = (float("nan"), 0.0, 0.999, -8.0, float("inf"), "loud", None)


def test_the_checks_of_the_keywords():
    assert follow_dynamics(None, 8.0) is None and follow_dynamics("target", 8) == 8.0 and follow_dynamics("target", 1) == 1.0
    assert follow_dynamics("target", np.float64(2.0 ** 30)) == 2.0 ** 30
    for bad in ("source", "Target", "", 1, True, 0.5, ("target",)):
        with pytest.raises(ValueError):
            follow_dynamics(bad, 8.0)
    for bad in BAD_GAINS:
        with pytest.raises(ValueError):
            follow_dynamics("target", bad)
        with pytest.raises(ValueError):
            follow_dynamics(None, bad)                              # a bad max_gain is refused whether it is used or not
    assert follow_boundaries([0, 0, 1, 258, 258, 514]).tolist() == [0, 0, 2, 5, 5, 7]


def test_engine_argument_errors_come_before_any_device_work():
    e = _NoDevice()
    y, x = np.zeros(900), np.zeros(700)
    for bad in BAD_GAINS:
        with pytest.raises(ValueError):
            Engine.follow_envelope(e, y, [0, 300, 900], x, [0, 300, 700], bad)
    bad = [
        dict(out_offsets=[0, 300]),                                 # n + 1 of each
        dict(ref_offsets=[0, 300, 600, 700]),
        dict(out_offsets=[]),
        dict(out_offsets=[1, 300, 900]),
        dict(ref_offsets=[2, 300, 700]),
        dict(out_offsets=[0, 900, 300]),
        dict(ref_offsets=[0, 700, 300]),
        dict(samples=np.zeros(899)),                                # fewer values than the offsets ask for
        dict(ref=np.zeros(699)),
        dict(ref=None),
        dict(samples=DeviceFrames(4096, 899, 1)),
        dict(ref=DeviceFrames(4096, 10, 1)),
    ]
    for change in bad:
        args = dict(samples=y, out_offsets=[0, 300, 900], ref=x, ref_offsets=[0, 300, 700])
        args.update(change)
        with pytest.raises(ValueError):
            Engine.follow_envelope(e, **args)


def test_every_method_has_the_keywords_and_checks_them_first():
    for cls, name in METHODS:
        params = inspect.signature(getattr(cls, name)).parameters
        assert params["dynamics"].default is None and params["max_gain"].default == 8.0, name
    assert inspect.signature(Engine.follow_envelope).parameters["max_gain"].default == 8.0
    assert list(inspect.signature(Engine.follow_envelope).parameters)[1:] == [
        "samples", "out_offsets", "ref", "ref_offsets", "max_gain", "want_pcm32", "want_gains", "on_device"]
    assert list(inspect.signature(follow_envelope).parameters) == ["sound", "reference", "max_gain", "engine"]
    e = _NoDevice()
    d = SoundDictionary(engine=e)
    d.sounds.append(object())
    sound = Sound(np.zeros(600), 44100.0, np.zeros(24))
    calls = [lambda **k: d.warp([object()], **k), lambda **k: d.reconstruct_spotted([object()], **k),
             lambda **k: d.reconstruct_covered(sound, **k), lambda **k: d.reconstruct_mosaic(sound, **k),
             lambda **k: SoundSequence.new([sound]).reconstruct_from_dictionary(d, **k),
             lambda **k: SoundSequence.new([sound]).reconstruct_warped_from_dictionary(d, **k),
             lambda **k: SoundSequence.new([sound]).reconstruct_spotted_from_dictionary(d, **k),
             lambda **k: SoundSequence.new([]).reconstruct_from_dictionary(d, **k),
             lambda **k: d.warp([], **k)]
    assert len(calls) == len(METHODS) + 2
    for call in calls:
        for kw in (dict(dynamics="source"), dict(dynamics=True), dict(dynamics="target", max_gain=0.5),
                   dict(dynamics="target", max_gain=float("inf")), dict(max_gain=float("nan"))):
            with pytest.raises(ValueError):
                call(**kw)
    for bad in BAD_GAINS:
        with pytest.raises(ValueError):
            follow_envelope(sound, sound, bad, engine=e)
    with pytest.raises(ValueError):
        follow_envelope(sound, np.zeros(600), engine=e)


class _Recorder:
    """Stands in for an engine: answers the reconstructing calls with marked arrays and records every follow_envelope."""
    metric, np_dtype = "dtw", np.float64

    def __init__(self):
        self.follows, self.calls = [], []

    def queries(self, flat, off, dim):
        return types.SimpleNamespace(close=lambda: None)

    def dictionary(self, flat, off, dim):
        return types.SimpleNamespace(close=lambda: None, n=1)

    def samples(self, smp, off):
        return types.SimpleNamespace(close=lambda: None)

    def match(self, d, q, **kw):
        return np.zeros(1, dtype=np.uint32), np.zeros(1)

    def match_batch(self, d, flat, off, distances=None):
        return np.zeros(len(off) - 1, dtype=np.uint32), np.zeros(len(off) - 1)

    def dtw_align_device(self, d, q, indices, **kw):
        return None, "lengths", None, "maps", None, np.array([0, 3], dtype=np.uint64)

    def _made(self, name, out_off, want_pcm32):
        self.calls.append(name)
        total = int(np.asarray(out_off)[-1])
        out = np.full(total, 0.25)
        return (out, np.full(total, 7, dtype=np.int32)) if want_pcm32 else out

    def reconstruct(self, smp, idx, out_off, want_pcm32=False):
        return self._made("reconstruct", out_off, want_pcm32)

    def reconstruct_warped(self, smp, idx, out_off, maps, m_off, frames, lengths, want_pcm32=False, **kw):
        return self._made("warped", out_off, want_pcm32)

    def reconstruct_wsola(self, smp, idx, out_off, maps, m_off, frames, lengths, search, want_pcm32=False, want_pos=False, **kw):
        res = self._made("wsola", out_off, want_pcm32)
        res = res if isinstance(res, tuple) else (res,)
        return res + (("pos",) if want_pos else ())

    def follow_envelope(self, samples, out_offsets, ref, ref_offsets, max_gain=8.0, want_pcm32=False, want_gains=False,
                        on_device=False):
        self.follows.append((np.array(samples), np.array(out_offsets), np.array(ref), np.array(ref_offsets), max_gain, want_pcm32))
        out = np.full(np.asarray(samples).size, 0.5)
        return (out, np.full(out.size, 9, dtype=np.int32)) if want_pcm32 else out


def _pair(rng):
    e = _Recorder()
    d = SoundDictionary(engine=e)
    d.sounds = [Sound(rng.uniform(-1, 1, size=900), 44100.0, rng.standard_normal(3 * 12))]
    targets = [Sound(rng.uniform(-1, 1, size=800), 44100.0, rng.standard_normal(3 * 12)),
               Sound(rng.uniform(-1, 1, size=300), 44100.0, rng.standard_normal(1 * 12))]
    return e, d, targets


def test_dynamics_none_makes_no_call_into_follow_envelope():
    e, d, targets = _pair(np.random.default_rng(5))
    e.dtw_align_device = lambda d_, q_, i_, **kw: (None, "lengths", None, "maps", None, np.array([0, 3, 4], dtype=np.uint64))
    e.match = lambda d_, q_, **kw: (np.zeros(2, dtype=np.uint32), np.zeros(2))
    seq = SoundSequence.new(targets)
    plain = [d.warp(targets, indices=[0, 0]), d.warp(targets, indices=[0, 0], dynamics=None),
             d.warp(targets, indices=[0, 0], search=16, want_pcm32=True, dynamics=None, max_gain=2.0),
             seq.reconstruct_from_dictionary(d), seq.reconstruct_from_dictionary(d, dynamics=None),
             seq.reconstruct_warped_from_dictionary(d), seq.reconstruct_warped_from_dictionary(d, dynamics=None, max_gain=3.0)]
    assert e.follows == [] and e.calls == ["warped", "warped", "wsola", "reconstruct", "reconstruct", "warped", "warped"]
    assert all(np.all((p[0] if isinstance(p, tuple) else p) == 0.25) for p in plain)


def test_dynamics_target_makes_one_call_against_the_targets_samples():
    e, d, targets = _pair(np.random.default_rng(6))
    e.dtw_align_device = lambda d_, q_, i_, **kw: (None, "lengths", None, "maps", None, np.array([0, 3, 4], dtype=np.uint64))
    e.match = lambda d_, q_, **kw: (np.zeros(2, dtype=np.uint32), np.zeros(2))
    ref = np.concatenate([t.samples() for t in targets])
    seq = SoundSequence.new(targets)

    def one_follow(res, gain, pcm):
        assert len(e.follows) == 1
        samples, off, x, r_off, max_gain, want_pcm32 = e.follows.pop()
        assert np.all(samples == 0.25) and samples.size == 1100 and off.tolist() == r_off.tolist() == [0, 800, 1100]
        assert np.array_equal(x, ref) and max_gain == gain and want_pcm32 == pcm
        out = res[0] if isinstance(res, tuple) else res
        assert np.all(out == 0.5) and (not pcm or np.all(res[1] == 9))

    one_follow(d.warp(targets, indices=[0, 0], dynamics="target"), 8.0, False)
    one_follow(d.warp(targets, indices=[0, 0], want_pcm32=True, dynamics="target", max_gain=3), 3.0, True)
    res = d.warp(targets, indices=[0, 0], search=16, want_pcm32=True, want_pos=True, dynamics="target", max_gain=2.0)
    one_follow(res, 2.0, True)
    assert res[2] == "pos" and res[3].tolist() == [0, 3, 4]          # what else the call returns stays
    one_follow(seq.reconstruct_from_dictionary(d, dynamics="target"), 8.0, False)
    one_follow(seq.reconstruct_from_dictionary(d, True, dynamics="target", max_gain=1.0), 1.0, True)
    one_follow(seq.reconstruct_warped_from_dictionary(d, dynamics="target", max_gain=16.0), 16.0, False)
    one_follow(seq.reconstruct_warped_from_dictionary(d, search=8, dynamics="target"), 8.0, False)
    assert e.calls == ["warped", "warped", "wsola", "reconstruct", "reconstruct", "warped", "wsola"]


def test_the_convenience_function_follows_one_sound():
    e = _Recorder()
    rng = np.random.default_rng(7)
    sound = Sound(rng.uniform(-1, 1, size=700), 22050.0, rng.standard_normal(12), "reconstruction")
    reference = Sound(rng.uniform(-1, 1, size=900), 22050.0, rng.standard_normal(12), "target")
    got = follow_envelope(sound, reference, 4.0, engine=e)
    samples, off, x, r_off, max_gain, want_pcm32 = e.follows.pop()
    assert off.tolist() == [0, 700] and r_off.tolist() == [0, 900] and max_gain == 4.0 and not want_pcm32
    assert np.array_equal(samples, sound.samples()) and np.array_equal(x, reference.samples())
    assert isinstance(got, Sound) and np.all(got.samples() == 0.5) and got.samples().size == 700
    assert got.sample_rate() == 22050.0 and got.name == "reconstruction"
