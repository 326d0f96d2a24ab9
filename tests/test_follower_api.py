"""Live envelope following without a GPU: what the library exports and declares, the definition's constants in the header
against the plan and the kernels, the one text of the chain, and the ValueErrors of Engine.follower / Follower /
mosaic_live(dynamics=) that come before any library call."""
import ctypes
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import Follower, SoundDictionary
from soundsym_amd import _native as nat
from soundsym_amd import engine as engine_mod
from soundsym_amd.api import HOP, LiveMosaic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ssym_follower_create", "ssym_follower_destroy", "ssym_follower_push", "ssym_follower_flush", "ssym_follower_samples",
           "ssym_follower_counts", "ssym_follower_reset"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_abi_lists_declares_and_exports_the_follower(native_lib):
    header = _read("include", "soundsym_amd.h")
    for name in SYMBOLS:
        assert name in nat.ABI_SYMBOLS and hasattr(native_lib, name)
        assert len(re.findall(r"SSYM_API int32_t %s\(" % name, header)) == 1, name
    assert "Follower" in soundsym_amd.__all__


def test_null_handles_are_refused_before_anything_is_written(native_lib):
    n = np.full(3, 9, dtype=np.uint64)
    f = np.full(4, -1.5)
    count = ctypes.c_uint64(77)
    p = lambda a: a.ctypes.data      # noqa: E731
    assert native_lib.ssym_follower_create(None, 1, 8.0, None) == nat.SSYM_E_INVALID
    assert native_lib.ssym_follower_push(None, None, p(f), p(n), p(f), p(n), 0, ctypes.byref(count)) == nat.SSYM_E_INVALID
    assert native_lib.ssym_follower_flush(None, None, 0, ctypes.byref(count)) == nat.SSYM_E_INVALID
    assert native_lib.ssym_follower_samples(None, None, p(n), p(f), None, p(n), p(f), 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_follower_counts(None, p(n), p(n), p(n)) == nat.SSYM_E_INVALID
    assert native_lib.ssym_follower_reset(None, None, 0) == nat.SSYM_E_INVALID
    assert native_lib.ssym_follower_destroy(None, None) == nat.SSYM_OK        # destroying nothing is fine
    assert (n == 9).all() and (f == -1.5).all() and count.value == 77


def test_the_definitions_constants_are_the_plans_and_the_kernels():
    plan, kernels, common = (_read("soundsym_amd", "csrc", x) for x in ("follower_plan.hpp", "follower.hip", "follow_common.hpp"))
    header = _read("include", "soundsym_amd.h")
    assert "constexpr uint64_t kFollowerRingMin = 2048;" in plan and "at least 2048" in header
    assert "constexpr uint64_t kFollowerRingBytes = 512ull << 20;" in plan and "within 512 MiB" in header
    assert "static_assert(kFollowerMaxLanes == 16384" in plan and "16384 lanes" in header
    assert "constexpr uint64_t kFollowerMaxLen = 1ull << 40;" in plan and "fewer than 2^40 samples per signal" in header
    # the plan and the kernels are tied together where both are visible
    assert "kFollowerHop == (uint64_t)kWarpHop && kFollowerBlock == (uint32_t)kFollowBlock && kFollowerMaxLen == kFollowMaxLen" in kernels
    # one text of the chain, the gain and the sample: both files call it, neither spells it out
    offline = _read("soundsym_amd", "csrc", "follow.hip")
    for text in (offline, kernels):
        assert '#include "follow_common.hpp"' in text
        assert len(re.findall(r"follow_chain\(s, sw\)", text)) == 1 and len(re.findall(r"follow_gain\(ex, acc, a\.maxGain\)", text)) == 1
        assert len(re.findall(r"follow_sample\(v\[q\], sG\[u \+ q\], sG\[u \+ q \+ 1\], f, fm\)", text)) == 1
        assert "__dsqrt_rn(" not in text and "__ddiv_rn(" not in text and "__dadd_rn(" not in text       # named, never called
    assert common.count("__dsqrt_rn(__ddiv_rn(ex, ey))") == 1
    # no atomics, no inline assembly, no cooperative launch in the follower's kernels
    assert not re.search(r"atomic\w*\s*\(|asm\s*(volatile)?\s*\(|hipLaunchCooperativeKernel|__builtin_amdgcn_s_sleep", kernels)


class _Lib:
    """Records the entry points a call makes; every call succeeds and writes nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return nat.SSYM_OK
        return call


def test_follower_calls_and_their_checks(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(engine_mod.nat, "lib", lambda: lib)
    e = soundsym_amd.Engine.__new__(soundsym_amd.Engine)
    e.ctx, e.device = None, 0
    for bad in (0.5, float("nan"), float("inf"), -1, "loud", None):
        with pytest.raises(ValueError, match="max_gain"):
            e.follower(1, bad)
    for bad in (0, -2, 1.5, True, 16385):
        with pytest.raises(ValueError, match="n_lanes"):
            e.follower(bad)
    assert lib.calls == []
    f = e.follower(2, 4)
    assert isinstance(f, Follower) and (f.n_lanes, f.max_gain, f.n_samples) == (2, 4.0, 0)
    assert e.follower(16384).n_lanes == 16384
    lib.calls.clear()
    y = np.arange(6.0)
    for call in (lambda: f.push(y, None, y, None),                       # two lanes: offsets are needed
                 lambda: f.push(y, [0, 6], y, [0, 3, 6]),                 # n_lanes + 1 of them
                 lambda: f.push(y, [1, 3, 6], y, [0, 3, 6]),              # starting at 0
                 lambda: f.push(y, [0, 4, 3], y, [0, 3, 6]),              # not decreasing
                 lambda: f.push(y, [0, 3, 7], y, [0, 3, 6]),              # within the array
                 lambda: f.push(y, [0, 3, 6], None, [0, 3, 6]),
                 lambda: f.push(y.astype(np.float32).reshape(2, 3)[:, :2], [0, 3, 6], y, [0, 3, 6]),
                 lambda: f.flush(2), lambda: f.flush(-1), lambda: f.reset(2)):
        with pytest.raises(ValueError):
            call()
    assert lib.calls == []
    assert f.push(y, [0, 2, 6], None, [0, 0, 0]) == 0 and f.push(None, [0, 0, 0], y[:1], [0, 1, 1]) == 0 and f.flush(1) == 0
    off, smp, pcm, g_off, g = f.samples(want_pcm32=True, want_gains=True)
    assert (off.shape, off.dtype, smp.shape, smp.dtype, pcm.shape, pcm.dtype) == ((3,), np.uint64, (0,), np.float64, (0,), np.int32)
    assert (g_off.shape, g_off.dtype, g.shape, g.dtype) == ((3,), np.uint64, (0,), np.float64)
    assert len(f.samples()) == 2 and len(f.samples(want_pcm32=True)) == 3 and len(f.samples(want_gains=True)) == 4
    ny, nx, rel = f.counts()
    assert ny.shape == nx.shape == rel.shape == (2,) and ny.dtype == np.uint64
    f.reset(1)
    f.close()
    f.close()
    assert [c for c in lib.calls if c[0] != "ssym_follower_samples"] == \
        [("ssym_follower_push", 8), ("ssym_follower_push", 8), ("ssym_follower_flush", 4), ("ssym_follower_counts", 4),
         ("ssym_follower_reset", 3)]                                       # (ctx is None: nothing to destroy)
    assert all(c == ("ssym_follower_samples", 8) for c in lib.calls if c[0] == "ssym_follower_samples")


class _FakeEngine:
    """Enough of an Engine for the checks that come before any library call; anything else fails loudly."""
    np_dtype = np.float64
    metric = "dtw"

    def __getattr__(self, name):
        raise AssertionError("device work reached: Engine.%s" % name)


def test_mosaic_live_checks_the_dynamics_before_any_library_call():
    from soundsym_amd import Sound
    rng = np.random.default_rng(0xA14)
    d = SoundDictionary(engine=_FakeEngine())
    d.sounds = [Sound(rng.standard_normal(20 * HOP), 8000.0, rng.standard_normal(20 * 5), "s", ncoeffs=5)]
    with pytest.raises(ValueError, match="audio=True"):
        d.mosaic_live(d.sounds, 1.0, None, dynamics="target")
    with pytest.raises(ValueError, match="audio=True"):
        d.mosaic_live(d.sounds, 1.0, None, audio=False, dynamics="target", max_gain=2.0)
    for kw in ({"dynamics": "source"}, {"dynamics": True}, {"dynamics": "target", "max_gain": 0.5},
               {"dynamics": "target", "max_gain": float("inf")}, {"dynamics": "target", "max_gain": float("nan")},
               {"dynamics": "target", "max_gain": "loud"}):
        with pytest.raises(ValueError, match="dynamics|max_gain"):
            d.mosaic_live(d.sounds, 1.0, None, audio=True, **kw)
    # good arguments get as far as the checks that were there before
    with pytest.raises(ValueError, match="share one stream"):
        d.mosaic_live(d.sounds, 1.0, None, audio=True, dynamics="target", max_gain=2.0)
    with pytest.raises(ValueError, match="share one stream"):
        d.mosaic_live(d.sounds, 1.0, None, audio=True, dynamics=None)


def test_live_mosaic_audio_feeds_the_follower_after_the_splice_and_flushes_ended_sounds():
    class _Sound:
        def __init__(self, n):
            self._s = np.arange(1.0, n + 1.0)

        def samples(self):
            return self._s

    class _Fl:
        n_lanes = 2

        def __init__(self):
            self.ny, self.nx, self.log, self.n_samples, self.last = [0, 0], [0, 0], [], 0, None

        def counts(self):
            return np.array(self.ny, dtype=np.uint64), np.array(self.nx, dtype=np.uint64), np.zeros(2, dtype=np.uint64)

        def push(self, y, off, x, r_off):
            self.log.append(("push", y.copy(), [int(v) for v in off], x.copy(), [int(v) for v in r_off]))
            for l in range(2):
                self.ny[l] += int(off[l + 1] - off[l])
                self.nx[l] += int(r_off[l + 1] - r_off[l])
            self.last = (np.array([0, 1, 1], dtype=np.uint64), np.array([-1.0]), np.array([-7], dtype=np.int32))
            self.n_samples = 1
            return 1

        def flush(self, lane):
            self.log.append(("flush", lane))
            self.last = (np.array([0, 0, 2] if lane else [0, 2, 2], dtype=np.uint64), np.array([-2.0, -3.0]), np.array([-8, -9], dtype=np.int32))
            self.n_samples = 2
            return 2

        def samples(self, want_pcm32=False):
            return self.last

        def close(self):
            self.log.append(("close",))

    class _Quiet:
        n_samples = 0
        n_lanes = 2

        def close(self):
            pass

    sounds = [_Sound(700), _Sound(300)]
    fl = _Fl()
    live = LiveMosaic(sounds, None, _Quiet(), 1.0, None, _Quiet(), "silence", fl)
    live._audio[0].append((np.full(256, 0.5), np.zeros(256, dtype=np.int32)))
    live._frames[0][0].append(3)
    out = live.audio(want_pcm32=True)
    kind, y, off, x, r_off = fl.log[0]
    assert kind == "push" and off == [0, 256, 256] and r_off == [0, 256, 256]
    assert np.array_equal(y, np.full(256, 0.5)) and np.array_equal(x, sounds[0].samples()[:256])      # the sound's own, up to the same count
    assert np.array_equal(out[0][0], [-1.0]) and np.array_equal(out[0][1], [-7]) and out[1][0].size == 0
    # nothing new and nothing ended: no call
    assert [a.size for a in live.audio()] == [0, 0] and len(fl.log) == 1
    # sound 1 ends with 300 samples the resynthesiser released at its flush; the reference stops at the sound's end
    live._audio[1].append((np.zeros(300), np.zeros(300, dtype=np.int32)))
    live._ended[1] = True
    out = live.audio()
    assert [c[0] for c in fl.log[1:]] == ["push", "flush"] and fl.log[2] == ("flush", 1)
    assert fl.log[1][2] == [0, 0, 300] and fl.log[1][4] == [0, 0, 300]
    assert np.array_equal(out[0], [-1.0]) and np.array_equal(out[1], [-2.0, -3.0])     # (the fake releases one sample of sound 0 per push)
    assert [a.size for a in live.audio()] == [0, 0] and len(fl.log) == 3                 # a lane is flushed once
    live.close()
    assert fl.log[-1] == ("close",)
