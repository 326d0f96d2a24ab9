"""SoundSequence.distances / analyze_mfccs / cosine_sim_angular without a GPU: the paths that must not reach the
device, and the two new C entry points' argument checks through the library (which loads without a GPU)."""
import ctypes

import numpy as np
import pytest

import soundsym_amd._native as nat
from soundsym_amd import Sound, SoundSequence, analyze_mfccs, cosine_sim_angular


class _Untouchable:
    """An engine that fails the test on any use."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was used ({name})")


def test_distances_of_short_sequences_need_no_device():
    s = Sound(np.zeros(4096), 44100.0, np.zeros(12))
    for seq in (SoundSequence([]), SoundSequence([s]), SoundSequence.new([Sound(np.zeros(10), 8000.0, None)])):
        d = seq.distances(engine=object())
        assert isinstance(d, np.ndarray) and d.shape == (0,)


def test_distances_mixed_ncoeffs_raise_before_the_engine():
    a = Sound(np.zeros(4096), 44100.0, np.zeros(24), ncoeffs=12)
    b = Sound(np.zeros(4096), 44100.0, None, ncoeffs=13)
    with pytest.raises(ValueError):
        SoundSequence([a, b]).distances(engine=_Untouchable())
    with pytest.raises(ValueError):
        SoundSequence([a, a, Sound(np.zeros(4096), 44100.0, np.zeros(20), ncoeffs=20)]).distances(engine=_Untouchable())


def test_analyze_mfccs_without_frames_needs_no_device():
    assert analyze_mfccs([], 44100.0, engine=_Untouchable()) == []
    out = analyze_mfccs([np.zeros(0), np.zeros(1023), np.ones(17)], 44100.0, engine=_Untouchable())
    assert [o.size for o in out] == [0, 0, 0]
    # with padded framing, 255 samples still hold no frame
    assert [o.size for o in analyze_mfccs([np.zeros(255)], 44100.0, engine=_Untouchable(), pad_tail=True)] == [0]


def test_from_timestamps_without_frames_needs_no_device():
    s = Sound(np.arange(2000, dtype=np.float64), 1000.0, None)
    seq = SoundSequence.from_timestamps(s, [(0.0, 0.5, "a"), (0.5, 1.0, "b"), (1.0, 1.999, None)], engine=_Untouchable())
    assert [x.samples().size for x in seq.sounds()] == [501, 501, 1000]
    assert [x.name for x in seq.sounds()] == ["a", "b", None]
    assert all(x.has_mfccs() and x.num_frames() == 0 for x in seq.sounds())


def test_cosine_sim_angular_needs_equal_lengths():
    with pytest.raises(ValueError):
        cosine_sim_angular(np.zeros(12), np.zeros(13), engine=_Untouchable())
    with pytest.raises(ValueError):
        cosine_sim_angular(np.zeros(0), np.zeros(0), engine=_Untouchable())


def test_new_entry_points_reject_a_null_context(native_lib):
    x = np.ones(4096)
    off = np.array([0, 4096], dtype=np.uint64)
    fo = np.full(2, 7, dtype=np.uint64)
    out, mean = np.full(13 * 12, 7.0), np.full(12, 7.0)
    rc = native_lib.ssym_mfcc_batch(None, x.ctypes.data, off.ctypes.data, 1, 44100.0, 12, 100.0, 8000.0, 0,
                                    fo.ctypes.data, out.ctypes.data, mean.ctypes.data)
    assert rc == nat.SSYM_E_INVALID
    feats = np.ones(24)
    foff = np.array([0, 1, 2], dtype=np.uint64)
    sim, dist = np.full(1, 7.0), np.full(1, 7.0)
    rc = native_lib.ssym_sequence_distances(None, feats.ctypes.data, foff.ctypes.data, 2, 12, 0, mean.ctypes.data,
                                            sim.ctypes.data, dist.ctypes.data)
    assert rc == nat.SSYM_E_INVALID
    assert np.all(fo == 7) and np.all(out == 7.0) and np.all(mean == 7.0) and sim[0] == 7.0 and dist[0] == 7.0


def test_frame_counts_are_host_arithmetic(native_lib):
    t = ctypes.c_uint64(0)
    for n, pad, want in ((0, 0, 0), (1023, 0, 0), (1024, 0, 1), (1279, 0, 1), (1280, 0, 2), (255, 4, 0), (256, 4, 1),
                         (44100, 0, 169), (44100, 4, 172)):
        assert native_lib.ssym_mfcc_num_frames(n, pad, ctypes.byref(t)) == nat.SSYM_OK and t.value == want
