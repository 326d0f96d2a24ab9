"""The alignment interface without a device: the header, the ctypes binding and the Rust declarations name the new entry
points; the limits the header states are the kernel's constants; Alignment and the Python argument checks."""
import os
import re

import numpy as np
import pytest

import soundsym_amd
from soundsym_amd import Alignment, SoundDictionary
from soundsym_amd import _native as nat
from soundsym_amd.engine import _align_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ssym_dtw_align_sizes", "ssym_dtw_align"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_binding_and_rust_name_the_new_symbols(native_lib):
    header, rust = _read("include", "soundsym_amd.h"), _read("bindings", "rust", "src", "gpu.rs")
    for name in NEW:
        assert re.search(r"SSYM_API\s+int32_t\s+%s\s*\(" % name, header), name
        assert name in nat.ABI_SYMBOLS and name in soundsym_amd.ABI_SYMBOLS
        assert re.search(r"pub fn %s\s*\(" % name, rust), name
        assert hasattr(native_lib, name)
    assert native_lib.ssym_abi_version() == 3 and "#define SSYM_ABI_VERSION 3" in header
    assert "align(" in _read("include", "soundsym.hpp")
    assert len(native_lib.ssym_dtw_align.argtypes) == 14 and len(native_lib.ssym_dtw_align_sizes.argtypes) == 8


def test_header_states_the_kernels_limits():
    src, header = _read("soundsym_amd", "csrc", "dtw_align.hip"), _read("include", "soundsym_amd.h")
    frames = int(re.search(r"kAlignMaxFrames\s*=\s*(\d+);", src).group(1))
    dim = int(re.search(r"kAlignMaxDim\s*=\s*(\d+);", src).group(1))
    assert (frames, dim) == (4096, 64)
    doc = header[header.index("DTW alignment"):header.index("ssym_dtw_align_sizes(const")]
    assert "at most %d frames" % frames in doc and "dim <= %d" % dim in doc
    assert "dtw_align.hip" in _read("soundsym_amd", "csrc", "Makefile")


def test_sizes_reject_null_handles_without_a_device(native_lib):
    # the host path needs resident sets, which only a device makes; what it can answer without one: NULL handles
    idx = np.zeros(1, dtype=np.uint32)
    off = np.zeros(2, dtype=np.uint64)
    rc = native_lib.ssym_dtw_align_sizes(None, None, idx.ctypes.data, None, 1, 0, off.ctypes.data, off.ctypes.data)
    assert rc == nat.SSYM_E_INVALID
    assert native_lib.ssym_dtw_align(None, None, None, idx.ctypes.data, None, 1, 0, None, None, None, None, None, None,
                                     0) == nat.SSYM_E_INVALID


def test_sizes_arithmetic_restated():
    # slot p holds Fa + Fb - 1 cells and Fb map entries, nothing for an empty segment or SSYM_NO_MATCH: the longest
    # path takes every row step and every column step once, the shortest max(Fa, Fb) cells
    import dtw_path_ref as ref
    rng = np.random.default_rng(3)
    for _ in range(30):
        fa, fb = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        _, path, fmap = ref.align(rng.integers(-1, 2, size=(fa, 1)), rng.integers(-1, 2, size=(fb, 1)), squared=True)
        assert max(fa, fb) <= path.shape[0] <= fa + fb - 1 and fmap.size == fb
    _, path, _ = ref.align(np.array([[0.0], [5.0], [5.0]]), np.array([[0.0], [0.0], [5.0]]), squared=True)
    assert path.shape[0] == 4                       # (0,0) (0,1) (1,2) (2,2): between the bounds
    _, path, _ = ref.align(np.array([[0.0], [1.0]]), np.array([[1.0], [0.0]]), squared=True)
    assert path.tolist() == [[0, 0], [1, 1]]


def test_alignment_value_class():
    a = Alignment(2.5, [[0, 0], [1, 1], [1, 2], [2, 3]], [0, 1, 1, 2], 7)
    assert a.cost == 2.5 and a.source_index == 7 and len(a) == 4
    assert a.path.dtype == np.uint32 and a.path.shape == (4, 2) and a.frame_map.dtype == np.uint32
    assert a.diagonal_share() == pytest.approx(2.0 / 3.0)
    assert "source_index=7" in repr(a)
    empty = Alignment(float("inf"), np.zeros((0, 2)), np.zeros(0), 0)
    assert len(empty) == 0 and empty.diagonal_share() == 0.0
    with pytest.raises(ValueError):
        Alignment(0.0, [0, 1, 2], [0], 0)
    with pytest.raises(ValueError):
        Alignment(0.0, [[0, 0]], [[0]], 0)


def test_python_argument_checks_need_no_device():
    src, tgt = _align_indices([3, 1, 2], None)
    assert src.dtype == np.uint32 and src.tolist() == [3, 1, 2] and tgt is None
    src, tgt = _align_indices(np.array([[1, 2]]), [0, 1])
    assert src.shape == (2,) and tgt.dtype == np.uint32
    with pytest.raises(ValueError):
        _align_indices([1, 2, 3], [0, 1])
    with pytest.raises(soundsym_amd.EmptyDictionaryError):
        SoundDictionary(engine=object()).align([])
    for name in ("Alignment",):
        assert name in soundsym_amd.__all__
    assert hasattr(soundsym_amd.Engine, "dtw_align") and hasattr(soundsym_amd.SoundSequence, "align_to_dictionary")
