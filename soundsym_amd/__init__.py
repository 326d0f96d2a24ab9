"""soundsym_amd -- MI355X-native segment-distance matching (the soundsym matcher hot path).

The compute lives in ``libsoundsym_amd.so`` (hand-written HIP for gfx950 behind the C ABI of
``include/soundsym_amd.h``).  This package is the host side: the ctypes binding, an array-level
engine, and a mirror of the reference's Sound / SoundDictionary / SoundSequence interface.
"""
from ._native import (  # noqa: F401
    ABI_SYMBOLS,
    EmptyDictionaryError,
    LIB_PATH,
    SsymError,
    build,
)
from .engine import Coverer, DeviceFrames, Engine, Follower, Gmm, Mosaicker, Resynth, Spotter, Stream, pack_segments, stream_plan  # noqa: F401
from .api import (  # noqa: F401
    Alignment,
    BIN,
    Cover,
    Gap,
    HOP,
    LiveCover,
    LiveMosaic,
    Mosaic,
    MosaicPiece,
    NCLUSTERS,
    NCOEFFS,
    Partitioner,
    Piece,
    Sound,
    SoundDictionary,
    SoundSequence,
    Spot,
    Watch,
    analyze_mfccs,
    analyze_sounds,
    cosine_sim_angular,
    discretize,
    discretize_with_model,
    follow_envelope,
    length_fit,
    push_sounds,
    train_model,
    watch,
)

__all__ = [
    "ABI_SYMBOLS", "Alignment", "BIN", "Cover", "Coverer", "DeviceFrames", "EmptyDictionaryError", "Engine", "Gap", "Gmm", "HOP", "LIB_PATH", "LiveCover", "LiveMosaic", "Mosaic", "MosaicPiece", "Mosaicker", "NCLUSTERS", "NCOEFFS",
    "Partitioner", "Piece", "Resynth", "Sound", "SoundDictionary", "SoundSequence", "Spot", "SsymError", "analyze_mfccs", "analyze_sounds", "build",
    "cosine_sim_angular", "discretize",
    "discretize_with_model", "follow_envelope", "Follower", "length_fit", "pack_segments", "push_sounds", "Spotter", "Stream", "stream_plan", "train_model", "Watch", "watch",
]
