"""Host-side mirror of the reference's matching interface: Sound / SoundDictionary / SoundSequence.

Same names, argument meaning and error behaviour as the reference for the hot path
(upstream src/sound.rs), so callers and tests read like the reference's own:

    Sound.from_samples / from_path / write_file             src/sound.rs:92, 114, 129
    SoundDictionary.new / from_path / from_segments / add_segments   src/sound.rs:296, 304, 323, 330
    SoundDictionary.match_sound / at_distance               src/sound.rs:346, 351
    SoundSequence.new / from_timestamps / morph_to / clone_from_dictionary   src/sound.rs:392, 419, 440, 451
    SoundSequence.from_distances / to_sound                 src/sound.rs:405, 475
    discretize / train_model / discretize_with_model        src/lib.rs:32-60
    Partitioner (new / from_path / depth / threshold / train / partition / partition_other)   src/lib.rs:67-151
    Sound.pitch_confidence / preload_pitch_confidence, analyze_sounds       src/sound.rs:170-179, 244-269
    SoundSequence.distances, cosine_sim_angular, analyze_mfccs (batched)    src/sound.rs:392-398, 436, 59-69, 215-242
    Sound.push_samples / mfcc_arrays, push_sounds (one push for many sounds) src/sound.rs:145-164, 196-203

Every comparison runs on the GPU through the C ABI (`engine.Engine`); this module only keeps the
containers, does the length fit of src/sound.rs:456-465 on the matched samples, and translates
errors.  A Sound is built from samples plus ready-made features (the `Some(mfccs)` form of
Sound::from_samples, src/sound.rs:92-94) or analysed on the GPU (`None`: `ssym_mfcc`, a
self-consistent MFCC -- the reference's arithmetic is in un-vendored crates, parity unpinned).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from ._native import COVER_GAP, NO_MATCH, SSYM_E_UNSUPPORTED, EmptyDictionaryError, SsymError
from .engine import FOLLOW_MAX_GAIN, Engine, _cover_gap_cost, _cover_penalty, _wsola_search, follow_dynamics, pack_segments, pitch_lags

NCOEFFS = 12   # src/lib.rs:22
NCLUSTERS = 26 # src/lib.rs:23
GMM_EPS = 0.1  # CovOption::Regularized(0.1), src/lib.rs:34, 45
HOP = 256      # src/lib.rs:24
BIN = 1024     # src/lib.rs:25
PITCH_RATE = 44100.0       # analyze_pitch_confidence passes this literal, whatever the sound's rate (src/sound.rs:265)
PITCH_F_MIN, PITCH_F_MAX = 100.0, 500.0
PITCH_VOICING = 0.2

_default_engine: Optional[Engine] = None


def default_engine() -> Engine:
    """refcos / f64 on GPU 0: the reference's own metric and dtype."""
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(metric="refcos", dtype="f64", device=0)
    return _default_engine


def frame_features(samples, sample_rate: float, ncoeffs: int = NCOEFFS, engine: Optional[Engine] = None,
                   pad_tail: bool = True) -> np.ndarray:
    """analyze_mfccs (src/sound.rs:215-242) for a whole sound on the GPU (`ssym_mfcc`; this package's own MFCC
    definition -- the reference's lives in un-vendored crates, PARITY UNPINNED): [n_frames * ncoeffs] f64,
    frame-major.  pad_tail=True gives len(samples) // 256 frames (the tail windows read zeros past the end), which is
    what the segment arithmetic of SoundDictionary::add_segments (`seg / HOP * NCOEFFS` values per segment,
    src/sound.rs:335) expects of a parent sound; pad_tail=False keeps full windows only."""
    e = engine or default_engine()
    return e.mfcc(samples, sample_rate, ncoeffs, pad_tail=pad_tail).reshape(-1)


def analyze_mfccs(sample_arrays, sample_rate: float, ncoeffs: int = NCOEFFS, engine: Optional[Engine] = None,
                  pad_tail: bool = False) -> List[np.ndarray]:
    """analyze_mfccs (src/sound.rs:215-242) for many sounds of one sample rate in ONE device call (ssym_mfcc_batch):
    a list of flat frame-major f64 arrays, array i bit for bit `Sound.from_samples(sample_arrays[i], rate,
    None).mfccs()`.  The frame counts are host arithmetic; when no sound holds a frame, no device call is made."""
    parts = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in sample_arrays]
    if not parts:
        return []
    frames = [Engine.mfcc_num_frames(p.size, pad_tail) for p in parts]
    if not any(frames):
        return [np.zeros(0) for _ in parts]
    offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    e = engine or default_engine()
    feats, fo = e.mfcc_batch(np.concatenate(parts), offsets, sample_rate, ncoeffs, pad_tail=pad_tail)
    flat = feats.reshape(-1)
    return [flat[int(fo[i]) * ncoeffs:int(fo[i + 1]) * ncoeffs].copy() for i in range(len(parts))]


def cosine_sim_angular(me, you, engine: Optional[Engine] = None) -> float:
    """cosine_sim_angular (src/sound.rs:59-69) of two equally long vectors on the GPU: the reference's cosine_sim
    (squared norms, rulinalg's dot), its clamp (a similarity below -1 also maps to 1), acos * FRAC_1_PI.  One
    ssym_sequence_distances call on two one-frame sounds (a one-frame mean is the frame itself)."""
    a = np.ascontiguousarray(me, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(you, dtype=np.float64).reshape(-1)
    if a.size != b.size or a.size == 0:
        raise ValueError("cosine_sim_angular: two non-empty vectors of the same length")
    e = engine or default_engine()
    dist = e.sequence_distances(np.concatenate([a, b]), np.array([0, 1, 2], dtype=np.uint64), a.size)
    return float(dist[0])


def _round_half_away(x: float) -> int:
    """f64::round (src/sound.rs:422-423): half away from zero -- Python's round() is half to even."""
    import math
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def _round_as_usize(x: float) -> int:
    """`x.round() as usize` (src/sound.rs:422-423): f64::round, then Rust's SATURATING float-to-integer cast -- a
    negative value or NaN becomes 0, +inf (and anything beyond) usize::MAX."""
    import math
    if x != x or x <= 0:
        return 0
    if math.isinf(x) or x >= 2.0 ** 64:
        return 2 ** 64 - 1
    return _round_half_away(x)


class _SoundList(list):
    """`pub sounds: Vec<Arc<Sound>>` as a list that counts its own mutations: the dictionary's GPU copies are rebuilt
    when `version` has moved, which costs O(1) per query instead of an identity scan of the whole list."""

    def __init__(self, *a):
        super().__init__(*a)
        self.version = 0


def _bumping(name):
    base = getattr(list, name)

    def method(self, *a, **k):
        self.version += 1
        return base(self, *a, **k)
    method.__name__ = name
    return method


for _m in ("append", "extend", "insert", "pop", "remove", "clear", "reverse", "sort", "__setitem__", "__delitem__",
           "__iadd__", "__imul__"):
    setattr(_SoundList, _m, _bumping(_m))


class Sound:
    """Samples + flat frame-major features of one sound (src/sound.rs:73-82)."""

    def __init__(self, samples, sample_rate: float, mfccs, name: Optional[str] = None,
                 ncoeffs: int = NCOEFFS):
        self.name = name
        self._samples = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        self._sample_rate = float(sample_rate)
        self.ncoeffs = int(ncoeffs)
        self._mfccs = None
        self._pitch_confidence = None
        self._stream = None                   # (Stream, lane) once push_samples / push_sounds has made it resident
        self._blocks = [None, None]           # ... and the growing host stores of its samples and features
        if mfccs is not None:
            m = np.ascontiguousarray(mfccs, dtype=np.float64).reshape(-1)
            if m.size % self.ncoeffs:
                raise ValueError("mfccs must hold whole frames of `ncoeffs` values")
            self._mfccs = m

    @staticmethod
    def from_samples(samples, sample_rate: float, mfccs=None, name: Optional[str] = None,
                     ncoeffs: int = NCOEFFS, engine: Optional[Engine] = None) -> "Sound":
        """Sound::from_samples (src/sound.rs:92-107).  mfccs=None runs the MFCC analysis as the
        reference does (analyze_mfccs, :215-242) -- here on the GPU (`ssym_mfcc`; its arithmetic is
        this package's own definition, parity unpinned)."""
        if mfccs is None:
            e = engine or default_engine()
            mfccs = e.mfcc(samples, sample_rate, ncoeffs).reshape(-1)
        return Sound(samples, sample_rate, mfccs, name, ncoeffs)

    @staticmethod
    def from_path(path, engine: Optional[Engine] = None) -> "Sound":
        """Sound::from_path (src/sound.rs:114-127): read a WAV (integer PCM scaled by
        i32::MAX >> (32 - bits), :116-119), name = file stem, features analysed (mfccs = None)."""
        import os
        from . import io as sio
        samples, rate = sio.read_wav(str(path))
        stem = os.path.splitext(os.path.basename(str(path)))[0]
        return Sound.from_samples(samples, float(rate), None, stem, engine=engine)

    def write_file(self, path) -> None:
        """Sound::write_file (src/sound.rs:129-143): mono 32-bit integer WAV,
        sample -> (i32::MAX as f64 * sample) as i32."""
        from . import io as sio
        sio.write_wav32(str(path), self._samples, int(self._sample_rate))

    def max_power(self) -> float:             # src/sound.rs:197, analyze_max_power :244-256 (host side)
        from . import io as sio
        return sio.max_power(self._samples)

    def pitch_confidence(self, engine: Optional[Engine] = None) -> float:
        """src/sound.rs:170-175: the preloaded value, else analyze_pitch_confidence (:258-269) now, on the GPU
        (ssym_sound_descriptors; its pitch arithmetic is this package's own definition, DESIGN.md 5.9, parity
        unpinned), with the reference's literal arguments: rate 44100 (whatever this sound's rate), 100-500 Hz,
        voicing threshold 0.2.  Not cached, as in the reference."""
        if self._pitch_confidence is not None:
            return self._pitch_confidence
        return float(analyze_sounds([self], engine)[1][0])

    def preload_pitch_confidence(self, engine: Optional[Engine] = None) -> None:
        """src/sound.rs:177-179: analyse once and keep the value."""
        self._pitch_confidence = None
        self._pitch_confidence = self.pitch_confidence(engine)

    def mean_mfccs(self) -> np.ndarray:       # src/sound.rs:205, analyze_mean_mfccs :271-286
        m = self.mfccs().reshape(-1, self.ncoeffs)
        acc = np.zeros(self.ncoeffs)
        for row in m:                         # frames in order, like the reference's fold
            acc = acc + row
        return acc / m.shape[0] if m.shape[0] else acc * np.nan

    def samples(self) -> np.ndarray:          # src/sound.rs:181
        return self._samples

    def sample_rate(self) -> float:           # src/sound.rs:185
        return self._sample_rate

    def mfccs(self) -> np.ndarray:            # src/sound.rs:191
        if self._mfccs is None:
            raise ValueError("this Sound carries no features (build it with Sound.from_samples(.., None) to analyse)")
        return self._mfccs

    def has_mfccs(self) -> bool:
        return self._mfccs is not None

    def num_frames(self) -> int:              # src/sound.rs:210
        return self.mfccs().size // self.ncoeffs

    def mfcc_arrays(self) -> np.ndarray:      # src/sound.rs:196-203
        """The features as [frames][ncoeffs] (a view of mfccs(): the reference's chunks of NCOEFFS)."""
        return self.mfccs().reshape(-1, self.ncoeffs)

    def push_samples(self, new_samples, engine: Optional[Engine] = None) -> None:
        """Sound::push_samples (src/sound.rs:145-164): append samples and analyse what they complete.  The first call
        makes the sound resident on the GPU (a one-lane ssym_stream seeded with the samples and the features, which
        are trusted as given, :146-148; frames the samples allow beyond them are analysed with the push); every later
        call uploads only the new samples.  Afterwards samples(), mfccs(), num_frames(),
        max_power() and mean_mfccs() are those of the longer sound -- bit for bit the sound analysed whole.  A preloaded
        pitch confidence stays as it was (:170-179)."""
        push_sounds([self], [new_samples], engine)

    def stream(self):
        """(Stream, lane) holding this sound on the GPU after a push, else None: its frames_device() feeds the
        partitioner and the matcher without a copy."""
        return self._stream


def analyze_sounds(sounds: Sequence[Sound], engine: Optional[Engine] = None, rate: float = PITCH_RATE,
                   f_min: float = PITCH_F_MIN, f_max: float = PITCH_F_MAX, voicing: float = PITCH_VOICING,
                   voiced_only: bool = False):
    """(max_power [n], pitch_confidence [n]) of a list of Sounds in ONE device call (ssym_sound_descriptors).  The
    defaults are the reference's literals (src/sound.rs:265: rate 44100 whatever the sounds' own rates).  max_power is
    the reference's arithmetic (equal to Sound.max_power() up to the summation order of the host helper); the pitch
    side is this package's own definition (parity unpinned).  voiced_only scores a window by its best
    voiced candidate alone (SSYM_PITCH_VOICED).  Arguments outside the limits raise ValueError before any device
    work."""
    pitch_lags(rate, f_min, f_max, voicing)
    sounds = list(sounds)
    if not sounds:
        return np.zeros(0), np.zeros(0)
    parts = [s.samples() for s in sounds]
    offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    e = engine or default_engine()
    return e.sound_descriptors(np.concatenate(parts), offsets, rate, f_min, f_max, voicing, voiced_only)


def _appended(block, old: np.ndarray, new: np.ndarray):
    """(block, old followed by new as a view of it): `block` is the Sound's own growing store (None before the first
    push) and doubles when it runs out, a Vec's amortised push; the caller's arrays are never written to."""
    n = old.size + new.size
    if block is None or block.size < n:
        block = np.empty(max(n, 2 * old.size), dtype=np.float64)
        block[:old.size] = old
    block[old.size:n] = new
    return block, block[:n]


def push_sounds(sounds: Sequence[Sound], chunks, engine: Optional[Engine] = None) -> None:
    """Sound.push_samples for many sounds in ONE device call (a multi-lane ssym_stream_push): chunks[i] is appended to
    sounds[i]; empty chunks are allowed.  The sounds must carry features and share a sample rate and ncoeffs
    (ValueError otherwise, before any device work).  Sounds that were pushed together before keep their shared
    stream; any other grouping opens a new one and seeds every lane once with the sound's samples and features."""
    sounds = list(sounds)
    parts = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in chunks]
    if len(parts) != len(sounds):
        raise ValueError("push_sounds: one chunk per sound")
    if not sounds:
        return
    if len({id(s) for s in sounds}) != len(sounds):
        raise ValueError("push_sounds: a sound appears twice")
    for s in sounds:
        m = s.mfccs()                         # raises the ValueError of mfccs() for a sound without features
        if m.size // s.ncoeffs > Engine.mfcc_num_frames(s.samples().size):
            raise ValueError("push_samples: the sound carries more frames than its samples allow")
    if len({s.sample_rate() for s in sounds}) != 1 or len({s.ncoeffs for s in sounds}) != 1:
        raise ValueError("push_sounds: the sounds must share a sample rate and ncoeffs")
    first = sounds[0]._stream
    shared = first is not None and first[0].ptr and first[0].n_lanes == len(sounds) and \
        (engine is None or first[0].engine is engine) and \
        all(s._stream is not None and s._stream[0] is first[0] and s._stream[1] == i for i, s in enumerate(sounds))
    if shared:
        st = first[0]
    else:
        e = engine or default_engine()
        st = e.stream(len(sounds), sounds[0].sample_rate(), sounds[0].ncoeffs,
                      capacity=2 * max(s.samples().size + p.size for s, p in zip(sounds, parts)))
        for i, s in enumerate(sounds):
            st.seed(i, s.samples(), s.mfccs())
        for i, s in enumerate(sounds):
            if s._stream is not None and len({id(o) for o in sounds if o._stream and o._stream[0] is s._stream[0]}) \
                    == s._stream[0].n_lanes:
                s._stream[0].close()          # every sound of the old stream has moved here
            s._stream = (st, i)
    offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    new, frames = st.push(np.concatenate(parts), offsets, want_frames=True)
    flat, at = frames.reshape(-1), 0
    for s, p, k in zip(sounds, parts, new):
        k = int(k) * s.ncoeffs
        s._blocks[0], s._samples = _appended(s._blocks[0], s._samples, p)
        s._blocks[1], s._mfccs = _appended(s._blocks[1], s._mfccs, flat[at:at + k])
        at += k


class Alignment:
    """One target aligned with a dictionary sound (ssym_dtw_align; definition in include/soundsym_amd.h and DESIGN.md
    section 2): `source_index` into the dictionary's sounds, the DTW `cost` of the pair, `path` an (L, 2) uint32 array
    of (source frame, target frame) cells from (0, 0) to the last frames, and `frame_map` a (target frames,) uint32
    array with the smallest source frame aligned with every target frame.  A pair without a finite cost (an empty
    sound, a band that cuts every path) has an empty path and an empty map.  An alignment of a spotted span
    (SoundDictionary.align(spans=)) counts source frames from the span's first frame: `span_start` is that frame, so
    span_start + frame_map are frames of the recording; it is 0 for every other alignment."""

    __slots__ = ("cost", "path", "frame_map", "source_index", "span_start")

    def __init__(self, cost: float, path, frame_map, source_index: int, span_start: int = 0):
        path = np.asarray(path, dtype=np.uint32)
        if path.ndim != 2 or path.shape[1] != 2:
            raise ValueError("path must be an (L, 2) array of (source frame, target frame) cells")
        frame_map = np.asarray(frame_map, dtype=np.uint32)
        if frame_map.ndim != 1:
            raise ValueError("frame_map must hold one source frame per target frame")
        self.cost, self.path, self.frame_map, self.source_index = float(cost), path, frame_map, int(source_index)
        self.span_start = int(span_start)

    def __len__(self) -> int:
        return int(self.path.shape[0])

    def diagonal_share(self) -> float:
        """Share of the path's steps that advance both sounds (1.0: no warping; 0.0 for a path of one cell)."""
        if len(self) < 2:
            return 0.0
        d = np.diff(self.path.astype(np.int64), axis=0)
        return float(np.mean((d[:, 0] == 1) & (d[:, 1] == 1)))

    def __repr__(self) -> str:
        return "Alignment(source_index=%d, cost=%r, cells=%d)" % (self.source_index, self.cost, len(self))


def _spot_step(step):
    if step not in ("symmetric", "paced"):
        raise ValueError('step must be "symmetric" or "paced"')


def _step_kw(step, max_cost_per_frame=None):
    """The keywords a call passes on for `step`: none at all for the default, so that "symmetric" is the call as it was."""
    kw = {} if step == "symmetric" else {"step": step}
    if max_cost_per_frame is not None:
        kw["max_cost_per_frame"] = max_cost_per_frame
    return kw


def _per_frame(step, cost, frames):
    return float(cost) / float(frames) if step == "paced" else None


def _match_kw(step, match_step):
    """The keywords the match of an align / warp passes on for `match_step`: none at all for None (the symmetric search,
    the call as it was) and for "symmetric"; "paced" searches under the paced pattern and needs the alignment to be paced."""
    if match_step is None:
        return {}
    _spot_step(match_step)
    if match_step == "paced" and step != "paced":
        raise ValueError('match_step="paced" needs step="paced": the match it picks is one the paced alignment can align')
    return {} if match_step == "symmetric" else {"step": match_step}


def _span_args(sounds, spots, targets, indices, match_step, context=False):
    """What align(spans=) and warp(spans=) hand the engine, checked before any library call: (source indices u32, (first,
    last) frames u32, sound indices u32, (first, len) sample windows u64).  An empty Spot is a pair without a source and
    without a span, and an empty window of sound 0.  context: every window runs on to the end of its recording."""
    if indices is not None or match_step is not None:
        raise ValueError("spans name the source of every target themselves: indices and match_step do not go with them")
    spots = list(spots)
    if len(spots) != len(targets):
        raise ValueError("spans must hold one Spot per target")
    n = len(spots)
    src, first, last = (np.full(n, NO_MATCH, dtype=np.uint32) for _ in range(3))
    snd, w_first, w_len = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for t, sp in enumerate(spots):
        if not isinstance(sp, Spot):
            raise ValueError("spans must hold one Spot per target")
        if not sp:
            continue
        if not 0 <= sp.source_index < len(sounds):
            raise ValueError("a spot names a sound outside the dictionary")
        s = sounds[sp.source_index]
        if sp.end_frame >= s.num_frames():
            raise ValueError("a spot ends beyond its sound's frames")
        size = s.samples().size
        a, b = sp.sample_span(size)
        a = min(a, size)
        src[t], first[t], last[t], snd[t] = sp.source_index, sp.start_frame, sp.end_frame, sp.source_index
        w_first[t], w_len[t] = a, (size if context else max(a, b)) - a
    return src, (first, last), snd, (w_first, w_len)


class Spot:
    """Where inside a dictionary recording a target sounds (ssym_dtw_spot / ssym_spot_queries; definition in
    include/soundsym_amd.h and DESIGN.md section 2 "Spotting"): `source_index` into the dictionary's sounds, the frames
    `start_frame` ... `end_frame` (INCLUSIVE) of that recording, and `cost`, the DTW cost of (those frames, the target),
    not normalised by any length.  A target without a spot (an empty sound, an empty recording) gives an empty Spot:
    falsy, no frames, cost +inf.  A spot of the paced step pattern (step="paced"; "Paced spotting") also has
    `cost_per_frame`, cost / the target's frames: every paced path has one cell per target frame, so this mean compares
    across targets of different lengths.  It is None for every other spot."""

    __slots__ = ("source_index", "start_frame", "end_frame", "cost", "cost_per_frame")

    def __init__(self, source_index: int, start_frame: int, end_frame: int, cost: float, cost_per_frame=None):
        self.source_index, self.start_frame, self.end_frame = int(source_index), int(start_frame), int(end_frame)
        self.cost = float(cost)
        self.cost_per_frame = None if cost_per_frame is None else float(cost_per_frame)
        if not self.empty() and not 0 <= self.start_frame <= self.end_frame:
            raise ValueError("a spot spans start_frame ... end_frame with 0 <= start_frame <= end_frame")

    @staticmethod
    def none() -> "Spot":
        return Spot(NO_MATCH, NO_MATCH, NO_MATCH, float("inf"))

    def empty(self) -> bool:
        return NO_MATCH in (self.source_index, self.start_frame, self.end_frame)

    def __bool__(self) -> bool:
        return not self.empty()

    def num_frames(self) -> int:
        return 0 if self.empty() else self.end_frame - self.start_frame + 1

    def sample_span(self, num_samples: int):
        """(first sample, one past the last sample) of the span in a recording of num_samples samples: frame f starts
        at sample f * HOP, and the last frame ends where the next one would start, or with the recording."""
        if self.empty():
            return (0, 0)
        n = int(num_samples)
        return (self.start_frame * HOP, min((self.end_frame + 1) * HOP, n))

    def __repr__(self) -> str:
        if self.empty():
            return "Spot(empty)"
        return "Spot(source_index=%d, frames=%d...%d, cost=%r)" % (self.source_index, self.start_frame, self.end_frame,
                                                                   self.cost)


class Piece:
    """One piece of a Cover: frames `start_frame` ... `end_frame` (INCLUSIVE) of the TARGET, covered by dictionary sound
    `source_index` at `cost`, the paced alignment cost of (that sound, those frames) -- a sum over the piece's frames;
    `cost_per_frame` is cost / num_frames(), a mean that compares across pieces."""

    __slots__ = ("source_index", "start_frame", "end_frame", "cost")
    is_gap = False

    def __init__(self, source_index: int, start_frame: int, end_frame: int, cost: float):
        self.source_index, self.start_frame, self.end_frame = int(source_index), int(start_frame), int(end_frame)
        self.cost = float(cost)
        if self.source_index < 0 or not 0 <= self.start_frame <= self.end_frame:
            raise ValueError("a piece spans start_frame ... end_frame with 0 <= start_frame <= end_frame and names a sound")

    def num_frames(self) -> int:
        return self.end_frame - self.start_frame + 1

    @property
    def cost_per_frame(self) -> float:
        return self.cost / float(self.num_frames())

    def sample_span(self, num_samples: int):
        """(first sample, one past the last sample) of the piece in a target of num_samples samples, by Spot.sample_span's
        rule: frame f starts at sample f * HOP, and the last frame ends where the next one would start, or with the sound."""
        n = int(num_samples)
        return (self.start_frame * HOP, min((self.end_frame + 1) * HOP, n))

    def __repr__(self) -> str:
        return "Piece(source_index=%d, frames=%d...%d, cost=%r)" % (self.source_index, self.start_frame, self.end_frame,
                                                                    self.cost)


class Gap:
    """A maximal run of frames a Cover leaves uncovered (cover(gap_cost=), "Cover with gaps"): frames `start_frame` ...
    `end_frame` (INCLUSIVE) of the TARGET, at `cost` = gap_cost x num_frames(); `cost_per_frame` is the price per frame, the
    figure a Piece's cost_per_frame competed with.  No dictionary sound belongs to it."""

    __slots__ = ("start_frame", "end_frame", "cost")
    is_gap = True

    def __init__(self, start_frame: int, end_frame: int, cost: float):
        self.start_frame, self.end_frame, self.cost = int(start_frame), int(end_frame), float(cost)
        if not 0 <= self.start_frame <= self.end_frame:
            raise ValueError("a gap spans start_frame ... end_frame with 0 <= start_frame <= end_frame")
        if not self.cost >= 0.0:
            raise ValueError("a gap's cost must not be negative or NaN")

    def num_frames(self) -> int:
        return self.end_frame - self.start_frame + 1

    @property
    def cost_per_frame(self) -> float:
        return self.cost / float(self.num_frames())

    def sample_span(self, num_samples: int):
        """(first sample, one past the last sample) of the gap in a target of num_samples samples: Piece.sample_span's rule."""
        n = int(num_samples)
        return (self.start_frame * HOP, min((self.end_frame + 1) * HOP, n))

    def __repr__(self) -> str:
        return "Gap(frames=%d...%d, cost=%r)" % (self.start_frame, self.end_frame, self.cost)


def _cover_tiles(src, start, end, cost) -> List:
    """The Pieces and Gaps of one cover from what the library reports: a gap comes frame by frame as (COVER_GAP, e, e,
    gap_cost), and a run of them is one Gap at gap_cost x its frames."""
    out = []
    for k in range(len(src)):
        if int(src[k]) != COVER_GAP:
            out.append(Piece(src[k], start[k], end[k], cost[k]))
        elif out and out[-1].is_gap and out[-1].end_frame + 1 == int(start[k]):
            run = out[-1]
            out[-1] = Gap(run.start_frame, end[k], float(cost[k]) * (int(end[k]) - run.start_frame + 1))
        else:
            out.append(Gap(start[k], end[k], float(cost[k]) * (int(end[k]) - int(start[k]) + 1)))
    return out


class Cover:
    """A target tiled by dictionary sounds (ssym_dtw_cover; definition in include/soundsym_amd.h and DESIGN.md section 2
    "Cover"): `pieces` in ascending start, tiling frames 0 ... num_frames - 1 of the target, and `total`, the least sum of
    (piece cost + piece_penalty) over every tiling and every choice of sounds.  Every paced path has one cell per target
    frame, so `total_per_frame` = total / num_frames is a mean per frame.  A target without a cover (no frames, a NaN
    frame, a stretch no dictionary sound can pace) gives an empty Cover: falsy, no pieces, total +inf.
    With gaps (cover(gap_cost=), "Cover with gaps") `pieces` holds Gaps among the Pieces -- the tiles, `is_gap` tells them
    apart -- each Gap a maximal run of uncovered frames; total then adds gap_cost per gap frame and no piece_penalty for
    it.  `gaps` are the Gaps, `sounding` the Pieces, `covered_frames` the frames the Pieces cover."""

    __slots__ = ("pieces", "total", "num_frames")

    def __init__(self, pieces: Sequence["Piece"], total: float, num_frames: int):
        self.pieces, self.total, self.num_frames = list(pieces), float(total), int(num_frames)
        if self.num_frames < 0:
            raise ValueError("a cover tiles num_frames >= 0 frames")
        at, after_gap = 0, False
        for p in self.pieces:
            if not isinstance(p, (Piece, Gap)) or p.start_frame != at:
                raise ValueError("the pieces of a cover tile the target: each starts where the one before it ended")
            if p.is_gap and after_gap:
                raise ValueError("a gap of a cover is a maximal run of frames: no gap follows a gap")
            at, after_gap = p.end_frame + 1, p.is_gap
        if self.pieces and at != self.num_frames:
            raise ValueError("the pieces of a cover tile the target: the last one ends with it")

    @staticmethod
    def none(num_frames: int = 0) -> "Cover":
        return Cover([], float("inf"), num_frames)

    def __len__(self) -> int:
        return len(self.pieces)

    def __bool__(self) -> bool:
        return bool(self.pieces)

    @property
    def total_per_frame(self) -> float:
        return self.total / float(self.num_frames) if self.pieces else float("inf")

    @property
    def sounding(self) -> List["Piece"]:
        """The Pieces: the tiles a dictionary sound covers."""
        return [p for p in self.pieces if not p.is_gap]

    @property
    def gaps(self) -> List["Gap"]:
        """The Gaps: the maximal runs of frames left uncovered."""
        return [p for p in self.pieces if p.is_gap]

    @property
    def covered_frames(self) -> int:
        """The frames dictionary sounds cover: num_frames less the gaps' frames (0 for an empty cover)."""
        return sum(p.num_frames() for p in self.pieces if not p.is_gap)

    def indices(self) -> np.ndarray:
        """The dictionary sound of every sounding piece (gaps have none), int64: what align and warp take as indices for
        the cut target."""
        return np.array([p.source_index for p in self.pieces if not p.is_gap], dtype=np.int64)

    def segment_lengths(self, num_samples: int) -> List[int]:
        """The cut as lengths in samples, as Partitioner.partition returns them: num_frames() * HOP per piece, and the
        last piece runs to the end of a sound of num_samples samples.  SoundDictionary.from_segments takes them as they
        are.  An empty cover has no segments.  Every tile counts, gaps included."""
        n = int(num_samples)
        if n < 0:
            raise ValueError("num_samples must not be negative")
        if not self.pieces:
            return []
        if self.pieces[-1].start_frame * HOP > n:
            raise ValueError("the last piece starts beyond num_samples: the cover belongs to a longer sound")
        return [p.num_frames() * HOP for p in self.pieces[:-1]] + [n - self.pieces[-1].start_frame * HOP]

    def __repr__(self) -> str:
        if not self.pieces:
            return "Cover(empty)"
        gaps = self.gaps
        if gaps:
            return "Cover(%d pieces, %d gaps, total=%r)" % (len(self.pieces) - len(gaps), len(gaps), self.total)
        return "Cover(%d pieces, total=%r)" % (len(self.pieces), self.total)


class MosaicPiece:
    """One piece of a Mosaic: frames `start_frame` ... `end_frame` (INCLUSIVE) of the TARGET, played by frames
    `source_first` ... `source_last` (INCLUSIVE) of dictionary sound `source_index` along `frame_map`, the sound's frame for
    every frame of the piece (int64; it advances by 0, 1 or 2 per frame, never by 0 twice in a row).  `cost` is the chain of
    the piece's frame costs, acc = c(first frame), acc = c + acc -- a sum over the piece's frames -- and `cost_per_frame`
    is cost / num_frames(), a mean that compares across pieces."""

    __slots__ = ("source_index", "source_first", "source_last", "start_frame", "end_frame", "cost", "frame_map")
    is_gap = False

    def __init__(self, source_index: int, source_first: int, source_last: int, start_frame: int, end_frame: int, cost: float,
                 frame_map):
        self.source_index, self.source_first, self.source_last = int(source_index), int(source_first), int(source_last)
        self.start_frame, self.end_frame, self.cost = int(start_frame), int(end_frame), float(cost)
        self.frame_map = np.asarray(frame_map, dtype=np.int64).reshape(-1).copy()
        if self.source_index < 0 or not 0 <= self.start_frame <= self.end_frame:
            raise ValueError("a piece spans start_frame ... end_frame with 0 <= start_frame <= end_frame and names a sound")
        if self.frame_map.size != self.num_frames():
            raise ValueError("a piece's frame_map holds one source frame per frame of the piece")
        steps = np.diff(self.frame_map)
        if (self.frame_map[0] != self.source_first or self.frame_map[-1] != self.source_last or self.source_first < 0
                or ((steps < 0) | (steps > 2)).any() or ((steps[1:] == 0) & (steps[:-1] == 0)).any()):
            raise ValueError("a piece's frame_map runs from source_first to source_last in steps of 0, 1 or 2, never 0 twice")

    def num_frames(self) -> int:
        return self.end_frame - self.start_frame + 1

    @property
    def cost_per_frame(self) -> float:
        return self.cost / float(self.num_frames())

    def sample_span(self, num_samples: int):
        """(first sample, one past the last sample) of the piece in a target of num_samples samples: Piece.sample_span's rule."""
        n = int(num_samples)
        return (self.start_frame * HOP, min((self.end_frame + 1) * HOP, n))

    def source_sample_span(self, num_samples: int):
        """(first sample, one past the last sample) of source_first ... source_last in a recording of num_samples samples:
        Spot.sample_span's rule."""
        n = int(num_samples)
        return (min(self.source_first * HOP, n), min((self.source_last + 1) * HOP, n))

    def __repr__(self) -> str:
        return "MosaicPiece(frames=%d...%d, source_index=%d, source frames=%d...%d, cost=%r)" % (
            self.start_frame, self.end_frame, self.source_index, self.source_first, self.source_last, self.cost)


def _mosaic_tiles(start, src, frame, frame_cost, base: int = 0) -> List:
    """The MosaicPieces and Gaps of one mosaic from what the library reports for one target: `start` its piece and gap-frame
    starts (ascending), `src`, `frame` and `frame_cost` its frames.  A gap comes frame by frame, and a run of them is one
    Gap at the sum of its frames' prices; a piece's cost is the chain of its frame costs.  base: the target frame the
    arrays begin at (a stretch of a live mosaic); the tiles count the target's frames."""
    frames = len(src)
    cuts = [int(s) for s in start] + [frames]
    out = []
    for s, e in zip(cuts[:-1], cuts[1:]):
        if int(src[s]) == COVER_GAP:
            if out and out[-1].is_gap:
                run = out[-1]
                out[-1] = Gap(run.start_frame, base + s, float(frame_cost[s]) * (base + s - run.start_frame + 1))
            else:
                out.append(Gap(base + s, base + s, float(frame_cost[s])))
            continue
        acc = float(frame_cost[s])
        for j in range(s + 1, e):
            acc = float(frame_cost[j]) + acc
        out.append(MosaicPiece(src[s], frame[s], frame[e - 1], base + s, base + e - 1, acc, frame[s:e]))
    return out


class Mosaic:
    """A target tiled by free spans of dictionary sounds (ssym_dtw_mosaic; definition in include/soundsym_amd.h and
    DESIGN.md section 2 "Mosaic"): `pieces` in ascending start -- MosaicPieces and, with a gap_cost, Gaps (maximal runs of
    uncovered frames; `is_gap` tells them apart) -- tiling frames 0 ... num_frames - 1 of the target; `total`, the least sum
    over every mosaic of the frame costs, piece_penalty per piece and gap_cost per gap frame; `frame_costs`, c for every
    target frame (gap_cost on a gap frame).  Every tiling has one cell per target frame, so `total_per_frame` = total /
    num_frames is a mean per frame.  A target without a mosaic (no frames; a NaN frame without gaps) gives an empty Mosaic:
    falsy, no pieces, total +inf."""

    __slots__ = ("pieces", "total", "num_frames", "frame_costs")

    def __init__(self, pieces, total: float, num_frames: int, frame_costs=None):
        self.pieces, self.total, self.num_frames = list(pieces), float(total), int(num_frames)
        self.frame_costs = (np.full(self.num_frames, float("inf")) if frame_costs is None else
                            np.asarray(frame_costs, dtype=np.float64).reshape(-1).copy())
        if self.num_frames < 0 or self.frame_costs.size != self.num_frames:
            raise ValueError("a mosaic tiles num_frames >= 0 frames and holds one frame cost for each")
        at, after_gap = 0, False
        for p in self.pieces:
            if not isinstance(p, (MosaicPiece, Gap)) or p.start_frame != at:
                raise ValueError("the pieces of a mosaic tile the target: each starts where the one before it ended")
            if p.is_gap and after_gap:
                raise ValueError("a gap of a mosaic is a maximal run of frames: no gap follows a gap")
            at, after_gap = p.end_frame + 1, p.is_gap
        if self.pieces and at != self.num_frames:
            raise ValueError("the pieces of a mosaic tile the target: the last one ends with it")

    @staticmethod
    def none(num_frames: int = 0) -> "Mosaic":
        return Mosaic([], float("inf"), num_frames)

    def __len__(self) -> int:
        return len(self.pieces)

    def __bool__(self) -> bool:
        return bool(self.pieces)

    @property
    def total_per_frame(self) -> float:
        return self.total / float(self.num_frames) if self.pieces else float("inf")

    @property
    def sounding(self) -> List["MosaicPiece"]:
        """The MosaicPieces: the tiles a dictionary sound plays."""
        return [p for p in self.pieces if not p.is_gap]

    @property
    def gaps(self) -> List["Gap"]:
        """The Gaps: the maximal runs of frames left uncovered."""
        return [p for p in self.pieces if p.is_gap]

    def segment_lengths(self, num_samples: int) -> List[int]:
        """The cut as lengths in samples, by Cover.segment_lengths' rule: num_frames() * HOP per tile, the last tile running
        to the end of a sound of num_samples samples."""
        n = int(num_samples)
        if n < 0:
            raise ValueError("num_samples must not be negative")
        if not self.pieces:
            return []
        if self.pieces[-1].start_frame * HOP > n:
            raise ValueError("the last piece starts beyond num_samples: the mosaic belongs to a longer sound")
        return [p.num_frames() * HOP for p in self.pieces[:-1]] + [n - self.pieces[-1].start_frame * HOP]

    def __repr__(self) -> str:
        if not self.pieces:
            return "Mosaic(empty)"
        gaps = self.gaps
        if gaps:
            return "Mosaic(%d pieces, %d gaps, total=%r)" % (len(self.pieces) - len(gaps), len(gaps), self.total)
        return "Mosaic(%d pieces, total=%r)" % (len(self.pieces), self.total)


def _mosaics(off, count, total, start, src, frame, frame_cost) -> List["Mosaic"]:
    """One Mosaic per target from the six arrays of ssym_dtw_mosaic and the query set's frame offsets."""
    off = np.asarray(off, dtype=np.int64)
    out = []
    for t in range(off.size - 1):
        a, b = int(off[t]), int(off[t + 1])
        if not count[t]:
            out.append(Mosaic.none(b - a))
            continue
        out.append(Mosaic(_mosaic_tiles(start[a:a + int(count[t])], src[a:b], frame[a:b], frame_cost[a:b]), total[t], b - a,
                          frame_cost[a:b]))
    return out


def _cover_sounds(sound: "Sound", cover: "Cover") -> List["Sound"]:
    """The target cut at the cover's pieces: samples by segment_lengths (Piece.sample_span, the last piece running to the
    end of the sound), MFCC rows start_frame ... end_frame.  Gaps are cut out: only the sounding pieces come back."""
    if not isinstance(cover, Cover):
        raise ValueError("a Cover is needed")
    if cover and cover.num_frames != sound.num_frames():
        raise ValueError("the cover tiles another number of frames than the sound has")
    smp, rows = sound.samples(), sound.mfcc_arrays()
    out, at = [], 0
    for p, n in zip(cover.pieces, cover.segment_lengths(smp.size)):
        if not p.is_gap:
            out.append(Sound(smp[at:at + n].copy(), sound.sample_rate(), rows[p.start_frame:p.end_frame + 1].copy(), None,
                             sound.ncoeffs))
        at += n
    return out


class LiveCover:
    """Growing Sounds covered live by a dictionary (`SoundDictionary.cover_live`): the sounds' shared stream followed by a
    Coverer (DESIGN.md section 2 "Live cover").  Pieces are (sound index, Piece), a Piece's frames those of the sound; a
    piece, once returned, is final: it is how the cover of the whole sound starts, whatever the sound gains later.
    With a gap_cost (cover_live(gap_cost=)) a call also returns (sound index, Gap): the gap frames the call committed, a run
    of them as one Gap; the run may go on in the next call, and `covers` merges across calls."""

    def __init__(self, sounds, stream, coverer, piece_penalty: float, gap_cost=None):
        self.sounds, self.stream, self.coverer, self.piece_penalty = sounds, stream, coverer, float(piece_penalty)
        self.gap_cost = gap_cost
        self._emitted = [[] for _ in sounds]             # per sound, the Pieces and Gaps returned so far
        self._costs = [[] for _ in sounds]               # ... and (is a gap frame, cost) as the coverer reported them

    def _pieces(self):
        lane, src, start, end, cost = self.coverer.pieces()
        out = []
        for l in np.unique(lane):
            at = np.flatnonzero(lane == l)
            self._costs[int(l)] += [(int(src[k]) == COVER_GAP, float(cost[k])) for k in at]
            out += [(int(l), p) for p in _cover_tiles(src[at], start[at], end[at], cost[at])]
        for l, p in out:
            self._emitted[l].append(p)
        return out

    def poll(self):
        """Consume what the sounds have gained since the last poll (device to device) and return the pieces that commits,
        ordered by (sound, start)."""
        self.coverer.follow(self.stream)
        return self._pieces()

    def flush(self):
        """"The sounds have ended": the rest of every sound's cover.  The cover consumes nothing more afterwards."""
        out = []
        for lane in range(self.coverer.n_lanes):
            self.coverer.flush(lane)
            out += self._pieces()
        return out

    def covers(self) -> List["Cover"]:
        """One Cover per sound from everything emitted so far: it tiles the frames committed, and its total is the chain's
        own sum over its pieces -- after flush, SoundDictionary.cover's Cover of the sound (of its coverable prefix, when a
        NaN frame or a stretch nothing can pace ends that early)."""
        out = []
        for emitted, costs in zip(self._emitted, self._costs):
            if not emitted:
                out.append(Cover.none(0))
                continue
            acc = 0.0
            for gap, cost in costs:                      # frame by frame; a gap frame carries no piece_penalty
                acc = (cost + acc) if gap else ((cost + self.piece_penalty) + acc)
            pieces = []
            for p in emitted:                            # a run of gap frames that two calls share is one Gap
                if p.is_gap and pieces and pieces[-1].is_gap:
                    first = pieces[-1].start_frame
                    pieces[-1] = Gap(first, p.end_frame, self.gap_cost * (p.end_frame - first + 1))
                else:
                    pieces.append(p)
            out.append(Cover(pieces, acc, pieces[-1].end_frame + 1))
        return out

    def pending(self):
        """(frames consumed, frames covered, frames committed, total), one entry per sound: total is
        SoundDictionary.cover's for what was consumed, +inf without a cover."""
        total, covered, committed = self.coverer.best()
        return self.coverer.counts()[0].astype(np.int64), covered.astype(np.int64), committed.astype(np.int64), total

    def close(self):
        self.coverer.close()


class LiveMosaic:
    """Growing Sounds tiled live by free spans of a dictionary's sounds (`SoundDictionary.mosaic_live`): the sounds' shared
    stream followed by a Mosaicker (DESIGN.md section 2 "Live mosaic").  The mosaicker commits FRAMES, a frame or two
    behind the input at moderate penalties; a piece is closed, and returned by poll as (sound index, MosaicPiece | Gap),
    once the next start -- or the flush -- has been committed.  The open piece's committed frames stay inside the object
    (`committed` shows them).  What is returned is final: it is how the mosaic of the whole sound starts, whatever the
    sound gains later.  A run of gap frames comes as one Gap per call; the run may go on in the next call, and `mosaics`
    merges across calls."""

    def __init__(self, sounds, stream, mosaicker, piece_penalty: float, gap_cost=None, resynth=None, gap_fill: str = "silence",
                 follower=None):
        self.sounds, self.stream, self.mosaicker, self.piece_penalty = sounds, stream, mosaicker, float(piece_penalty)
        self.gap_cost = gap_cost
        # per sound: (src, frame, cost, start) of every committed frame, and the frames already returned as closed pieces
        self._frames = [([], [], [], []) for _ in sounds]
        self._closed = [0 for _ in sounds]
        self._emitted = [[] for _ in sounds]
        self._held = []                                  # pieces closed by a poll that was refused part-way
        # mosaic_live(audio=True): a Resynth takes every frame log; per sound the (samples, pcm) blocks released and not
        # yet returned by audio(), and the sample they start at
        self.resynth, self.gap_fill = resynth, gap_fill
        self._audio = [[] for _ in sounds]
        self._audio_at = [0 for _ in sounds]
        # mosaic_live(dynamics="target"): a Follower takes what audio() has spliced, against the sounds' own samples; per
        # sound whether flush() has ended it and whether the follower's lane has been flushed since
        self.follower = follower
        self._ended = [False for _ in sounds]
        self._followed = [False for _ in sounds]

    def _take(self, ended=()):
        lane, col, src, frame, cost, start = self.mosaicker.frames()
        for k in range(lane.size):
            rows = self._frames[int(lane[k])]
            if int(col[k]) != len(rows[0]):
                raise RuntimeError("the mosaicker's frames do not continue the frames committed before")
            for row, v in zip(rows, (int(src[k]), int(frame[k]), float(cost[k]), int(start[k]))):
                row.append(v)
        out = []
        for l, (src, frame, cost, start) in enumerate(self._frames):
            a, n = self._closed[l], len(src)
            cuts = [j for j in range(a, n) if start[j]]
            b = n if l in ended else (cuts[-1] if cuts else a)       # the last start opens a piece that may still grow
            if b <= a:
                continue
            tiles = _mosaic_tiles([j - a for j in cuts if j < b], src[a:b], np.array(frame[a:b], dtype=np.uint32), cost[a:b], a)
            self._closed[l] = b
            self._emitted[l] += tiles
            out += [(l, p) for p in tiles]
        if self._held:
            out = sorted(self._held + out, key=lambda t: (t[0], t[1].start_frame))
            self._held = []
        return out

    def poll(self):
        """Consume what the sounds have gained since the last poll (device to device) and return the pieces that closes,
        ordered by (sound, start).  A poll the mosaicker refuses part-way (SSYM_E_UNSUPPORTED: a sound's uncommitted
        stretch fills the mosaicker's memory) raises, but what it consumed stays consumed and what it committed is kept:
        `committed` shows it, and the pieces it closed come with the next poll or flush."""
        try:
            self.mosaicker.follow(self.stream)
        except SsymError as err:
            if err.code == SSYM_E_UNSUPPORTED:
                self._held = self._take()
                self._take_audio()
            raise
        out = self._take()
        self._take_audio()
        return out

    def flush(self):
        """"The sounds have ended": the rest of every sound's mosaic.  The mosaic consumes nothing more afterwards.  With
        audio, every sound's resynthesis ends too, at len(sound.samples()) samples."""
        out = []
        for lane in range(self.mosaicker.n_lanes):
            self.mosaicker.flush(lane)
            out += self._take(ended=(lane,))
            self._take_audio()
            if self.resynth is not None:
                self.resynth.flush(lane, len(self.sounds[lane].samples()))
                self._gather_audio()
                self._ended[lane] = True
        return sorted(out, key=lambda t: (t[0], t[1].start_frame))   # (only pieces held from a refused poll move)

    def _take_audio(self):
        """The resynthesiser consumes the mosaicker's last frame log, device to device; what that releases is kept for audio()."""
        if self.resynth is not None:
            self.resynth.take(self.mosaicker)
            self._gather_audio()

    def _gather_audio(self):
        if not self.resynth.n_samples:
            return
        off, smp, pcm = self.resynth.samples(want_pcm32=True)
        for l in range(len(self.sounds)):
            a, b = int(off[l]), int(off[l + 1])
            if b > a:
                self._audio[l].append((smp[a:b], pcm[a:b]))

    def audio(self, want_pcm32: bool = False):
        """mosaic_live(audio=True): per sound, the samples released since the last call (f64; with want_pcm32 (samples,
        pcm int32)).  Released samples are final: concatenated from the first poll to flush they are
        reconstruct_mosaic(sound, mosaic=mosaics()[i], search=, gap_fill=)'s, bit for bit.  A sample leaves when no later
        frame can change it: at most 4 frames behind the committed frames for search = 0, at most 12 with a search (DESIGN.md
        section 2 "Live resynthesis").  gap_fill="target": gap stretches are filled here, on the host, with the sound's own
        samples, as reconstruct_mosaic fills them.  With dynamics="target" what is returned has gone through the LiveMosaic's
        Follower as well, after the gap splice, against the sound's own samples: it trails the resynthesiser by two more
        hops, and from the first poll to flush it is reconstruct_mosaic(..., dynamics="target", max_gain=)'s, bit for bit."""
        if self.resynth is None:
            raise ValueError("audio: the LiveMosaic was made without audio (mosaic_live(audio=True))")
        out = []
        for l, sound in enumerate(self.sounds):
            parts, self._audio[l] = self._audio[l], []
            smp = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0)
            pcm = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.int32)
            src = self._frames[l][0]
            if self.gap_fill == "target" and smp.size and src:
                k = np.arange(self._audio_at[l], self._audio_at[l] + smp.size)
                gap = np.array(src, dtype=np.uint32)[np.minimum(k // HOP, len(src) - 1)] == COVER_GAP   # the last tile runs to the end
                own = np.asarray(sound.samples(), dtype=np.float64)[k[gap]]
                smp[gap] = own
                with np.errstate(invalid="ignore", over="ignore"):
                    x = np.nan_to_num(2147483647.0 * own, nan=0.0)
                    pcm[gap] = np.trunc(np.clip(x, -2147483648.0, 2147483647.0)).astype(np.int64).astype(np.int32)
            self._audio_at[l] += smp.size
            out.append((smp, pcm) if want_pcm32 else smp)
        return out if self.follower is None else self._follow(out, want_pcm32)

    def _follow(self, spliced, want_pcm32: bool):
        """What audio() has spliced goes into the follower, one push for all sounds, with the sounds' own samples up to the
        same count; a sound that flush() has ended is then flushed there too.  Returns what that released, per sound."""
        spliced = [p[0] if want_pcm32 else p for p in spliced]
        ny, nx, _ = self.follower.counts()
        ref = []
        for l, (sound, smp) in enumerate(zip(self.sounds, spliced)):
            own = np.asarray(sound.samples(), dtype=np.float64).reshape(-1)
            ref.append(own[min(int(nx[l]), own.size):min(int(ny[l]) + smp.size, own.size)])
        parts = [[] for _ in self.sounds]

        def gather():
            if self.follower.n_samples:
                off, smp, pcm = self.follower.samples(want_pcm32=True)
                for l in range(len(self.sounds)):
                    a, b = int(off[l]), int(off[l + 1])
                    if b > a:
                        parts[l].append((smp[a:b], pcm[a:b]))
        if any(a.size for a in spliced) or any(a.size for a in ref):
            offsets = lambda arrays: np.concatenate([[0], np.cumsum([a.size for a in arrays])]).astype(np.uint64)      # noqa: E731
            self.follower.push(np.concatenate(spliced), offsets(spliced), np.concatenate(ref), offsets(ref))
            gather()
        for l in range(len(self.sounds)):
            if self._ended[l] and not self._followed[l]:
                self.follower.flush(l)
                self._followed[l] = True
                gather()
        out = []
        for p in parts:
            smp = np.concatenate([q[0] for q in p]) if p else np.zeros(0)
            pcm = np.concatenate([q[1] for q in p]) if p else np.zeros(0, dtype=np.int32)
            out.append((smp, pcm) if want_pcm32 else smp)
        return out

    def committed(self):
        """Per sound (src uint32, frame uint32, frame_cost f64, start bool), one entry per committed frame -- the open
        piece's included: what a caller that resynthesises frame by frame reads (a gap frame: COVER_GAP, NO_MATCH,
        gap_cost)."""
        return [(np.array(s, dtype=np.uint32), np.array(f, dtype=np.uint32), np.array(c, dtype=np.float64),
                 np.array(a, dtype=bool)) for s, f, c, a in self._frames]

    def mosaics(self) -> List["Mosaic"]:
        """One Mosaic per sound from every frame committed so far: it tiles those frames, and its total is the recurrence's
        own sum over them -- after flush, SoundDictionary.mosaic's Mosaic of the sound (of its prefix with a mosaic, when
        a NaN frame ends that early without gaps)."""
        out = []
        for src, frame, cost, start in self._frames:
            if not src:
                out.append(Mosaic.none(0))
                continue
            acc = 0.0
            for s, c, a in zip(src, cost, start):
                acc = (c + (self.piece_penalty + acc)) if a and s != COVER_GAP else (c + acc)
            cuts = [j for j in range(len(src)) if start[j]]
            out.append(Mosaic(_mosaic_tiles(cuts, src, np.array(frame, dtype=np.uint32), cost), acc, len(src), cost))
        return out

    def pending(self):
        """(frames consumed, frames with a mosaic, frames committed, total), one entry per sound: total is
        SoundDictionary.mosaic's for what was consumed, +inf without a mosaic."""
        total, covered, committed = self.mosaicker.best()
        return self.mosaicker.counts()[0].astype(np.int64), covered.astype(np.int64), committed.astype(np.int64), total

    def close(self):
        if self.follower is not None:
            self.follower.close()
        if self.resynth is not None:
            self.resynth.close()
        self.mosaicker.close()


def _shared_stream(sounds, what: str):
    """The stream that resident sounds share, sound i in lane i -- what one push_sounds(sounds, ...) leaves."""
    first = sounds[0]._stream if sounds else None
    if first is None or not first[0].ptr or first[0].n_lanes != len(sounds) or \
            any(s._stream is None or s._stream[0] is not first[0] or s._stream[1] != i for i, s in enumerate(sounds)):
        raise ValueError(what + ": the sounds must share one stream (feed them together with push_sounds first)")
    return first[0]


class Watch:
    """Targets watched in growing Sounds (`watch`): the sounds' shared stream followed by a Spotter.  Events are
    (sound index, target index, Spot) with Spot.source_index the sound index; frames are those of the sound, so
    Spot.sample_span applies as it is.  Under step="paced" every Spot carries cost_per_frame, cost / the target's
    frames."""

    def __init__(self, sounds, stream, spotter, queries, frames=None):
        self.sounds, self.stream, self.spotter, self._queries = sounds, stream, spotter, queries
        self._frames = frames                 # per target, for cost_per_frame

    def _spot(self, lane, t, start, end, cost):
        step = getattr(self.spotter, "step", "symmetric")
        return Spot(lane, start, end, cost, _per_frame(step, cost, self._frames[t]) if step == "paced" else None)

    def _events(self):
        lane, tgt, cost, start, end = self.spotter.events()
        return [(int(lane[k]), int(tgt[k]), self._spot(int(lane[k]), int(tgt[k]), int(start[k]), int(end[k]), cost[k]))
                for k in range(lane.size)]

    def poll(self):
        """Consume what the sounds have gained since the last poll (in place, on the GPU) and return the events that
        emits, ordered by (sound, target, end)."""
        self.spotter.follow(self.stream)
        return self._events()

    def flush(self):
        """"The sounds have ended": what is pending is emitted, for every sound."""
        out = []
        for lane in range(self.spotter.n_lanes):
            self.spotter.flush(lane)
            out += self._events()
        return out

    def best(self):
        """[sound][target] the best span so far as a Spot (SoundDictionary.spot's for what was consumed)."""
        cost, start, end = self.spotter.best()
        return [[self._spot(l, t, int(start[l, t]), int(end[l, t]), cost[l, t]) if int(end[l, t]) != NO_MATCH else Spot.none()
                 for t in range(cost.shape[1])] for l in range(cost.shape[0])]

    def close(self):
        self.spotter.close()
        self._queries.close()


def watch(sounds: Sequence[Sound], targets: Sequence[Sound], max_cost=None, engine: Optional[Engine] = None,
          step: str = "symmetric", max_cost_per_frame=None) -> Watch:
    """Watch for `targets` in Sounds that are fed with push_samples / push_sounds (streaming DTW spotting, DESIGN.md
    section 2 "Watching"; dtw engines without a band).  The sounds must be resident and share one stream, sound i in lane
    i -- what one push_sounds(sounds, ...) leaves -- ValueError otherwise, before any device work.  max_cost: a scalar or
    one value per target.  The first poll consumes everything the sounds hold.  step="paced": the paced step pattern
    ("Paced watching": spans of about half to twice the target's frames, Spot.cost_per_frame set, and a NaN frame in a
    sound costs a bounded stretch, not the rest of the lane); max_cost_per_frame (instead of max_cost; a scalar or one
    value per target) is then a threshold on that mean: target t's events cost at most max_cost_per_frame * its frames, so
    one value serves targets of every length."""
    _spot_step(step)
    if max_cost_per_frame is not None:
        if max_cost is not None:
            raise ValueError("max_cost and max_cost_per_frame exclude each other")
        if step != "paced":
            raise ValueError('max_cost_per_frame needs step="paced": only there is cost / frames a mean per-frame distance')
    sounds, targets = list(sounds), list(targets)
    st = _shared_stream(sounds, "watch")
    e = engine or st.engine
    if e is not st.engine:
        raise ValueError("watch: the engine must be the one that holds the sounds' stream")
    if getattr(e, "metric", None) != "dtw":
        raise SsymError(SSYM_E_UNSUPPORTED, "watch aligns with dtw: a refcos engine has no alignment")
    if any(t.ncoeffs != st.ncoeffs for t in targets):
        raise ValueError("watch: the targets' ncoeffs must be the sounds'")
    if max_cost is not None:
        mc = np.asarray(max_cost, dtype=np.float64)
        if mc.ndim and mc.size != len(targets):
            raise ValueError("max_cost must be a scalar or one value per target")
        if np.isnan(mc).any():
            raise ValueError("max_cost must not be NaN")
    if max_cost_per_frame is not None:
        max_cost_per_frame = np.asarray(max_cost_per_frame, dtype=np.float64)
        if max_cost_per_frame.ndim and max_cost_per_frame.size != len(targets):
            raise ValueError("max_cost_per_frame must be a scalar or one value per target")
        if np.isnan(max_cost_per_frame).any():
            raise ValueError("max_cost_per_frame must not be NaN")
    flat, off = pack_segments([t.mfccs() for t in targets], st.ncoeffs, e.np_dtype)
    frames = np.diff(off.astype(np.int64))
    if max_cost_per_frame is not None:
        # a sum per target, in f64 on the host: max_cost[t] = x * Fb[t]; a target without frames has no candidate anyway,
        # and +inf * 0 would be the NaN that creation refuses
        x = np.broadcast_to(max_cost_per_frame.reshape(-1), (len(targets),))
        max_cost = np.where(frames >= 1, x * np.maximum(frames, 1).astype(np.float64), np.inf)
    q = e.queries(flat, off, st.ncoeffs)
    try:
        sp = e.spotter(q, len(sounds), max_cost, **_step_kw(step))
    except Exception:
        q.close()
        raise
    return Watch(sounds, st, sp, q, frames)


def _follow_targets(engine, res, targets, gain, want_pcm32: bool):
    """The dynamics="target" tail of the reconstructing methods.  res is what the method would have returned from its
    synthesis: the samples, or a tuple that starts with them (then their 32-bit conversion with want_pcm32, then whatever
    else).  The samples go through ONE Engine.follow_envelope call against the targets' own samples, target by target;
    the samples and the conversion are replaced by that call's, everything else stays."""
    parts = res if isinstance(res, tuple) else (res,)
    ref = [np.asarray(t.samples(), dtype=np.float64).reshape(-1) for t in targets]
    off = np.concatenate([[0], np.cumsum([r.size for r in ref])]).astype(np.uint64)
    out = engine.follow_envelope(parts[0], off, np.concatenate(ref) if ref else np.zeros(0), off, gain, want_pcm32)
    out = out if isinstance(out, tuple) else (out,)
    new = out + tuple(parts[len(out):])
    return new if isinstance(res, tuple) else new[0]


def follow_envelope(sound: Sound, reference: Sound, max_gain: float = FOLLOW_MAX_GAIN, engine: Optional[Engine] = None) -> Sound:
    """`sound` with the loudness of `reference`, hop by hop (ssym_follow_envelope; definition in include/soundsym_amd.h):
    a new Sound of sound's length, rate and name whose features are analysed when they are asked for.  Where the
    reference is shorter it counts as silent; what it has beyond sound's length is not used.  max_gain: the greatest
    gain, finite and at least 1."""
    gain = follow_dynamics("target", max_gain)
    if not isinstance(sound, Sound) or not isinstance(reference, Sound):
        raise ValueError("follow_envelope takes two Sounds")
    y, x = sound.samples(), reference.samples()
    out = (engine or default_engine()).follow_envelope(y, [0, y.size], x, [0, x.size], gain)
    return Sound(out, sound.sample_rate(), None, sound.name, sound.ncoeffs)


class SoundDictionary:
    """Cache of Sounds searched by similarity (src/sound.rs:290-371)."""

    def __init__(self, engine: Optional[Engine] = None):
        self._sounds = _SoundList()           # `pub sounds: Vec<Arc<Sound>>` (the `sounds` property below)
        self._engine = engine
        self._resident = None
        self._resident_key = None
        self._samples_res = None
        self._samples_key = None

    # constructors -----------------------------------------------------------------------------
    @staticmethod
    def new(engine: Optional[Engine] = None) -> "SoundDictionary":     # src/sound.rs:296
        return SoundDictionary(engine)

    @staticmethod
    def from_path(path, engine: Optional[Engine] = None) -> "SoundDictionary":
        """SoundDictionary::from_path (src/sound.rs:304-321): every *.wav of a directory, in directory
        order (sorted here, so that indices do not depend on the file system), features analysed -- one
        ssym_mfcc_batch per sample rate, each sound's features bit for bit those of Sound.from_path."""
        import os
        from . import io as sio
        d = SoundDictionary(engine)
        files = []
        for name in sorted(os.listdir(str(path))):
            if os.path.splitext(name)[1] != ".wav":
                continue
            samples, rate = sio.read_wav(os.path.join(str(path), name))
            files.append((np.ascontiguousarray(samples, dtype=np.float64).reshape(-1), float(rate),
                          os.path.splitext(name)[0]))
        feats = [None] * len(files)
        for rate in dict.fromkeys(f[1] for f in files):
            which = [i for i, f in enumerate(files) if f[1] == rate]
            for i, m in zip(which, analyze_mfccs([files[i][0] for i in which], rate, NCOEFFS, engine)):
                feats[i] = m
        for (samples, rate, stem), m in zip(files, feats):
            d.sounds.append(Sound(samples, rate, m, stem, NCOEFFS))
        return d

    @staticmethod
    def from_segments(sound: Sound, segments: Sequence[int],
                      engine: Optional[Engine] = None) -> "SoundDictionary":   # src/sound.rs:323
        d = SoundDictionary(engine)
        d.add_segments(sound, segments)
        return d

    def add_segments(self, sound: Sound, segments: Sequence[int]) -> None:
        """src/sound.rs:330-343: consecutive `seg` samples and `seg / HOP * ncoeffs` feature
        values per segment (integer division), taken in order from the parent sound; a segment
        running past the end gets what is left, like `take` on an exhausted iterator."""
        samples, mfccs = sound.samples(), sound.mfccs()
        spos = mpos = 0
        for seg in segments:
            seg = int(seg)
            samp = samples[spos:spos + seg]
            spos = min(spos + seg, samples.size)
            nm = seg // HOP * sound.ncoeffs
            mf = mfccs[mpos:mpos + nm]
            mpos = min(mpos + nm, mfccs.size)
            self.sounds.append(Sound(samp.copy(), sound.sample_rate(), mf.copy(), None, sound.ncoeffs))

    # device residency ---------------------------------------------------------------------------
    @property
    def engine(self) -> Engine:
        if self._engine is None:
            self._engine = default_engine()
        return self._engine

    def _dim(self) -> int:
        return self.sounds[0].ncoeffs

    @property
    def sounds(self) -> List[Sound]:
        return self._sounds

    @sounds.setter
    def sounds(self, value) -> None:
        self._sounds = _SoundList(value)      # a fresh list object: its identity is part of the key below

    def _content_key(self):
        """What `sounds` holds now, in O(1).  `sounds` is the public, mutable list (`pub sounds`): entries may have
        been replaced, reordered, or popped and pushed since the last pack, so the length alone does not say.  The
        list counts its own mutations (_SoundList.version) and assigning a new list makes a new object, so (the list
        object, its version) changes whenever the content can have; a Sound's arrays are fixed at construction.  The
        key holds the list, so its identity cannot be reused while the key is kept."""
        return (self._sounds, self._sounds.version)

    @staticmethod
    def _same(key, now) -> bool:
        return key is not None and key[0] is now[0] and key[1] == now[1]

    def invalidate(self) -> None:
        """Drop the GPU copies (they are rebuilt on the next query)."""
        if self._resident is not None:
            self._resident.close()
        self._resident = self._resident_key = None
        if self._samples_res is not None:
            self._samples_res.close()
        self._samples_res = self._samples_key = None

    def resident(self):
        """Pack the dictionary's features once per content change, not per query."""
        key = self._content_key()
        if self._resident is None or not self._same(self._resident_key, key):
            if self._resident is not None:
                self._resident.close()
            dim = self._dim() if self.sounds else NCOEFFS
            flat, off = pack_segments([s.mfccs() for s in self.sounds], dim, self.engine.np_dtype)
            self._resident = self.engine.dictionary(flat, off, dim)
            self._resident_key = key
        return self._resident

    def resident_samples(self):
        """The sounds' samples on the GPU, for the reconstruction tail (ssym_samples_create)."""
        key = self._content_key()
        if self._samples_res is None or not self._same(self._samples_key, key):
            if self._samples_res is not None:
                self._samples_res.close()
            smp = [s.samples() for s in self.sounds]
            off = np.concatenate([[0], np.cumsum([x.size for x in smp])]).astype(np.uint64)
            flat = np.concatenate(smp) if smp else np.zeros(0)
            self._samples_res = self.engine.samples(flat, off)
            self._samples_key = key
        return self._samples_res

    # queries ------------------------------------------------------------------------------------
    def match_sound(self, other: Sound) -> Sound:                       # src/sound.rs:346
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")          # reference: panic, :369
        default = 1.0 if self.engine.metric == "refcos" else 0.0
        return self.at_distance(default, other)

    def at_distance(self, distance: float, other: Sound) -> Sound:      # src/sound.rs:351
        if not self.sounds:
            # the reference indexes an empty Vec and panics (src/sound.rs:369)
            raise EmptyDictionaryError(-2, "empty dictionary")
        idx, _ = self.engine.match_one(self.resident(), other.mfccs(), distance)
        return self.sounds[idx]              # Some(self.sounds[min_idx].clone())

    def match_indices(self, targets: Sequence[Sound], distances=None, step: str = "symmetric", per_frame: bool = False):
        """Batched form of the loops at src/sound.rs:442-446 and :453-454.  step="paced": the search runs under the paced
        step pattern (ssym_match_queries_step with SSYM_STEP_PACED, dtw engines): the cost of a pair is its paced
        alignment's, +inf where the shapes admit no paced path, so the match is one align(step="paced") can align, at the
        same cost; a target nothing fits gets index 0 and +inf.  Every paced path has one cell per target frame, so with
        per_frame=True the distances are means per frame (multiplied by the target's frames before the call) and the
        returned costs are divided by them: values that compare across targets of every length."""
        _spot_step(step)
        if per_frame and step != "paced":
            raise ValueError('per_frame needs step="paced": only there is cost / frames a mean per-frame distance')
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        if step == "symmetric":
            return self.engine.match_batch(self.resident(), flat, off, distances)
        frames = np.diff(np.asarray(off, dtype=np.int64)).astype(np.float64)
        if distances is not None:
            distances = np.asarray(distances, dtype=np.float64).reshape(-1)
            if per_frame:
                distances = distances * frames
        q = self.engine.queries(flat, off, self._dim())
        try:
            idx, cost = self.engine.match(self.resident(), q, distances, step=step)
        finally:
            q.close()
        if per_frame:
            with np.errstate(divide="ignore", invalid="ignore"):
                cost = cost / frames
        return idx, cost


    def align(self, targets: Sequence[Sound], indices=None, step: str = "symmetric", match_step=None,
              spans=None) -> List["Alignment"]:
        """The warping path of every target onto a dictionary sound (dtw engines; ssym_dtw_align).  indices=None:
        every target is matched first (match_indices) and aligned with its match -- two library calls in all;
        otherwise indices[t] is the dictionary sound target t is aligned with.  step="paced": the paced step pattern
        (ssym_dtw_align_step with SSYM_STEP_PACED) -- the alignment of a span that spot(step="paced") found and cut()
        took out: one source frame per target frame, so the path has as many cells as the target has frames and
        frame_map is its first column; a sound too short or too long for the target (outside about half to twice its
        frames) has no such path and gives an empty Alignment.  match_step (looked at with indices=None): None keeps the
        symmetric search, which may pick such a sound; "paced" (with step="paced" only) searches under the paced pattern
        (match_indices(step="paced")), so every match that has a finite cost is aligned at that cost.  spans: one Spot per
        target (what spot and spot_all return; not with indices or match_step) -- target t is aligned with frames
        start_frame ... end_frame of recording source_index where they lie, in the resident dictionary
        (ssym_dtw_align_spans): the results of cut(spots).align(targets, indices=arange) bit for bit, with
        Alignment.source_index the recording, path and frame_map counted from Alignment.span_start = start_frame, and an
        empty Alignment for an empty Spot."""
        _spot_step(step)
        targets = list(targets)
        if spans is not None:
            src, frames, _, _ = _span_args(self.sounds, spans, targets, indices, match_step)
            if not self.sounds:
                raise EmptyDictionaryError(-2, "empty dictionary")
            if not targets:
                return []
            flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
            q = self.engine.queries(flat, off, self._dim())
            try:
                cost, _, paths, maps = self.engine.dtw_align(self.resident(), q, src, spans=frames, **_step_kw(step))
            finally:
                q.close()
            return [Alignment(cost[t], paths[t], maps[t], int(src[t]), 0 if src[t] == NO_MATCH else int(frames[0][t]))
                    for t in range(len(targets))]
        match_kw = _match_kw(step, match_step)
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        if indices is not None:
            indices = np.asarray(indices, dtype=np.int64).reshape(-1)
            if indices.size != len(targets):
                raise ValueError("indices must name one dictionary sound per target")
            if indices.size and (indices.min() < 0 or indices.max() >= len(self.sounds)):
                raise ValueError("an index is outside the dictionary")
        if not targets:
            return []
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        q = self.engine.queries(flat, off, self._dim())
        try:
            if indices is None:
                indices, _ = self.engine.match(self.resident(), q, **match_kw)
            cost, _, paths, maps = self.engine.dtw_align(self.resident(), q, indices, **_step_kw(step))
        finally:
            q.close()
        return [Alignment(cost[t], paths[t], maps[t], int(indices[t])) for t in range(len(targets))]

    def warp(self, targets: Sequence[Sound], indices=None, want_pcm32: bool = False, search: int = 0,
             want_pos: bool = False, step: str = "symmetric", match_step=None, spans=None, context: bool = False,
             dynamics=None, max_gain: float = FOLLOW_MAX_GAIN):
        """The reconstruction of the targets with every match warped onto its target's timing (dtw engines): match
        (unless indices[t] names the dictionary sound of target t), align with the outputs left on the device, and
        resynthesise along the maps -- ssym_match_queries, ssym_dtw_align, ssym_reconstruct_warped; the maps never
        visit the host.  Returns the concatenated samples, one stretch of len(target.samples()) per target (with
        want_pcm32 also their 32-bit conversion).  A target without a finite alignment takes the length fit of
        reconstruct_from_dictionary.  search > 0 (at most 512 samples): ssym_reconstruct_wsola in place of the last
        call -- every source frame may move that far to continue the frame before it in phase; want_pos then also
        returns the frames' sample starts and the map offsets they are laid out by (Engine.reconstruct_wsola).
        step="paced": the alignment is the paced one (align), whose maps move by 0, 1 or 2 source frames per target frame
        and never stand still twice in a row; a pair whose shape admits no paced path takes the length fit.  match_step
        as for align: "paced" (with step="paced") matches under the paced pattern too, so that no target falls back to the
        length fit because the symmetric search chose a sound of the wrong length.  spans: one Spot per target (not with
        indices or match_step) -- every span is aligned and resynthesised where it lies, from the resident dictionary and
        the resident samples (ssym_dtw_align_spans, then ssym_reconstruct_warped_spans or ssym_reconstruct_wsola_spans over
        the samples of spot.sample_span()): the results of cut(spots).warp(targets, indices=arange) bit for bit, zeros for an
        empty Spot, with no second dictionary and no second sample store.  context=True (with spans) lets every window run
        on to the end of its recording: look-ahead taps and WSOLA candidates past the span's end then read the
        recording's real continuation instead of dropping out; nothing else changes.  dynamics="target": what the call
        would have returned goes through one Engine.follow_envelope call against the targets' own samples, so every
        stretch takes its target's loudness, no gain above max_gain (None: this method as it was, no extra call)."""
        _spot_step(step)
        gain = follow_dynamics(dynamics, max_gain)
        targets = list(targets)
        span_args = None
        if spans is not None:
            span_args = _span_args(self.sounds, spans, targets, indices, match_step, bool(context))
        elif context:
            raise ValueError("context widens the sample windows of spans: it needs spans")
        match_kw = _match_kw(step, match_step)
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        if getattr(self.engine, "metric", None) != "dtw":
            raise SsymError(SSYM_E_UNSUPPORTED, "warp follows dtw alignments: a refcos engine has none")
        search = _wsola_search(search)
        if want_pos and not search:
            raise ValueError("want_pos needs search > 0: without a search the positions are the map times 256")
        if indices is not None:
            indices = np.asarray(indices, dtype=np.int64).reshape(-1)
            if indices.size != len(targets):
                raise ValueError("indices must name one dictionary sound per target")
            if indices.size and (indices.min() < 0 or indices.max() >= len(self.sounds)):
                raise ValueError("an index is outside the dictionary")
        if not targets:
            res = (np.zeros(0),) + ((np.zeros(0, dtype=np.int32),) if want_pcm32 else ())
            res += (np.zeros(0, dtype=np.uint64), np.zeros(1, dtype=np.uint64)) if want_pos else ()
            return res if len(res) > 1 else res[0]
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        out_off = np.concatenate([[0], np.cumsum([t.samples().size for t in targets])]).astype(np.uint64)
        q = self.engine.queries(flat, off, self._dim())
        try:
            if span_args is not None:
                res = self._warp_spans(q, span_args, out_off, step, search, want_pcm32, want_pos)
                return res if gain is None else _follow_targets(self.engine, res, targets, gain, want_pcm32)
            if indices is None:
                indices, _ = self.engine.match(self.resident(), q, **match_kw)
            _, lengths, _, maps, _, m_off = self.engine.dtw_align_device(self.resident(), q, indices, **_step_kw(step))
            if not search:
                res = self.engine.reconstruct_warped(self.resident_samples(), indices, out_off, maps, m_off,
                                                     np.diff(m_off.astype(np.int64)), lengths, want_pcm32)
                return res if gain is None else _follow_targets(self.engine, res, targets, gain, want_pcm32)
            res = self.engine.reconstruct_wsola(self.resident_samples(), indices, out_off, maps, m_off,
                                                np.diff(m_off.astype(np.int64)), lengths, search, want_pcm32, want_pos)
            res = res + (m_off,) if want_pos else res
            return res if gain is None else _follow_targets(self.engine, res, targets, gain, want_pcm32)
        finally:
            q.close()

    def _warp_spans(self, q, span_args, out_off, step, search, want_pcm32, want_pos):
        """The tail of warp(spans=) and reconstruct_spotted: span alignment with the outputs left on the device, then the
        window reconstruction -- two library calls on the resident query set q; maps and lengths never visit the host."""
        src, frames, snd, windows = span_args
        _, lengths, _, maps, _, m_off = self.engine.dtw_align_device(self.resident(), q, src, spans=frames, **_step_kw(step))
        if not search:
            return self.engine.reconstruct_warped(self.resident_samples(), snd, out_off, maps, m_off,
                                                  np.diff(m_off.astype(np.int64)), lengths, want_pcm32, windows=windows)
        res = self.engine.reconstruct_wsola(self.resident_samples(), snd, out_off, maps, m_off,
                                            np.diff(m_off.astype(np.int64)), lengths, search, want_pcm32, want_pos,
                                            windows=windows)
        return res + (m_off,) if want_pos else res

    def reconstruct_spotted(self, targets: Sequence[Sound], step: str = "symmetric", search: int = 0,
                            want_pcm32: bool = False, dynamics=None, max_gain: float = FOLLOW_MAX_GAIN):
        """spot, then warp(spans=) on one upload of the targets: every target is located in the dictionary's recordings
        (ssym_spot_queries), its span aligned with the outputs left on the device (ssym_dtw_align_spans) and
        resynthesised from the resident samples (ssym_reconstruct_warped_spans, or with search > 0
        ssym_reconstruct_wsola_spans) -- three library calls, one query set, no cut.  Returns (spots, samples), with
        want_pcm32 (spots, samples, pcm).  dynamics and max_gain as for warp."""
        _spot_step(step)
        gain = follow_dynamics(dynamics, max_gain)
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        if getattr(self.engine, "metric", None) != "dtw":
            raise SsymError(SSYM_E_UNSUPPORTED, "reconstruct_spotted aligns with dtw: a refcos engine has no alignment")
        search = _wsola_search(search)
        targets = list(targets)
        if not targets:
            return ([], np.zeros(0)) + ((np.zeros(0, dtype=np.int32),) if want_pcm32 else ())
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        out_off = np.concatenate([[0], np.cumsum([t.samples().size for t in targets])]).astype(np.uint64)
        frames = np.diff(off.astype(np.int64))
        q = self.engine.queries(flat, off, self._dim())
        try:
            indices, cost, start, end = self.engine.spot_queries(self.resident(), q, **_step_kw(step))
            spots = [Spot(int(indices[t]), int(start[t]), int(end[t]), cost[t], _per_frame(step, cost[t], frames[t]))
                     if int(end[t]) != NO_MATCH else Spot.none() for t in range(len(targets))]
            res = self._warp_spans(q, _span_args(self.sounds, spots, targets, None, None), out_off, step, search,
                                   want_pcm32, False)
        finally:
            q.close()
        if gain is not None:
            res = _follow_targets(self.engine, res, targets, gain, want_pcm32)
        return (spots,) + (res if isinstance(res, tuple) else (res,))

    def cover(self, targets: Sequence[Sound], piece_penalty: float = 0.0, gap_cost=None) -> List["Cover"]:
        """Every target tiled by dictionary sounds, the cut points and the sounds chosen together on the GPU so that the
        paced alignment costs of the pieces sum to the least total (ssym_dtw_cover, one call; dtw engines without a band):
        a partition of the target that has seen the dictionary.  piece_penalty >= 0 is added per piece and trades total
        fit for fewer, longer pieces; 0 is the plain optimum.  Every piece's cost is what align(step="paced") gives for
        (its sound, its frames of the target).  A target without a cover gives an empty Cover.
        gap_cost (None: no gaps, everything above as it is): target frames may stay uncovered at gap_cost >= 0 per frame
        (ssym_dtw_cover_gaps, "Cover with gaps") -- the price is a cost per frame, so it says how bad a Piece's
        cost_per_frame may get before silence is better.  The Cover then holds Gaps (maximal runs) among its Pieces; every
        target with a frame has a cover, and a NaN or infinite frame costs one gap frame, not the whole target.
        float("inf") gives the Covers of None."""
        penalty, gap = _cover_penalty(piece_penalty), _cover_gap_cost(gap_cost)
        targets = list(targets)
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        if getattr(self.engine, "metric", None) != "dtw":
            raise SsymError(SSYM_E_UNSUPPORTED, "cover aligns with dtw: a refcos engine has no alignment")
        if not targets:
            return []
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        q = self.engine.queries(flat, off, self._dim())
        try:
            count, total, src, start, end, cost = self.engine.dtw_cover(self.resident(), q, penalty, gap_cost=gap)
        finally:
            q.close()
        off = np.asarray(off, dtype=np.int64)
        out = []
        for t in range(len(targets)):
            a, frames = int(off[t]), int(off[t + 1] - off[t])
            if not count[t]:
                out.append(Cover.none(frames))
                continue
            b = a + int(count[t])
            out.append(Cover(_cover_tiles(src[a:b], start[a:b], end[a:b], cost[a:b]), total[t], frames))
        return out

    def mosaic(self, targets: Sequence[Sound], piece_penalty: float = 0.0, gap_cost=None) -> List["Mosaic"]:
        """Every target tiled by free spans of the dictionary's sounds, the cuts, the sounds, the spans and the paced paths
        chosen together on the GPU for the least total (ssym_dtw_mosaic, one call; dtw engines without a band): neither
        the targets nor the dictionary's recordings need cutting beforehand, and a recording may be of any length.
        piece_penalty >= 0 is charged once per piece and trades total fit for fewer, longer pieces; at 0 the optimum is
        frame-wise (a stretched span comes back in fragments), so ask with a penalty > 0.  gap_cost (None: no gaps):
        target frames may stay uncovered at gap_cost >= 0 per frame; the Mosaic then holds Gaps among its MosaicPieces,
        every target with a frame has a mosaic, and a NaN frame costs one gap frame, not the whole target."""
        penalty, gap = self._cover_checks(piece_penalty, "mosaic"), _cover_gap_cost(gap_cost)
        targets = list(targets)
        if not targets:
            return []
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        q = self.engine.queries(flat, off, self._dim())
        try:
            arrays = self.engine.dtw_mosaic(self.resident(), q, penalty, gap)
        finally:
            q.close()
        return _mosaics(off, *arrays)

    def reconstruct_mosaic(self, target: Sound, piece_penalty: float = 0.0, gap_cost=None, gap_fill: str = "silence",
                           search: int = 0, want_pcm32: bool = False, mosaic: Optional["Mosaic"] = None, dynamics=None,
                           max_gain: float = FOLLOW_MAX_GAIN):
        """mosaic, then warp: every sounding piece of the target's Mosaic is resynthesised from its span of its recording
        along its frame_map, in ONE call of the existing window reconstruction (ssym_reconstruct_warped_spans, or with
        search > 0 ssym_reconstruct_wsola_spans): the window is the piece's source_sample_span, the map frame_map -
        source_first, the output length the piece's entry of Mosaic.segment_lengths.  Gaps' stretches are spliced in as
        zeros (gap_fill="silence") or as the target's own samples ("target"), as reconstruct_covered does.  Returns
        (mosaic, samples), with want_pcm32 (mosaic, samples, pcm); the samples are len(target.samples()); a target
        without a mosaic gives silence.  mosaic (default None: computed here): a Mosaic of the target made elsewhere --
        by mosaic_long, or a LiveMosaic's mosaics() -- is resynthesised as it is; piece_penalty and gap_cost are then not
        used.  dynamics="target": the spliced samples, gaps included, go through one Engine.follow_envelope call against
        the target's samples (max_gain as there), so the pieces take the target's loudness and a gap_fill="target" stretch
        meets a gain of 1 from two hops inside its ends; None: this method as it was."""
        penalty, gap = _cover_penalty(piece_penalty), _cover_gap_cost(gap_cost)
        gain = follow_dynamics(dynamics, max_gain)
        search = _wsola_search(search)
        if gap_fill not in ("silence", "target"):
            raise ValueError('gap_fill must be "silence" or "target"')
        if not isinstance(target, Sound):
            raise ValueError("reconstruct_mosaic takes one Sound")
        if mosaic is None:
            mosaic = self.mosaic([target], penalty, gap)[0]
        elif not isinstance(mosaic, Mosaic):
            raise ValueError("mosaic must be a Mosaic")
        smp = np.asarray(target.samples(), dtype=np.float64)
        outs = [np.zeros(smp.size), np.zeros(smp.size, dtype=np.int32)][:2 if want_pcm32 else 1]
        lengths = mosaic.segment_lengths(smp.size)
        sounding = [(p, n) for p, n in zip(mosaic.pieces, lengths) if not p.is_gap]
        if sounding:
            idx = np.array([p.source_index for p, _ in sounding], dtype=np.uint32)
            spans = [p.source_sample_span(self.sounds[p.source_index].samples().size) for p, _ in sounding]
            w_first = np.array([a for a, _ in spans], dtype=np.uint64)
            w_len = np.array([max(a, b) - a for a, b in spans], dtype=np.uint64)
            out_off = np.concatenate([[0], np.cumsum([n for _, n in sounding])]).astype(np.uint64)
            frames = np.array([p.num_frames() for p, _ in sounding], dtype=np.uint32)
            m_off = np.concatenate([[0], np.cumsum(frames)]).astype(np.uint64)
            maps = np.concatenate([p.frame_map - p.source_first for p, _ in sounding]).astype(np.uint32)
            if search:
                res = self.engine.reconstruct_wsola(self.resident_samples(), idx, out_off, maps, m_off, frames, None, search,
                                                    want_pcm32, windows=(w_first, w_len))
            else:
                res = self.engine.reconstruct_warped(self.resident_samples(), idx, out_off, maps, m_off, frames, None,
                                                     want_pcm32, windows=(w_first, w_len))
            warped = res if isinstance(res, tuple) else (res,)
        at = took = 0
        for p, n in zip(mosaic.pieces, lengths):
            if not p.is_gap:
                for o, w in zip(outs, warped):
                    o[at:at + n] = w[took:took + n]
                took += n
            elif gap_fill == "target":
                outs[0][at:at + n] = smp[at:at + n]
                if want_pcm32:
                    with np.errstate(invalid="ignore", over="ignore"):
                        x = np.nan_to_num(2147483647.0 * smp[at:at + n], nan=0.0)
                        outs[1][at:at + n] = np.trunc(np.clip(x, -2147483648.0, 2147483647.0)).astype(np.int64).astype(np.int32)
            at += n
        if gain is not None:
            outs = _follow_targets(self.engine, tuple(outs), [target], gain, want_pcm32)
        return (mosaic,) + tuple(outs)

    def _cover_checks(self, piece_penalty, what: str) -> float:
        penalty = _cover_penalty(piece_penalty)
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        if getattr(self.engine, "metric", None) != "dtw":
            raise SsymError(SSYM_E_UNSUPPORTED, what + " aligns with dtw: a refcos engine has no alignment")
        return penalty

    def cover_live(self, sounds: Sequence[Sound], piece_penalty: float = 0.0, gap_cost=None) -> "LiveCover":
        """Cover Sounds that are still growing (fed with push_samples / push_sounds): a Coverer on this dictionary follows
        the sounds' stream (ssym_coverer_*, DESIGN.md section 2 "Live cover"; dtw engines without a band).  The sounds must
        be resident and share one stream, sound i in lane i -- what one push_sounds(sounds, ...) leaves -- ValueError
        otherwise, before any device work.  LiveCover.poll() returns the pieces no longer recording can change,
        flush() the rest; on f64 engines the pieces from first poll to flush are `cover`'s, bit for bit.  On f32 engines
        `cover` rounds the targets' features to f32 first while the coverer reads the stream's f64 frames as they are (as
        `watch` does), so the two can differ there.  The LiveCover keeps the dictionary's resident copy: close it before
        the dictionary changes.  gap_cost as for `cover` (ssym_coverer_create_gaps): a NaN or infinite frame then becomes
        a gap frame and the sound goes on being covered; covers() after flush are cover(gap_cost=)'s."""
        penalty, gap = self._cover_checks(piece_penalty, "cover_live"), _cover_gap_cost(gap_cost)
        sounds = list(sounds)
        st = _shared_stream(sounds, "cover_live")
        if self.engine is not st.engine:
            raise ValueError("cover_live: the dictionary's engine must be the one that holds the sounds' stream")
        if st.ncoeffs != self._dim():
            raise ValueError("cover_live: the sounds' ncoeffs must be the dictionary's")
        return LiveCover(sounds, st, self.engine.coverer(self.resident(), len(sounds), penalty, gap), penalty, gap)

    def mosaic_live(self, sounds: Sequence[Sound], piece_penalty: float = 0.0, gap_cost=None, audio: bool = False,
                    search: int = 0, gap_fill: str = "silence", dynamics=None, max_gain: float = FOLLOW_MAX_GAIN) -> "LiveMosaic":
        """Tile Sounds that are still growing (fed with push_samples / push_sounds): a Mosaicker on this dictionary follows
        the sounds' stream (ssym_mosaicker_*, DESIGN.md section 2 "Live mosaic"; dtw engines without a band).  The sounds
        must be resident and share one stream, sound i in lane i -- what one push_sounds(sounds, ...) leaves -- ValueError
        otherwise, before any device work.  LiveMosaic.poll() returns the pieces no longer recording can change, flush()
        the rest; on f64 engines the mosaics() after flush are `mosaic`'s, bit for bit.  On f32 engines `mosaic` rounds
        the targets' features to f32 first while the mosaicker reads the stream's f64 frames as they are (as `watch`
        does), so the two can differ there.  The LiveMosaic keeps the dictionary's resident copy: close it before the
        dictionary changes.  gap_cost as for `mosaic`: a NaN frame then becomes a gap frame and the sound goes on.
        audio=True: the LiveMosaic also owns a Resynth on the dictionary's resident samples (ssym_resynth_*, "Live
        resynthesis"): every poll hands it the committed frames device to device, and LiveMosaic.audio() returns the samples
        that releases -- from the first poll to flush reconstruct_mosaic's (search and gap_fill as there), bit for bit.
        With audio=False (the default) search and gap_fill are not used.
        dynamics="target" (with audio=True): the LiveMosaic also owns a Follower (ssym_follower_*, "Live envelope
        following"): audio() feeds it what the resynthesiser released -- after the gap splice, as reconstruct_mosaic follows
        after its splice -- beside the sound's own samples, and returns what that releases: from the first poll to flush
        reconstruct_mosaic(..., dynamics="target", max_gain=)'s, bit for bit.  None: everything as it was, no follower."""
        gain = follow_dynamics(dynamics, max_gain)
        if gain is not None and not audio:
            raise ValueError('dynamics="target" follows the audio: it needs audio=True')
        penalty, gap = self._cover_checks(piece_penalty, "mosaic_live"), _cover_gap_cost(gap_cost)
        if audio:
            search = _wsola_search(search)
            if gap_fill not in ("silence", "target"):
                raise ValueError('gap_fill must be "silence" or "target"')
        sounds = list(sounds)
        st = _shared_stream(sounds, "mosaic_live")
        if self.engine is not st.engine:
            raise ValueError("mosaic_live: the dictionary's engine must be the one that holds the sounds' stream")
        if st.ncoeffs != self._dim():
            raise ValueError("mosaic_live: the sounds' ncoeffs must be the dictionary's")
        mk = self.engine.mosaicker(self.resident(), len(sounds), penalty, gap)
        if not audio:
            return LiveMosaic(sounds, st, mk, penalty, gap)
        try:
            rs = self.engine.resynth(self.resident_samples(), len(sounds), search)
        except Exception:
            mk.close()
            raise
        fl = None
        if gain is not None:
            try:
                fl = self.engine.follower(len(sounds), gain)
            except Exception:
                rs.close()
                mk.close()
                raise
        return LiveMosaic(sounds, st, mk, penalty, gap, rs, gap_fill, fl)

    def mosaic_long(self, target: Sound, piece_penalty: float = 0.0, block_frames: int = 4096, gap_cost=None) -> "Mosaic":
        """`mosaic` for one target of any length: a one-lane Mosaicker is pushed the target's frames block_frames at a time
        and flushed, so the tables hold the uncommitted columns alone, not one byte per (source frame, target frame).  The
        Mosaic is `mosaic`'s, bit for bit, where `mosaic` takes the target (on f32 engines the features are rounded to f32
        first, as `mosaic` does).  gap_cost as for `mosaic`."""
        penalty, gap = self._cover_checks(piece_penalty, "mosaic_long"), _cover_gap_cost(gap_cost)
        if isinstance(target, (list, tuple)):
            raise ValueError("mosaic_long takes one Sound")
        block = int(block_frames)
        if block < 1 or block != block_frames:
            raise ValueError("block_frames must be a whole number of frames, at least 1")
        rows = np.asarray(target.mfcc_arrays(), dtype=self.engine.np_dtype).astype(np.float64)
        if rows.shape[1:] != (self._dim(),):
            raise ValueError("mosaic_long: the target's ncoeffs must be the dictionary's")
        frames = rows.shape[0]
        mk = self.engine.mosaicker(self.resident(), 1, penalty, gap)
        try:
            parts = []
            for at in range(0, frames, block):
                if mk.push(rows[at:at + block]):
                    parts.append(mk.frames()[2:])
            total = float(mk.best()[0][0])
            if mk.flush(0):
                parts.append(mk.frames()[2:])
        finally:
            mk.close()
        if not np.isfinite(total):
            return Mosaic.none(frames)
        src, frame, cost, start = (np.concatenate(x) for x in zip(*parts))
        return Mosaic(_mosaic_tiles(np.flatnonzero(start), src, frame, cost), total, frames, cost)

    def cover_long(self, target: Sound, piece_penalty: float = 0.0, block_frames: int = 4096, gap_cost=None) -> "Cover":
        """`cover` for one target of any length: a one-lane Coverer is pushed the target's frames block_frames at a time
        and flushed, so the tables never hold more than a block and the dictionary's horizon.  The Cover is `cover`'s, bit
        for bit, where `cover` takes the target (on f32 engines the features are rounded to f32 first, as `cover` does).
        gap_cost as for `cover`."""
        penalty, gap = self._cover_checks(piece_penalty, "cover_long"), _cover_gap_cost(gap_cost)
        if isinstance(target, (list, tuple)):
            raise ValueError("cover_long takes one Sound")
        block = int(block_frames)
        if block < 1 or block != block_frames:
            raise ValueError("block_frames must be a whole number of frames, at least 1")
        rows = np.asarray(target.mfcc_arrays(), dtype=self.engine.np_dtype).astype(np.float64)
        if rows.shape[1:] != (self._dim(),):
            raise ValueError("cover_long: the target's ncoeffs must be the dictionary's")
        frames = rows.shape[0]
        cv = self.engine.coverer(self.resident(), 1, penalty, gap)
        try:
            raw = []

            def take():
                _, src, start, end, cost = cv.pieces()
                raw.extend((src[k], start[k], end[k], cost[k]) for k in range(src.size))
            for at in range(0, frames, block):
                if cv.push(rows[at:at + block]):
                    take()
            total = float(cv.best()[0][0])
            if cv.flush(0):
                take()
        finally:
            cv.close()
        return Cover(_cover_tiles(*zip(*raw)) if raw else [], total, frames) if np.isfinite(total) else Cover.none(frames)

    def reconstruct_covered(self, target: Sound, piece_penalty: float = 0.0, search: int = 0, want_pcm32: bool = False,
                            gap_cost=None, gap_fill: str = "silence", dynamics=None, max_gain: float = FOLLOW_MAX_GAIN):
        """cover, cut, warp: the target is covered (ssym_dtw_cover), cut at the pieces (samples by
        Cover.segment_lengths, MFCC rows start_frame ... end_frame) and every piece warped from its sound under the paced
        pattern -- self.warp(pieces, indices=cover.indices(), step="paced", search=search), the existing calls.  Returns
        (cover, samples), with want_pcm32 (cover, samples, pcm); the samples are len(target.samples()).  A target without
        a cover takes what SoundSequence([target]).reconstruct_from_dictionary gives it whole.
        gap_cost as for `cover`.  The sounding pieces then go through warp exactly as above, and every Gap's stretch of
        samples (its entry of Cover.segment_lengths: Gap.sample_span, a gap that ends the target running to the sound's last
        sample) is spliced in between them as zeros (gap_fill="silence") or as the target's own samples ("target"; their
        32-bit conversion is warp's: truncated, saturated, NaN as 0).  dynamics="target": the samples, after the splice,
        go through one Engine.follow_envelope call against the whole target's samples (max_gain as there); None: this
        method as it was."""
        penalty, gap = _cover_penalty(piece_penalty), _cover_gap_cost(gap_cost)
        gain = follow_dynamics(dynamics, max_gain)
        search = _wsola_search(search)
        if gap_fill not in ("silence", "target"):
            raise ValueError('gap_fill must be "silence" or "target"')
        if not isinstance(target, Sound):
            raise ValueError("reconstruct_covered takes one Sound")
        cover = self.cover([target], penalty, gap)[0]
        if not cover:
            res = SoundSequence([target]).reconstruct_from_dictionary(self, want_pcm32)
        elif not cover.gaps:
            res = self.warp(_cover_sounds(target, cover), cover.indices(), want_pcm32, search, step="paced")
        else:
            res = self._splice_gaps(target, cover, gap_fill, want_pcm32, search)
        if gain is not None:
            res = _follow_targets(self.engine, res, [target], gain, want_pcm32)
        return (cover,) + (res if isinstance(res, tuple) else (res,))

    def _splice_gaps(self, target: Sound, cover: "Cover", gap_fill: str, want_pcm32: bool, search: int):
        """reconstruct_covered for a cover with gaps: warp's samples of the sounding pieces, the gaps' stretches between
        them."""
        smp = np.asarray(target.samples(), dtype=np.float64)
        res = self.warp(_cover_sounds(target, cover), cover.indices(), want_pcm32, search, step="paced")
        warped = res if isinstance(res, tuple) else (res,)
        outs = [np.zeros(smp.size), np.zeros(smp.size, dtype=np.int32)][:len(warped)]
        at = took = 0
        for p, n in zip(cover.pieces, cover.segment_lengths(smp.size)):
            if not p.is_gap:
                for o, w in zip(outs, warped):
                    o[at:at + n] = w[took:took + n]
                took += n
            elif gap_fill == "target":
                outs[0][at:at + n] = smp[at:at + n]
                if want_pcm32:
                    with np.errstate(invalid="ignore", over="ignore"):
                        x = np.nan_to_num(2147483647.0 * smp[at:at + n], nan=0.0)
                        outs[1][at:at + n] = np.trunc(np.clip(x, -2147483648.0, 2147483647.0)).astype(np.int64).astype(np.int32)
            at += n
        return tuple(outs) if want_pcm32 else outs[0]

    def spot(self, targets: Sequence[Sound], indices=None, step: str = "symmetric") -> List["Spot"]:
        """Where inside the dictionary's (unsegmented) recordings every target sounds: subsequence DTW on the GPU (dtw
        engines without a band).  indices=None: every recording is tried for every target and the best one kept, the
        lower index on a tie -- one ssym_spot_queries call; otherwise indices[t] names the recording target t is
        spotted in (ssym_dtw_spot).  A target without a spot gives an empty Spot.  step="paced": the paced step pattern
        (the _step calls with SSYM_STEP_PACED): spans of about half to twice the target's frames, and Spot.cost_per_frame
        set."""
        _spot_step(step)
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        if getattr(self.engine, "metric", None) != "dtw":
            raise SsymError(SSYM_E_UNSUPPORTED, "spot aligns with dtw: a refcos engine has no alignment")
        targets = list(targets)
        if indices is not None:
            indices = np.asarray(indices, dtype=np.int64).reshape(-1)
            if indices.size != len(targets):
                raise ValueError("indices must name one dictionary sound per target")
            if indices.size and (indices.min() < 0 or indices.max() >= len(self.sounds)):
                raise ValueError("an index is outside the dictionary")
        if not targets:
            return []
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        q = self.engine.queries(flat, off, self._dim())
        try:
            if indices is None:
                indices, cost, start, end = self.engine.spot_queries(self.resident(), q, **_step_kw(step))
            else:
                cost, start, end = self.engine.dtw_spot(self.resident(), q, indices, **_step_kw(step))
        finally:
            q.close()
        frames = np.diff(off.astype(np.int64))
        return [Spot(int(indices[t]), int(start[t]), int(end[t]), cost[t], _per_frame(step, cost[t], frames[t]))
                if int(end[t]) != NO_MATCH else Spot.none() for t in range(len(targets))]

    def spot_all(self, targets: Sequence[Sound], indices=None, max_spots: int = 8, max_cost=None, step: str = "symmetric",
                 max_cost_per_frame=None) -> List[List["Spot"]]:
        """Every place a target sounds inside the dictionary's recordings: per target its occurrences by ascending cost,
        pairwise disjoint within a recording (ssym_dtw_spot_all, one call; dtw engines without a band).  With indices,
        target t is searched in recording indices[t] and max_cost is a scalar or one value per target; without, in every
        recording -- max_spots then applies per recording, max_cost is a scalar, and a target's list is merged by
        (cost, source index, end).  An occurrence costs at most max_cost; the cost is not normalised by any length, so
        without max_cost the list goes on with spans the target merely fits least badly.  step="paced": the paced step
        pattern (ssym_dtw_spot_all_step with SSYM_STEP_PACED), Spot.cost_per_frame set, and max_cost_per_frame (instead
        of max_cost; a scalar, or with indices one value per target) is a threshold on that mean: target t's occurrences
        cost at most max_cost_per_frame * its frames, so one value serves targets of every length."""
        _spot_step(step)
        if max_cost_per_frame is not None:
            if max_cost is not None:
                raise ValueError("max_cost and max_cost_per_frame exclude each other")
            if step != "paced":
                raise ValueError('max_cost_per_frame needs step="paced": only there is cost / frames a mean per-frame distance')
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        if getattr(self.engine, "metric", None) != "dtw":
            raise SsymError(SSYM_E_UNSUPPORTED, "spot_all aligns with dtw: a refcos engine has no alignment")
        targets = list(targets)
        if not 1 <= int(max_spots) <= 64:
            raise ValueError("max_spots must be 1 ... 64")
        n, m = len(self.sounds), len(targets)
        if max_cost is not None:
            max_cost = np.asarray(max_cost, dtype=np.float64)
            if max_cost.ndim and (indices is None or max_cost.size != m):
                raise ValueError("max_cost must be a scalar, or with indices one value per target")
            if np.isnan(max_cost).any():
                raise ValueError("max_cost must not be NaN")
        if max_cost_per_frame is not None:
            max_cost_per_frame = np.asarray(max_cost_per_frame, dtype=np.float64)
            if max_cost_per_frame.ndim and (indices is None or max_cost_per_frame.size != m):
                raise ValueError("max_cost_per_frame must be a scalar, or with indices one value per target")
            if np.isnan(max_cost_per_frame).any():
                raise ValueError("max_cost_per_frame must not be NaN")
        if indices is not None:
            indices = np.asarray(indices, dtype=np.int64).reshape(-1)
            if indices.size != m:
                raise ValueError("indices must name one dictionary sound per target")
            if indices.size and (indices.min() < 0 or indices.max() >= n):
                raise ValueError("an index is outside the dictionary")
        if not targets:
            return []
        if indices is None:
            src, tgt = np.repeat(np.arange(n), m), np.tile(np.arange(m), n)
        else:
            src, tgt = indices, np.arange(m)
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        frames = np.diff(off.astype(np.int64))
        if max_cost_per_frame is not None:
            # a sum per pair, in f64 on the host: max_cost[p] = x * Fb[p]
            max_cost = np.broadcast_to(max_cost_per_frame.reshape(-1), (m,))[tgt] * frames[tgt].astype(np.float64)
        q = self.engine.queries(flat, off, self._dim())
        try:
            count, cost, start, end = self.engine.dtw_spot_all(self.resident(), q, src, tgt, max_spots=int(max_spots),
                                                               max_cost=max_cost, **_step_kw(step))
        finally:
            q.close()
        out: List[List[Spot]] = [[] for _ in range(m)]
        for p in range(src.size):
            out[int(tgt[p])] += [Spot(int(src[p]), int(start[p, k]), int(end[p, k]), cost[p, k],
                                      _per_frame(step, cost[p, k], frames[int(tgt[p])])) for k in range(int(count[p]))]
        for spots in out:
            spots.sort(key=lambda sp: (sp.cost, sp.source_index, sp.end_frame))
        return out

    def cut(self, spots: Sequence["Spot"]) -> "SoundDictionary":
        """A dictionary with one Sound per spot: the recording's samples over spot.sample_span() and its feature frames
        start_frame ... end_frame; an empty spot gives an empty Sound.  Sound t of the result is what target t was
        spotted as, so align, warp and reconstruct_from_dictionary take it with indices = arange(len(spots))."""
        out = SoundDictionary(self._engine)
        for sp in spots:
            if not sp:
                ref = self.sounds[0] if self.sounds else None
                out.sounds.append(Sound(np.zeros(0), ref.sample_rate() if ref else 44100.0, np.zeros(0), None,
                                        ref.ncoeffs if ref else NCOEFFS))
                continue
            if not 0 <= sp.source_index < len(self.sounds):
                raise ValueError("a spot names a sound outside the dictionary")
            s = self.sounds[sp.source_index]
            if sp.end_frame >= s.num_frames():
                raise ValueError("a spot ends beyond its sound's frames")
            a, b = sp.sample_span(s.samples().size)
            feats = s.mfcc_arrays()[sp.start_frame:sp.end_frame + 1]
            out.sounds.append(Sound(s.samples()[a:b].copy(), s.sample_rate(), feats.reshape(-1).copy(), s.name, s.ncoeffs))
        return out

    def candidates(self, targets: Sequence[Sound], k: int, distances=None) -> List[List[Sound]]:
        """The k best dictionary sounds per target, best first: what k
        successive at_distance calls (src/sound.rs:351) would return if each winner were removed."""
        if not self.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")
        flat, off = pack_segments([t.mfccs() for t in targets], self._dim(), self.engine.np_dtype)
        q = self.engine.queries(flat, off, self._dim())
        idx, _ = self.engine.match_topk(self.resident(), q, k, distances)
        q.close()
        return [[self.sounds[int(i)] for i in row if int(i) != NO_MATCH] for row in idx]


def length_fit(matched: np.ndarray, n_target: int) -> np.ndarray:
    """src/sound.rs:456-465: zero-pad the matched samples up to the target's sample count, or
    truncate them down to it."""
    out = np.zeros(n_target, dtype=np.float64)
    n = min(matched.size, n_target)
    out[:n] = matched[:n]
    return out


class SoundSequence:
    """Sequence of sounds (src/sound.rs:375-484).  The reference stores the angular distances between neighbours when
    the sequence is built (SoundSequence::new, :392-398); here `sounds()` is a mutable list, so `distances()` computes
    them from the current sounds on every call, on the GPU (ssym_sequence_distances).  Sounds without features (the
    length-fitted sounds of clone_from_dictionary, to_sound()) are analysed for it as the reference re-analyses them
    (:457-462), in one ssym_mfcc_batch per sample rate, and nothing is stored on the Sound."""

    def __init__(self, sounds: Sequence[Sound]):
        self._sounds = list(sounds)

    @staticmethod
    def new(sounds: Sequence[Sound]) -> "SoundSequence":                # src/sound.rs:392
        return SoundSequence(sounds)

    def sounds(self) -> List[Sound]:                                    # src/sound.rs:432
        return self._sounds

    def distances(self, engine: Optional[Engine] = None) -> np.ndarray:  # src/sound.rs:436 (values: :392-398)
        """cosine_sim_angular of the mean MFCCs of each pair of neighbouring sounds: len(sounds) - 1 values, NaN
        next to a sound without frames (its mean is 0 / 0).  Mixed ncoeffs raise ValueError before any device work."""
        sounds = list(self._sounds)
        if len(sounds) < 2:
            return np.zeros(0)
        dims = {s.ncoeffs for s in sounds}
        if len(dims) != 1:
            raise ValueError(f"distances: the sounds carry different ncoeffs {sorted(dims)}")
        dim = dims.pop()
        e = engine or default_engine()
        feats = [s.mfccs() if s.has_mfccs() else None for s in sounds]
        missing = [i for i, f in enumerate(feats) if f is None]
        for rate in dict.fromkeys(sounds[i].sample_rate() for i in missing):
            which = [i for i in missing if sounds[i].sample_rate() == rate]
            for i, m in zip(which, analyze_mfccs([sounds[i].samples() for i in which], rate, dim, e)):
                feats[i] = m
        flat, off = pack_segments(feats, dim)
        return e.sequence_distances(flat, off, dim)

    @staticmethod
    def from_timestamps(sound: Sound, timestamps, engine: Optional[Engine] = None) -> "SoundSequence":
        """SoundSequence::from_timestamps (src/sound.rs:419-430): one Sound per (start s, end s, label),
        samples [round(start * rate), round(end * rate)] INCLUSIVE (:422-424), features analysed.  The cast is Rust's
        saturating one: a negative or NaN time reads as sample 0 and the call proceeds; only an end beyond the sound
        (or a start beyond the end) fails, where the reference's slice panics."""
        cuts = []
        smp, rate = sound.samples(), sound.sample_rate()
        for start, end, label in timestamps:
            a, b = _round_as_usize(start * rate), _round_as_usize(end * rate)        # `.round() as usize`, :422-423
            if b + 1 > smp.size or a > b + 1:
                # the reference slices `samples[start_sample..end_sample + 1]` (:424) and panics out of range
                raise IndexError(f"timestamp ({start}, {end}) -> samples [{a}, {b}] outside the sound's {smp.size} samples")
            cuts.append((smp[a:b + 1].copy(), label))
        # every sound's features in one ssym_mfcc_batch (Sound.from_samples' framing, bit for bit)
        feats = analyze_mfccs([c[0] for c in cuts], rate, sound.ncoeffs, engine)
        return SoundSequence([Sound(c[0], rate, m, c[1], sound.ncoeffs) for c, m in zip(cuts, feats)])

    @staticmethod
    def from_cover(sound: Sound, cover: "Cover") -> "SoundSequence":
        """The target as the sequence of its pieces: `sound` cut at the pieces of `cover` (SoundDictionary.cover), samples
        by Cover.segment_lengths and MFCC rows start_frame ... end_frame, so that align, warp and clone_from_dictionary
        take the pieces as they are.  An empty cover gives an empty sequence.  Gaps are skipped."""
        return SoundSequence(_cover_sounds(sound, cover))

    @staticmethod
    def from_distances(distances: Sequence[float], start: Sound,
                       dict_: SoundDictionary) -> "SoundSequence":      # src/sound.rs:405-417
        """Greedy chain: each step's query is the previous result.  The steps run on the device
        back to back (ssym_chain): one call, one wait."""
        if not len(distances):
            return SoundSequence([start])
        if not dict_.sounds:
            raise EmptyDictionaryError(-2, "empty dictionary")          # reference: panic, :369
        idx, _ = dict_.engine.chain(dict_.resident(), start.mfccs(), distances)
        return SoundSequence([start] + [dict_.sounds[int(i)] for i in idx])

    def morph_to(self, distances: Sequence[float], dict_: SoundDictionary, step: str = "symmetric",
                 per_frame: bool = False) -> "SoundSequence":
        """src/sound.rs:440-449: zip(sounds, distances) -> at_distance, here as ONE batch.  step="paced", per_frame: as for
        SoundDictionary.match_indices -- with both, a distance is a mean per frame and means the same for every sound."""
        _spot_step(step)
        if per_frame and step != "paced":
            raise ValueError('per_frame needs step="paced": only there is cost / frames a mean per-frame distance')
        n = min(len(self._sounds), len(distances))
        if n == 0:
            return SoundSequence([])
        kw = dict(_step_kw(step), **({"per_frame": True} if per_frame else {}))
        idx, _ = dict_.match_indices(self._sounds[:n], np.asarray(distances[:n], dtype=np.float64), **kw)
        return SoundSequence([dict_.sounds[int(i)] for i in idx])

    def clone_from_dictionary(self, dict_: SoundDictionary, step: str = "symmetric") -> "SoundSequence":
        """src/sound.rs:451-472: match every sound, then fit the match to the target's length.  step="paced": the match
        is SoundDictionary.match_indices(step="paced")'s."""
        _spot_step(step)
        if not self._sounds:
            return SoundSequence([])
        idx, _ = dict_.match_indices(self._sounds, None, **_step_kw(step))
        out = []
        for sound, i in zip(self._sounds, idx):
            s = dict_.sounds[int(i)]
            diff = sound.samples().size - s.samples().size
            if diff == 0:
                out.append(s)                                            # :463-464 shares the Arc
            else:
                # :457-462 builds a new Sound from the fitted samples and re-analyses it; here the
                # fitted Sound carries no features and distances() analyses it when asked
                out.append(Sound(length_fit(s.samples(), sound.samples().size), sound.sample_rate(),
                                 None, None, s.ncoeffs))
        return SoundSequence(out)

    def align_to_dictionary(self, dict_: SoundDictionary, step: str = "symmetric", match_step=None) -> List[Alignment]:
        """Every sound of the sequence matched against dict_ and aligned with its match (SoundDictionary.align)."""
        _spot_step(step)
        match_kw = {} if match_step is None else {"match_step": match_step}
        _match_kw(step, match_step)
        if not self._sounds:
            return []
        return dict_.align(self._sounds, **_step_kw(step), **match_kw)

    def spot_in_dictionary(self, dict_: SoundDictionary, step: str = "symmetric") -> List[Spot]:
        """Every sound of the sequence located inside dict_'s recordings (SoundDictionary.spot)."""
        if not self._sounds:
            return []
        return dict_.spot(self._sounds, **_step_kw(step))

    def spot_all_in_dictionary(self, dict_: SoundDictionary, max_spots: int = 8, max_cost=None, step: str = "symmetric",
                               max_cost_per_frame=None) -> List[List[Spot]]:
        """Every occurrence of every sound of the sequence inside dict_'s recordings (SoundDictionary.spot_all)."""
        if not self._sounds:
            return []
        return dict_.spot_all(self._sounds, max_spots=max_spots, max_cost=max_cost, **_step_kw(step, max_cost_per_frame))

    def reconstruct_from_dictionary(self, dict_: "SoundDictionary", want_pcm32: bool = False, dynamics=None,
                                    max_gain: float = FOLLOW_MAX_GAIN):
        """clone_from_dictionary(dict).to_sound().samples() in one go (src/sound.rs:451-480): match
        on the GPU, then gather / length-fit / concatenate on the GPU (ssym_reconstruct), optionally
        with write_file's 32-bit conversion (:139).  dynamics="target": the result goes through one
        Engine.follow_envelope call against this sequence's sounds (max_gain as there); None: this method as it was."""
        gain = follow_dynamics(dynamics, max_gain)
        if not self._sounds:
            return (np.zeros(0), np.zeros(0, dtype=np.int32)) if want_pcm32 else np.zeros(0)
        idx, _ = dict_.match_indices(self._sounds, None)
        lens = np.array([s.samples().size for s in self._sounds], dtype=np.uint64)
        out_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        res = dict_.engine.reconstruct(dict_.resident_samples(), idx, out_off, want_pcm32)
        return res if gain is None else _follow_targets(dict_.engine, res, self._sounds, gain, want_pcm32)

    def reconstruct_warped_from_dictionary(self, dict_: "SoundDictionary", want_pcm32: bool = False, search: int = 0,
                                           step: str = "symmetric", match_step=None, dynamics=None,
                                           max_gain: float = FOLLOW_MAX_GAIN):
        """reconstruct_from_dictionary with every match warped onto its target's timing instead of cut off or padded
        (SoundDictionary.warp: match, align, resynthesise along the alignment, all on the GPU; dtw engines).
        search > 0: with the waveform-similarity search of that width in samples (at most 512).  step and match_step as
        for SoundDictionary.warp, dynamics and max_gain too."""
        search = _wsola_search(search)
        follow_kw = {} if follow_dynamics(dynamics, max_gain) is None else {"dynamics": dynamics, "max_gain": max_gain}
        _spot_step(step)
        match_kw = {} if match_step is None else {"match_step": match_step}
        _match_kw(step, match_step)
        if not self._sounds:
            return (np.zeros(0), np.zeros(0, dtype=np.int32)) if want_pcm32 else np.zeros(0)
        return dict_.warp(self._sounds, None, want_pcm32, search, **_step_kw(step), **match_kw, **follow_kw)

    def reconstruct_spotted_from_dictionary(self, dict_: "SoundDictionary", step: str = "symmetric", search: int = 0,
                                            want_pcm32: bool = False, dynamics=None, max_gain: float = FOLLOW_MAX_GAIN):
        """dict_.reconstruct_spotted of this sequence's sounds: (spots, samples[, pcm]).  dynamics and max_gain as there."""
        follow_kw = {} if follow_dynamics(dynamics, max_gain) is None else {"dynamics": dynamics, "max_gain": max_gain}
        return dict_.reconstruct_spotted(self._sounds, step, search, want_pcm32, **follow_kw)

    def to_sound(self) -> Sound:                                        # src/sound.rs:475-483
        parts = [s.samples() for s in self._sounds]
        samples = np.concatenate(parts) if parts else np.zeros(0)
        rate = self._sounds[0].sample_rate() if self._sounds else 44100.0
        ncoeffs = self._sounds[0].ncoeffs if self._sounds else NCOEFFS
        return Sound(samples, rate, None, None, ncoeffs)


# ---- partitioner (src/lib.rs:32-151; DESIGN.md 5.8: own definitions, PARITY UNPINNED) ---------------------------------

def _data(data, ncoeffs: int) -> np.ndarray:
    x = np.ascontiguousarray(data, dtype=np.float64)
    return x.reshape(-1, ncoeffs) if x.ndim == 1 else x


def init_rows(n_rows: int, k: int = NCLUSTERS, seed=None) -> np.ndarray:
    """The starting means of a mixture: k distinct rows drawn by a seeded generator (the library itself draws
    nothing at random, so a model is a function of the data and these rows)."""
    if n_rows < k:
        raise ValueError(f"a mixture of {k} components needs at least {k} frames, got {n_rows}")
    return np.sort(np.random.default_rng(seed).choice(n_rows, size=k, replace=False)).astype(np.uint64)


def train_model(data, seed=None, engine: Optional[Engine] = None, max_iters: int = 5):
    """train_model (src/lib.rs:43-54): standardise, then a 26-component mixture, CovOption::Regularized(0.1),
    5 EM iterations, on the GPU (ssym_gmm_train).  data: [frames][ncoeffs] (or flat NCOEFFS-value frames)."""
    e = engine or default_engine()
    x = _data(data, NCOEFFS)
    return e.gmm_train(x, x.shape[1], init_rows(x.shape[0], NCLUSTERS, seed), GMM_EPS, max_iters, standardize=True)


def discretize_with_model(data, gmm, engine: Optional[Engine] = None) -> np.ndarray:
    """discretize_with_model (src/lib.rs:56-60): standardise with the data's own statistics, then the posteriors
    [frames][K] of the model."""
    e = engine or gmm.engine
    x = _data(data, gmm.dim)
    return e.gmm_predict(gmm, x, standardize=True, want_post=True)[1]


def discretize(data, seed=None, engine: Optional[Engine] = None) -> np.ndarray:
    """discretize (src/lib.rs:32-41): train with up to 1000 EM iterations, then the posteriors of the same data."""
    gmm = train_model(data, seed, engine, max_iters=1000)
    try:
        return discretize_with_model(data, gmm)
    finally:
        gmm.close()


class Partitioner:
    """Partitioner (src/lib.rs:67-151): cuts a sound into phoneme-like segments -- GMM letters per MFCC frame, then
    voting experts over the letter string.  `sound` may be reassigned (examples/reconstruction.rs:72)."""

    def __init__(self, sound: Sound, engine: Optional[Engine] = None):
        self.sound = sound
        self._depth = 5          # src/lib.rs:78-79
        self._threshold = 4
        self.model = None
        self._engine = engine

    @staticmethod
    def new(sound: Sound, engine: Optional[Engine] = None) -> "Partitioner":
        return Partitioner(sound, engine)

    @staticmethod
    def from_path(path, engine: Optional[Engine] = None) -> "Partitioner":
        return Partitioner(Sound.from_path(path, engine=engine), engine)

    def depth(self, n: Optional[int] = None):
        """Builder: depth(n) sets the depth of the n-gram trie and returns the partitioner; depth() reads it."""
        if n is None:
            return self._depth
        self._depth = int(n)
        return self

    def threshold(self, n: Optional[int] = None):
        """Builder: threshold(n) sets the votes a boundary needs and returns the partitioner; threshold() reads it."""
        if n is None:
            return self._threshold
        self._threshold = int(n)
        return self

    @property
    def engine(self) -> Engine:
        if self._engine is None:
            self._engine = default_engine()
        return self._engine

    def train(self, seed=None) -> None:
        """src/lib.rs:97-103: train_model on this partitioner's sound."""
        if self.model is not None:
            self.model.close()
        self.model = train_model(self.sound.mfccs().reshape(-1, self.sound.ncoeffs), seed, self.engine)

    def partition_other(self, sound: Sound) -> List[int]:
        """src/lib.rs:108-141: segment lengths in SAMPLES (frames x HOP) of `sound`, cut with this model; the frames
        are standardised with `sound`'s own statistics."""
        if self.model is None:
            raise RuntimeError("Must first train model")
        frames = self.engine.partition(self.model, sound.mfccs().reshape(-1, sound.ncoeffs), self._depth,
                                       self._threshold, standardize=True)
        return [int(f) * HOP for f in frames]

    def partition(self) -> List[int]:
        """src/lib.rs:145-147."""
        return self.partition_other(self.sound)
