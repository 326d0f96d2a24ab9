"""Array-level host interface over the C ABI: contexts, resident dictionaries / query sets, match.

Everything here forwards to ``libsoundsym_amd.so``; no arithmetic of the matching path happens in
Python.  Feature buffers may be numpy arrays (host) or torch CUDA tensors (device, handed over as
raw pointers -- torch is only the owner of the memory).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat


def pack_segments(segments: Sequence[np.ndarray], dim: int, dtype=np.float64):
    """List of per-segment arrays (frames_i x dim, or flat) -> (flat values, frame offsets)."""
    off = np.zeros(len(segments) + 1, dtype=np.uint64)
    for i, s in enumerate(segments):
        n = int(np.asarray(s).size)
        if n % dim:
            raise ValueError(f"segment {i}: {n} values is not a whole number of {dim}-dim frames")
        off[i + 1] = off[i] + np.uint64(n // dim)
    flat = np.zeros(int(off[-1]) * dim, dtype=dtype)
    for i, s in enumerate(segments):
        flat[int(off[i]) * dim:int(off[i + 1]) * dim] = np.asarray(s, dtype=dtype).reshape(-1)
    return flat, off


def _is_device_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _align_indices(src_idx, tgt_idx):
    """The pair list of dtw_align as contiguous uint32 arrays (tgt None: pair p uses target p)."""
    src = np.ascontiguousarray(src_idx, dtype=np.uint32).reshape(-1)
    tgt = None
    if tgt_idx is not None:
        tgt = np.ascontiguousarray(tgt_idx, dtype=np.uint32).reshape(-1)
        if tgt.size != src.size:
            raise ValueError("src_idx and tgt_idx must list the same number of pairs")
    return src, tgt


def _align_spans(spans, n):
    """spans=(first, last) of dtw_align as two contiguous uint32 arrays of n inclusive source frames, or None."""
    if spans is None:
        return None
    first, last = (np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in spans)
    if first.size != n or last.size != n:
        raise ValueError("spans must give one first and one last source frame per pair")
    return first, last


def _warp_windows(windows, n):
    """windows=(first, len) of reconstruct_warped / reconstruct_wsola as two contiguous uint64 arrays of n sample counts, or
    None."""
    if windows is None:
        return None
    first, length = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in windows)
    if first.size != n or length.size != n:
        raise ValueError("windows must give one first sample and one length per target")
    return first, length


def _spot_step(step):
    """SSYM_STEP_* of step="symmetric" | "paced", checked before the library is asked."""
    if step == "symmetric":
        return nat.STEP_SYMMETRIC
    if step == "paced":
        return nat.STEP_PACED
    raise ValueError('step must be "symmetric" or "paced"')


def _cover_penalty(piece_penalty) -> float:
    """piece_penalty of dtw_cover as a float, checked before the library is asked."""
    penalty = float(piece_penalty)
    if not 0.0 <= penalty < float("inf"):
        raise ValueError("piece_penalty must be finite and not negative")
    return penalty


def _cover_gap_cost(gap_cost):
    """gap_cost of dtw_cover / coverer: None (no gaps: the calls without the argument) or a float >= 0 (+inf allowed),
    checked before the library is asked."""
    if gap_cost is None:
        return None
    gap = float(gap_cost)
    if not gap >= 0.0:
        raise ValueError("gap_cost must not be negative or NaN (None or +inf: no gaps)")
    return gap


def _spot_all_args(src, max_spots, max_cost):
    """(K, per-pair thresholds as a contiguous f64 array or None) of dtw_spot_all, checked before the library is asked."""
    k = int(max_spots)
    if not 1 <= k <= 64:
        raise ValueError("max_spots must be 1 ... 64")
    if max_cost is None:
        return k, None
    mc = np.asarray(max_cost, dtype=np.float64)
    if mc.ndim == 0:
        mc = np.full(src.size, float(mc))
    mc = np.ascontiguousarray(mc.reshape(-1))
    if mc.size != src.size:
        raise ValueError("max_cost must be a scalar or one value per pair")
    if np.isnan(mc).any():
        raise ValueError("max_cost must not be NaN")
    return k, mc


def _output(device, shape, dtype):
    """One output array of a call as (array, address): a zeroed numpy array, or with a device number (SSYM_OUT_DEVICE) a
    torch tensor in that device's memory, float64 or -- for the call's u32 values -- int32.  The tensor has room for at
    least one row, so it has an address when shape[0] is 0; what is returned is its first shape[0] rows."""
    if device is None:
        x = np.zeros(shape, dtype=dtype)
        return x, x.ctypes.data
    import torch
    x = torch.empty((max(shape[0], 1),) + tuple(shape[1:]), dtype=torch.float64 if dtype == np.float64 else torch.int32,
                    device=torch.device("cuda", device))
    return x[:shape[0]], x.data_ptr()


def _device_words(x, what: str):
    """(pointer, count) of 32-bit words in device memory: a torch CUDA tensor of a 4-byte integer type, or a
    DeviceFrames-style object (data_ptr / numel) whose owner vouches for the content."""
    size = getattr(x, "element_size", None)
    if callable(size) and size() != 4:
        raise ValueError(f"{what}: a device tensor of 32-bit integers is needed")
    contiguous = getattr(x, "is_contiguous", None)
    if callable(contiguous) and not contiguous():
        raise ValueError(f"{what}: the device tensor must be contiguous")
    n = int(x.numel())
    return (int(x.data_ptr()) if n else None), n


def _warp_inputs(idx, out_offsets, maps, map_offsets, map_frames, pair_len):
    """The arguments of reconstruct_warped, checked on the host before anything reaches the device.  Returns (idx u32
    [n], out_offsets u64 [n + 1], map_offsets u64 [n + 1], map_frames u32 [n], map pointer, pair_len pointer, maps on
    the device?, objects to keep alive for the call)."""
    idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    n = idx.size
    off = np.ascontiguousarray(out_offsets, dtype=np.uint64).reshape(-1)
    m_off = np.ascontiguousarray(map_offsets, dtype=np.uint64).reshape(-1)
    frames = np.ascontiguousarray(map_frames, dtype=np.uint32).reshape(-1)
    if off.size != n + 1 or m_off.size != n + 1 or frames.size != n:
        raise ValueError("reconstruct_warped: n + 1 out_offsets, n + 1 map_offsets and n map_frames for n indices")
    if off[0] != 0 or np.any(off[1:] < off[:-1]):
        raise ValueError("reconstruct_warped: out_offsets must start at 0 and not decrease")
    if np.any(m_off[1:] < m_off[:-1]) or np.any(m_off[1:] - m_off[:-1] < frames):
        raise ValueError("reconstruct_warped: map_offsets must not decrease and must leave map_frames[t] entries per target")
    need = int(m_off[-1]) if frames.any() else 0
    device = _is_device_tensor(maps) or (maps is None and _is_device_tensor(pair_len))
    keep = [maps, pair_len]
    if device:
        map_ptr, have = _device_words(maps, "maps") if maps is not None else (None, 0)
        len_ptr = None
        if pair_len is not None:
            if not _is_device_tensor(pair_len):
                raise ValueError("reconstruct_warped: maps in device memory need pair_len in device memory too")
            len_ptr, have_len = _device_words(pair_len, "pair_len")
            if have_len < n:
                raise ValueError("reconstruct_warped: pair_len holds fewer than n entries")
    else:
        if _is_device_tensor(pair_len):
            raise ValueError("reconstruct_warped: pair_len in device memory needs maps in device memory too")
        host = np.ascontiguousarray(maps if maps is not None else [], dtype=np.uint32).reshape(-1)
        have, map_ptr = host.size, (host.ctypes.data if host.size else None)
        len_ptr = None
        keep.append(host)
        if pair_len is not None:
            plen = np.ascontiguousarray(pair_len, dtype=np.uint32).reshape(-1)
            if plen.size != n:
                raise ValueError("reconstruct_warped: pair_len must hold one entry per target")
            len_ptr = plen.ctypes.data if n else None
            keep.append(plen)
    if have < need:
        raise ValueError(f"reconstruct_warped: maps holds {have} entries, map_offsets asks for {need}")
    return idx, off, m_off, frames, map_ptr, len_ptr, device, keep


FOLLOW_MAX_GAIN = 8.0


def _follow_max_gain(max_gain) -> float:
    """max_gain of follow_envelope as a float, checked before the library is asked: finite and at least 1."""
    try:
        gain = float(max_gain)
    except (TypeError, ValueError):
        raise ValueError("max_gain must be a number") from None
    if not 1.0 <= gain < float("inf"):
        raise ValueError("max_gain must be finite and at least 1")
    return gain


def follow_dynamics(dynamics, max_gain):
    """The dynamics= / max_gain= keywords of the reconstructing methods, checked before any device work: None (the method as
    it was) or the checked max_gain of dynamics="target"."""
    if dynamics is not None and dynamics != "target":
        raise ValueError('dynamics must be None or "target"')
    gain = _follow_max_gain(max_gain)
    return gain if dynamics == "target" else None


def _follow_samples(x, need: int, what: str):
    """(pointer, device?, what to keep alive) of follow_envelope's samples or ref: a numpy array, or f64 device memory (a
    contiguous torch CUDA tensor, a DeviceFrames-style pointer) of at least `need` values."""
    if _is_device_tensor(x):
        size = getattr(x, "element_size", None)
        if callable(size) and size() != 8 or "float64" not in str(getattr(x, "dtype", "float64")):
            raise ValueError(f"follow_envelope: {what} in device memory must be float64")
        contiguous = getattr(x, "is_contiguous", None)
        if callable(contiguous) and not contiguous():
            raise ValueError(f"follow_envelope: the device tensor {what} must be contiguous")
        have = int(x.numel())
        ptr = int(x.data_ptr()) if have else None
        keep, device = x, True
    else:
        keep = np.ascontiguousarray(x if x is not None else [], dtype=np.float64).reshape(-1)
        have, ptr, device = keep.size, (keep.ctypes.data if keep.size else None), False
    if have < need:
        raise ValueError(f"follow_envelope: {what} holds {have} values, its offsets ask for {need}")
    return ptr, device, keep


def follow_boundaries(out_offsets) -> np.ndarray:
    """Offsets of the targets' gains in follow_envelope's packed gain array: n + 1 int64, target t has ceil(n_t / HOP) + 1
    boundaries when it has samples and none when it has not."""
    off = np.asarray(out_offsets, dtype=np.uint64).astype(np.int64)
    n = off[1:] - off[:-1]
    return np.concatenate([[0], np.cumsum(np.where(n > 0, (n + nat.MFCC_HOP - 1) // nat.MFCC_HOP + 1, 0))]).astype(np.int64)


WSOLA_MAX_SEARCH = 512


def _wsola_search(search) -> int:
    """The search width of reconstruct_wsola, checked on the host: an integer in 0 ... 512."""
    if isinstance(search, bool) or not isinstance(search, (int, np.integer)):
        raise ValueError("search must be an integer number of samples")
    if not 0 <= int(search) <= WSOLA_MAX_SEARCH:
        raise ValueError(f"search must lie in 0 ... {WSOLA_MAX_SEARCH} samples")
    return int(search)


def _warp_call(engine, name, smp, idx, out_offsets, maps, map_offsets, map_frames, pair_len, search, want_pcm32, want_pos,
               windows):
    """Engine.reconstruct_warped (search None) and reconstruct_wsola: the checks -- the metric, the search width, the inputs,
    all before anything touches the context -- the output arrays and the call of ssym_<name> or, with windows, of
    ssym_<name>_spans.  Returns (samples, pcm or None, positions or None)."""
    if engine.metric != "dtw":
        raise nat.SsymError(nat.SSYM_E_UNSUPPORTED, name + " follows dtw alignments: a refcos engine has none")
    if search is not None:
        search = _wsola_search(search)
    idx, off, m_off, frames, map_ptr, len_ptr, device, keep = _warp_inputs(idx, out_offsets, maps, map_offsets,
                                                                           map_frames, pair_len)
    windows = _warp_windows(windows, idx.size)
    total = int(off[-1])
    out = np.zeros(total, dtype=np.float64)
    pcm = np.zeros(total, dtype=np.int32) if want_pcm32 else None
    pos = np.full(int(m_off[-1]), np.iinfo(np.uint64).max, dtype=np.uint64) if want_pos else None
    flags = nat.WARP_MAP_DEVICE if device else 0
    mid = (flags,) if search is None else (search, flags, pos.ctypes.data if pos is not None and pos.size else None)
    args = (off.ctypes.data, idx.size, map_ptr, m_off.ctypes.data, frames.ctypes.data, len_ptr) + mid + (
        out.ctypes.data, pcm.ctypes.data if pcm is not None else None)
    if windows is None:
        rc = getattr(nat.lib(), "ssym_" + name)(engine.ctx, smp.ptr, idx.ctypes.data, *args)
    else:
        rc = getattr(nat.lib(), "ssym_" + name + "_spans")(engine.ctx, smp.ptr, idx.ctypes.data, windows[0].ctypes.data,
                                                          windows[1].ctypes.data, *args)
    nat.check(rc, engine.ctx)
    del keep
    return out, pcm, pos


class _Handle:
    def __init__(self, engine: "Engine", ptr: int, n: int, dim: int, kind: str):
        self.engine, self.ptr, self.n, self.dim, self.kind = engine, ptr, n, dim, kind

    def close(self):
        if self.ptr and self.engine.ctx:
            L = nat.lib()
            (L.ssym_dict_destroy if self.kind == "dict" else L.ssym_queries_destroy)(
                self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SamplesHandle:
    def __init__(self, engine, ptr, n):
        self.engine, self.ptr, self.n = engine, ptr, n

    def close(self):
        if self.ptr and self.engine.ctx:
            nat.lib().ssym_samples_destroy(self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Gmm:
    """A trained Gaussian mixture (ssym_gmm): K components over `dim`-value frames, resident on the engine's GPU."""

    def __init__(self, engine: "Engine", ptr: int, k: int, dim: int):
        self.engine, self.ptr, self.k, self.dim = engine, ptr, k, dim
        w, mu, cov = np.zeros(k), np.zeros((k, dim)), np.zeros((k, dim, dim))
        ll, it = ctypes.c_double(), ctypes.c_uint32()
        nat.check(nat.lib().ssym_gmm_get(ptr, w.ctypes.data, mu.ctypes.data, cov.ctypes.data, ctypes.byref(ll),
                                         ctypes.byref(it)))
        self.weights, self.means, self.covs, self.log_lik, self.iters = w, mu, cov, ll.value, it.value

    def close(self):
        if self.ptr and self.engine.ctx:
            nat.lib().ssym_gmm_destroy(self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceFrames:
    """A view of f64 values in device memory owned by somebody else (a Stream's resident frames or samples): the raw
    pointer and its shape.  It stands in for a contiguous float64 device tensor wherever the engine takes one
    (queries / dictionary, sequence_distances, gmm_predict, partition).  `owner` is kept alive; the view itself is
    valid only as long as the owner says (a Stream: until the next push, seed or close)."""

    is_cuda = True
    dtype = "torch.float64"

    def __init__(self, ptr: int, rows: int, dim: int, owner=None):
        self.ptr, self.shape, self.owner = int(ptr or 0), (int(rows), int(dim)), owner

    def data_ptr(self) -> int:
        return self.ptr

    def numel(self) -> int:
        return self.shape[0] * self.shape[1]

    def is_contiguous(self) -> bool:
        return True


def stream_plan(n_old: int, n_add: int):
    """What a push of `n_add` samples onto a sound of `n_old` analyses (host arithmetic only):
    (first new frame, new frames, first new power window, new power windows) for full 1024 / 256 MFCC windows and full
    128 / 64 power windows.  The old frames and windows plus the new ones are exactly those of the sound of
    n_old + n_add samples."""
    n_old, n_add = int(n_old), int(n_add)
    if n_old < 0 or n_add < 0:
        raise ValueError("stream_plan: sample counts must not be negative")

    def count(n, size, hop):
        return (n - size) // hop + 1 if n >= size else 0
    f0, f1 = count(n_old, nat.MFCC_BIN, nat.MFCC_HOP), count(n_old + n_add, nat.MFCC_BIN, nat.MFCC_HOP)
    w0, w1 = count(n_old, nat.POWER_WINDOW, nat.POWER_HOP), count(n_old + n_add, nat.POWER_WINDOW, nat.POWER_HOP)
    return f0, f1 - f0, w0, w1 - w0


class _Lanes:
    """What Stream, Spotter and Coverer share: `n_lanes` lanes, one of them named by a call."""

    def _lane(self, lane) -> int:
        if not 0 <= int(lane) < self.n_lanes:
            raise ValueError(f"lane {lane} outside 0..{self.n_lanes - 1}")
        return int(lane)


class Stream(_Lanes):
    """Growing sounds on the engine's GPU (ssym_stream): `n_lanes` independent sounds whose samples,
    MFCC frames, max_power and per-coefficient sums stay resident; a push uploads and analyses only what is new."""

    def __init__(self, engine: "Engine", ptr: int, n_lanes: int, ncoeffs: int, sample_rate: float):
        self.engine, self.ptr, self.n_lanes, self.ncoeffs, self.sample_rate = engine, ptr, n_lanes, ncoeffs, sample_rate

    def counts(self) -> Tuple[np.ndarray, np.ndarray]:
        """(samples [n_lanes], frames [n_lanes]) held now (u64)."""
        ns, nf = np.zeros(self.n_lanes, dtype=np.uint64), np.zeros(self.n_lanes, dtype=np.uint64)
        nat.check(nat.lib().ssym_stream_counts(self.ptr, ns.ctypes.data, nf.ctypes.data), self.engine.ctx)
        return ns, nf

    def push(self, samples, sample_offsets=None, want_frames: bool = False):
        """ssym_stream_push: lane l gets samples[sample_offsets[l]:sample_offsets[l+1]] (a one-lane stream takes the
        bare chunk).  Returns the new frames per lane [n_lanes] u64, and with want_frames also the new frames
        themselves, lane after lane, [sum][ncoeffs]."""
        x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        if sample_offsets is None:
            if self.n_lanes != 1:
                raise ValueError("push: a stream of several lanes needs sample_offsets")
            sample_offsets = [0, x.size]
        off = np.ascontiguousarray(sample_offsets, dtype=np.uint64).reshape(-1)
        if off.size != self.n_lanes + 1 or np.any(np.diff(off.astype(np.int64)) < 0) or int(off[-1]) > x.size:
            raise ValueError("sample_offsets: n_lanes + 1 non-decreasing sample offsets within `samples`")
        new = np.zeros(self.n_lanes, dtype=np.uint64)
        out = None
        if want_frames:
            ns, nf = self.counts()
            total = 0
            for l in range(self.n_lanes):
                f_all = stream_plan(int(ns[l]), int(off[l + 1] - off[l]))
                total += max(f_all[0] + f_all[1] - int(nf[l]), 0)      # (a seeded lane may lag behind its samples)
            out = np.zeros((total, self.ncoeffs), dtype=np.float64)
        nat.check(nat.lib().ssym_stream_push(self.engine.ctx, self.ptr, x.ctypes.data if x.size else None,
                                             off.ctypes.data, 0, new.ctypes.data,
                                             out.ctypes.data if out is not None and out.size else None),
                  self.engine.ctx)
        return (new, out) if want_frames else new

    def seed(self, lane: int, samples, mfccs=None) -> None:
        """ssym_stream_seed: fill an empty lane with an existing sound; `mfccs` (whole frames) are adopted as given,
        frames the samples allow beyond them are analysed by the next push; without them every frame is analysed."""
        x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        m = None if mfccs is None else np.ascontiguousarray(mfccs, dtype=np.float64).reshape(-1)
        if m is not None and m.size % self.ncoeffs:
            raise ValueError("mfccs must hold whole frames of `ncoeffs` values")
        frames = 0 if m is None else m.size // self.ncoeffs
        # (with mfccs a non-NULL pointer is passed even for 0 frames: NULL means "analyse")
        mp = None if m is None else (m.ctypes.data if m.size else np.zeros(1).ctypes.data)
        nat.check(nat.lib().ssym_stream_seed(self.engine.ctx, self.ptr, self._lane(lane),
                                             x.ctypes.data if x.size else None, x.size, mp, frames), self.engine.ctx)

    def read(self, lane: int = 0, first_frame: int = 0, n_frames: Optional[int] = None) -> np.ndarray:
        """ssym_stream_read: frames [first_frame, first_frame + n_frames) of a lane (default: to its end)."""
        lane = self._lane(lane)
        if n_frames is None:
            n_frames = max(int(self.counts()[1][lane]) - int(first_frame), 0)
        out = np.zeros((int(n_frames), self.ncoeffs), dtype=np.float64)
        nat.check(nat.lib().ssym_stream_read(self.engine.ctx, self.ptr, lane, int(first_frame), int(n_frames), 0,
                                             out.ctypes.data if out.size else None), self.engine.ctx)
        return out

    def frames_device(self, lane: int = 0) -> DeviceFrames:
        """The lane's resident frames [frames][ncoeffs] as a device view, valid until the next push / seed / close."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        nat.check(nat.lib().ssym_stream_frames_device(self.ptr, self._lane(lane), ctypes.byref(p), ctypes.byref(n)),
                  self.engine.ctx)
        return DeviceFrames(p.value, n.value, self.ncoeffs, self)

    def samples_device(self, lane: int = 0) -> DeviceFrames:
        """The lane's resident samples [samples][1] as a device view, valid until the next push / seed / close."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        nat.check(nat.lib().ssym_stream_samples_device(self.ptr, self._lane(lane), ctypes.byref(p), ctypes.byref(n)),
                  self.engine.ctx)
        return DeviceFrames(p.value, n.value, 1, self)

    def descriptors(self) -> Tuple[np.ndarray, np.ndarray]:
        """(max_power [n_lanes], mean MFCCs [n_lanes][ncoeffs]; NaN for a lane without frames)."""
        mp, mean = np.zeros(self.n_lanes), np.zeros((self.n_lanes, self.ncoeffs))
        nat.check(nat.lib().ssym_stream_descriptors(self.engine.ctx, self.ptr, mp.ctypes.data, mean.ctypes.data),
                  self.engine.ctx)
        return mp, mean

    def reset(self, lane: int = 0) -> None:
        """Empty one lane; its capacity stays."""
        nat.check(nat.lib().ssym_stream_reset(self.engine.ctx, self.ptr, self._lane(lane)), self.engine.ctx)

    def close(self):
        if self.ptr and self.engine.ctx:
            nat.lib().ssym_stream_destroy(self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _spotter_args(q, n_lanes, max_cost):
    """(lanes, per-target thresholds as a contiguous f64 array or None) of Engine.spotter, checked before the library is
    asked."""
    lanes = int(n_lanes)
    if lanes < 1:
        raise ValueError("n_lanes must be at least 1")
    if max_cost is None:
        return lanes, None
    mc = np.asarray(max_cost, dtype=np.float64)
    if mc.ndim == 0:
        mc = np.full(q.n, float(mc))
    mc = np.ascontiguousarray(mc.reshape(-1))
    if mc.size != q.n:
        raise ValueError("max_cost must be a scalar or one value per target")
    if np.isnan(mc).any():
        raise ValueError("max_cost must not be NaN")
    return lanes, mc


def _push_args(noun: str, n_lanes: int, dim: int, feats, frame_offsets):
    """(frames as a flat contiguous f64 array, n_lanes + 1 u64 frame offsets) of Spotter.push and Coverer.push, checked
    before the library is asked: whole frames, the bare block on one lane only, non-decreasing offsets within `feats`."""
    x = np.ascontiguousarray(feats, dtype=np.float64).reshape(-1)
    if x.size % dim:
        raise ValueError(f"feats must hold whole frames of {dim} values")
    if frame_offsets is None:
        if n_lanes != 1:
            raise ValueError(f"push: a {noun} of several lanes needs frame_offsets")
        frame_offsets = [0, x.size // dim]
    off = np.ascontiguousarray(frame_offsets, dtype=np.uint64).reshape(-1)
    if off.size != n_lanes + 1 or np.any(np.diff(off.astype(np.int64)) < 0) or int(off[-1]) * dim > x.size:
        raise ValueError("frame_offsets: n_lanes + 1 non-decreasing frame offsets within `feats`")
    return x, off


class Spotter(_Lanes):
    """The targets of a query set watched in `n_lanes` growing sources (ssym_spotter; definition in
    include/soundsym_amd.h and DESIGN.md section 2 "Watching"): a push costs the new frames alone, the best span so far is
    ssym_dtw_spot's for everything consumed, and occurrences are reported as events by a causal rule.  The spotter reads
    the query set's resident features for as long as it lives: it keeps `q` alive and must be closed before it.
    `step` is the pattern it was created with ("Paced watching" for "paced": the best is ssym_dtw_spot_step's)."""

    def __init__(self, engine: "Engine", ptr: int, q: _Handle, n_lanes: int, step: str = "symmetric"):
        self.engine, self.ptr, self.q, self.n_lanes, self.n_targets, self.dim = engine, ptr, q, n_lanes, q.n, q.dim
        self.step = step
        self.n_events = 0

    def _run(self, call, new_rows, want_profile: bool):
        n = ctypes.c_uint64()
        pd = ps = None
        if want_profile:
            total = int(np.sum(new_rows)) * self.n_targets
            pd, ps = np.zeros(total, dtype=np.float64), np.zeros(total, dtype=np.uint32)
        nat.check(call(ctypes.byref(n), pd.ctypes.data if pd is not None and pd.size else None,
                       ps.ctypes.data if ps is not None and ps.size else None), self.engine.ctx)
        self.n_events = int(n.value)
        if not want_profile:
            return self.n_events
        cuts = np.cumsum([0] + [int(r) * self.n_targets for r in new_rows])
        shape = lambda x: [x[cuts[l]:cuts[l + 1]].reshape(self.n_targets, int(new_rows[l])) for l in range(self.n_lanes)]
        return self.n_events, shape(pd), shape(ps)

    def push(self, feats, frame_offsets=None, want_profile: bool = False):
        """ssym_spotter_push: lane l consumes the frames feats[frame_offsets[l]:frame_offsets[l+1]] ([frames][dim]; a
        one-lane spotter takes the bare block).  Returns the number of events emitted, and with want_profile also the new
        rows of the profile per lane: two lists of [n_targets][new rows] arrays (delta f64, s uint32)."""
        x, off = _push_args("spotter", self.n_lanes, self.dim, feats, frame_offsets)
        L = nat.lib()
        call = lambda n, pd, ps: L.ssym_spotter_push(self.engine.ctx, self.ptr, x.ctypes.data if x.size else None,
                                                     off.ctypes.data, 0, n, pd, ps)
        return self._run(call, np.diff(off.astype(np.int64)), want_profile)

    def follow(self, stream: "Stream", want_profile: bool = False):
        """ssym_spotter_follow: every lane consumes, in place, the frames the stream's lane holds beyond those consumed.
        Returns as push."""
        if stream.n_lanes != self.n_lanes or stream.ncoeffs != self.dim:
            raise ValueError("follow: the stream's lanes and ncoeffs must be the spotter's lanes and dim")
        new = stream.counts()[1].astype(np.int64) - self.counts().astype(np.int64)
        L = nat.lib()
        call = lambda n, pd, ps: L.ssym_spotter_follow(self.engine.ctx, self.ptr, stream.ptr, 0, n, pd, ps)
        return self._run(call, np.maximum(new, 0), want_profile)

    def events(self):
        """The events of the last push / follow / flush, ordered by (lane, target, end): (lane uint32 [n], target uint32
        [n], cost f64 [n], start uint32 [n], end uint32 [n]); end is inclusive."""
        n = self.n_events
        lane, tgt, start, end = (np.zeros(n, dtype=np.uint32) for _ in range(4))
        cost = np.zeros(n, dtype=np.float64)
        if n:
            nat.check(nat.lib().ssym_spotter_events(self.engine.ctx, self.ptr, lane.ctypes.data, tgt.ctypes.data,
                                                    cost.ctypes.data, start.ctypes.data, end.ctypes.data, 0), self.engine.ctx)
        return lane, tgt, cost, start, end

    def flush(self, lane: int = 0) -> int:
        """ssym_spotter_flush: "the lane has ended" -- what it has pending is emitted.  Returns the number of events."""
        lane = self._lane(lane)
        n = ctypes.c_uint64()
        nat.check(nat.lib().ssym_spotter_flush(self.engine.ctx, self.ptr, lane, ctypes.byref(n)), self.engine.ctx)
        self.n_events = int(n.value)
        return self.n_events

    def best(self):
        """(cost f64, start uint32, end uint32), each [n_lanes][n_targets]: ssym_dtw_spot's result for what every lane has
        consumed so far; +inf and NO_MATCH where there is none."""
        shape = (self.n_lanes, self.n_targets)
        cost, start, end = np.zeros(shape), np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32)
        nat.check(nat.lib().ssym_spotter_best(self.engine.ctx, self.ptr, cost.ctypes.data, start.ctypes.data,
                                              end.ctypes.data, 0), self.engine.ctx)
        return cost, start, end

    def counts(self) -> np.ndarray:
        """Frames consumed per lane [n_lanes] (u64)."""
        out = np.zeros(self.n_lanes, dtype=np.uint64)
        nat.check(nat.lib().ssym_spotter_counts(self.ptr, out.ctypes.data), self.engine.ctx)
        return out

    def reset(self, lane: int = 0) -> None:
        """One lane back to "nothing consumed"."""
        lane = self._lane(lane)
        nat.check(nat.lib().ssym_spotter_reset(self.engine.ctx, self.ptr, lane), self.engine.ctx)

    def close(self):
        if self.ptr and self.engine.ctx:
            nat.lib().ssym_spotter_destroy(self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _LiveTiling(_Lanes):
    """What Coverer and Mosaicker share: `n_lanes` growing targets tiled from one resident dictionary, fed by push or follow,
    ended lane by lane with flush.  A subclass names its noun (the ssym_<noun>_* calls), the attribute that holds the count
    of the last call's results, what the count counts, and what its capacity is.  The object reads the dictionary's
    resident features for as long as it lives: it keeps `d` alive and must be closed before it."""

    _noun = _count = None
    _count_on_refusal = False        # True: a refused call's count is recorded as well

    def __init__(self, engine: "Engine", ptr: int, d: _Handle, n_lanes: int, piece_penalty: float, gap_cost=None):
        self.engine, self.ptr, self.d, self.n_lanes, self.dim = engine, ptr, d, n_lanes, d.dim
        self.piece_penalty, self.gap_cost = piece_penalty, gap_cost
        setattr(self, self._count, 0)

    def _call(self, name: str, *args) -> int:
        return getattr(nat.lib(), f"ssym_{self._noun}_{name}")(self.engine.ctx, self.ptr, *args)

    def _ran(self, name: str, *args) -> int:
        """A call that ends in the count output: the count it leaves is that of the last call's results."""
        n = ctypes.c_uint64()
        rc = self._call(name, *args, ctypes.byref(n))
        if self._count_on_refusal:
            setattr(self, self._count, int(n.value))
        nat.check(rc, self.engine.ctx)
        setattr(self, self._count, int(n.value))
        return int(n.value)

    def push(self, feats, frame_offsets=None) -> int:
        """ssym_<noun>_push: lane l consumes the frames feats[frame_offsets[l]:frame_offsets[l+1]] ([frames][dim]; an object
        of one lane takes the bare block).  Returns the number of pieces (coverer) or frames (mosaicker) the push committed;
        `pieces` / `frames` reads them."""
        x, off = _push_args(self._noun, self.n_lanes, self.dim, feats, frame_offsets)
        return self._ran("push", x.ctypes.data if x.size else None, off.ctypes.data, 0)

    def follow(self, stream: "Stream") -> int:
        """ssym_<noun>_follow: every lane consumes, device to device, the frames the stream's lane holds beyond those
        consumed (a lane that has ended is skipped).  Returns as push."""
        if stream.n_lanes != self.n_lanes or stream.ncoeffs != self.dim:
            raise ValueError(f"follow: the stream's lanes and ncoeffs must be the {self._noun}'s lanes and dim")
        return self._ran("follow", stream.ptr, 0)

    def flush(self, lane: int = 0) -> int:
        """ssym_<noun>_flush: "the lane has ended" -- the rest of its cover or mosaic is emitted, and the lane consumes
        nothing more until `reset`.  Returns the number of pieces or frames."""
        return self._ran("flush", self._lane(lane))

    def _results(self, name: str, dtypes, on_device: bool):
        """The arrays of the last call's results through ssym_<noun>_<name>, in the order of its outputs."""
        n = getattr(self, self._count)
        device = self.engine.device if on_device else None
        outs = [_output(device, (n,), t) for t in dtypes]
        if n:
            nat.check(self._call(name, *(p for _, p in outs), 0 if device is None else nat.OUT_DEVICE), self.engine.ctx)
        return [a for a, _ in outs]

    def best(self, on_device: bool = False):
        """(total f64, covered uint32, committed uint32), each [n_lanes]: the offline call's total (ssym_dtw_cover's or
        ssym_dtw_mosaic's) for what the lane has consumed so far (+inf without a cover or mosaic), the frames of the longest
        prefix that has one, and the frames whose pieces or frames have been emitted."""
        device = self.engine.device if on_device else None
        (total, pt), (covered, pc), (committed, pm) = (_output(device, (self.n_lanes,), t)
                                                      for t in (np.float64, np.uint32, np.uint32))
        nat.check(self._call("best", pt, pc, pm, 0 if device is None else nat.OUT_DEVICE), self.engine.ctx)
        return total, covered, committed

    def counts(self):
        """(frames consumed per lane [n_lanes] u64, capacity: of the coverer's back-pointer ring in frames, of the
        mosaicker's ring in columns)."""
        out = np.zeros(self.n_lanes, dtype=np.uint64)
        cap = ctypes.c_uint64()
        nat.check(getattr(nat.lib(), f"ssym_{self._noun}_counts")(self.ptr, out.ctypes.data, ctypes.byref(cap)), self.engine.ctx)
        return out, int(cap.value)

    def reset(self, lane: int = 0) -> None:
        """One lane back to "nothing consumed"."""
        nat.check(self._call("reset", self._lane(lane)), self.engine.ctx)

    def close(self):
        if self.ptr and self.engine.ctx:
            self._call("destroy")
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Coverer(_LiveTiling):
    """`n_lanes` growing targets tiled by the segments of one resident dictionary (ssym_coverer; definition in
    include/soundsym_amd.h and DESIGN.md section 2 "Live cover"): every piece is reported by the push after which no
    longer recording could change it, the pieces from reset to flush are ssym_dtw_cover's for the whole, and `best` gives
    ssym_dtw_cover's total for everything consumed so far.  The coverer reads the dictionary's resident features for as
    long as it lives: it keeps `d` alive and must be closed before it.  After a refused call n_pieces is what it was."""

    _noun, _count = "coverer", "n_pieces"

    def pieces(self, on_device: bool = False):
        """The pieces of the last push / follow / flush, ordered by (lane, start): (lane uint32 [n], src uint32 [n], start
        uint32 [n], end uint32 [n], cost f64 [n]); start / end count the lane's frames since its reset, end inclusive.
        On a coverer with a gap_cost a frame left uncovered is the piece (lane, COVER_GAP, e, e, gap_cost).
        on_device: SSYM_OUT_DEVICE, the five arrays as torch tensors in device memory."""
        return tuple(self._results("pieces", (np.uint32, np.uint32, np.uint32, np.uint32, np.float64), on_device))


class Mosaicker(_LiveTiling):
    """`n_lanes` growing targets tiled by free spans of the uncut recordings of one resident dictionary (ssym_mosaicker;
    definition in include/soundsym_amd.h and DESIGN.md section 2 "Live mosaic"): every target frame is reported by the
    push after which no longer recording could change it, the frames from reset to flush are ssym_dtw_mosaic's for the
    whole, and `best` gives ssym_dtw_mosaic's total for everything consumed so far.  The mosaicker reads the dictionary's
    resident features for as long as it lives: it keeps `d` alive and must be closed before it.  A call refused after some
    slices has those slices' frames in its log, so n_frames is recorded before the refusal is raised."""

    _noun, _count, _count_on_refusal = "mosaicker", "n_frames", True

    def frames(self, on_device: bool = False):
        """The frames of the last push / follow / flush, ordered by (lane, column): (lane uint32 [n], column uint32 [n],
        src uint32 [n], frame uint32 [n], cost f64 [n], start uint32 [n]).  column counts the lane's frames since its
        reset; (src, frame, cost) are dtw_mosaic's per-frame outputs (a gap frame: COVER_GAP, NO_MATCH, gap_cost); start
        is 1 where a piece or a gap frame starts.  on_device: SSYM_OUT_DEVICE, the six arrays as torch tensors."""
        return tuple(self._results("frames", (np.uint32, np.uint32, np.uint32, np.uint32, np.float64, np.uint32), on_device))


class Resynth(_Lanes):
    """`n_lanes` lanes of live resynthesis against one resident sample store (ssym_resynth; definition in
    include/soundsym_amd.h and DESIGN.md section 2 "Live resynthesis"): a lane takes committed mosaic frames -- a
    Mosaicker's frame log device to device (`take`) or host arrays (`push`) -- and releases output samples as soon as their
    bits can no longer change; from reset to flush a lane's output is reconstruct_mosaic's, bit for bit.  The object reads
    the sample store for as long as it lives: it keeps `store` alive and must be closed before it.  n_samples: the samples
    the last push / take / flush released, `samples` reads them."""

    def __init__(self, engine: "Engine", ptr: int, store, n_lanes: int, search: int):
        self.engine, self.ptr, self.store, self.n_lanes, self.search = engine, ptr, store, n_lanes, search
        self.n_samples = 0

    def _ran(self, name: str, *args) -> int:
        n = ctypes.c_uint64()
        nat.check(getattr(nat.lib(), "ssym_resynth_" + name)(self.engine.ctx, self.ptr, *args, ctypes.byref(n)), self.engine.ctx)
        self.n_samples = int(n.value)
        return self.n_samples

    def push(self, lane, column, src, frame, start) -> int:
        """ssym_resynth_push: frames in host arrays ordered by (lane, column) -- a Mosaicker.frames() result's lane,
        column, src, frame and start pass straight in.  Returns the number of samples released."""
        arrays = [np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (lane, column, src, frame, start)]
        n = arrays[0].size
        if any(a.size != n for a in arrays):
            raise ValueError("push: lane, column, src, frame and start must hold one entry per frame")
        return self._ran("push", *(a.ctypes.data if n else None for a in arrays), n)

    def take(self, mosaicker: "Mosaicker") -> int:
        """ssym_resynth_take: consume the mosaicker's last frame log where it lies, device to device.  Returns as push."""
        if mosaicker.n_lanes != self.n_lanes:
            raise ValueError("take: the mosaicker's lanes must be the resynthesiser's")
        return self._ran("take", mosaicker.ptr)

    def flush(self, lane: int, total_samples: int) -> int:
        """ssym_resynth_flush: "the lane has ended with total_samples samples" -- the open tile is closed, the rest and the
        tail behind the last frame are released, and the lane consumes nothing more until `reset`."""
        total = int(total_samples)
        if total < 0 or total != total_samples:
            raise ValueError("total_samples must be a whole number of samples, not negative")
        return self._ran("flush", self._lane(lane), total)

    def samples(self, want_pcm32: bool = False, on_device: bool = False):
        """The samples of the last push / take / flush: (lane_offsets uint64 [n_lanes + 1], samples f64 [n_samples]) and
        with want_pcm32 the int32 samples too; lane l's are [lane_offsets[l], lane_offsets[l + 1]).  on_device:
        SSYM_OUT_DEVICE, the samples as torch tensors in device memory (the offsets stay a numpy array)."""
        off = np.zeros(self.n_lanes + 1, dtype=np.uint64)
        device = self.engine.device if on_device else None
        (out, po), (pcm, pp) = _output(device, (self.n_samples,), np.float64), _output(device, (self.n_samples,), np.int32)
        nat.check(nat.lib().ssym_resynth_samples(self.engine.ctx, self.ptr, off.ctypes.data, po if self.n_samples else None,
                                                 pp if want_pcm32 and self.n_samples else None,
                                                 0 if device is None else nat.OUT_DEVICE), self.engine.ctx)
        return (off, out, pcm) if want_pcm32 else (off, out)

    def counts(self):
        """(frames consumed, samples released) per lane since its reset, uint64 [n_lanes] each."""
        frames, smp = np.zeros(self.n_lanes, dtype=np.uint64), np.zeros(self.n_lanes, dtype=np.uint64)
        nat.check(nat.lib().ssym_resynth_counts(self.ptr, frames.ctypes.data, smp.ctypes.data), self.engine.ctx)
        return frames, smp

    def reset(self, lane: int = 0) -> None:
        """One lane back to "nothing consumed"."""
        nat.check(nat.lib().ssym_resynth_reset(self.engine.ctx, self.ptr, self._lane(lane)), self.engine.ctx)

    def close(self):
        if self.ptr and self.engine.ctx:
            nat.lib().ssym_resynth_destroy(self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FOLLOWER_MAX_LANES = 16384


class Follower(_Lanes):
    """`n_lanes` lanes of live envelope following (ssym_follower; definition in include/soundsym_amd.h and DESIGN.md
    section 2 "Live envelope following"): a lane takes the resynthesis y and the reference x as they grow, in any amounts,
    and releases every output hop once its two boundaries are settled -- two hops of look-ahead on both signals; from reset
    to flush a lane's samples and gains are follow_envelope's for what it consumed, bit for bit.  n_samples: the samples the
    last push / flush released, `samples` reads them."""

    def __init__(self, engine: "Engine", ptr: int, n_lanes: int, max_gain: float):
        self.engine, self.ptr, self.n_lanes, self.max_gain = engine, ptr, n_lanes, max_gain
        self.n_samples = 0

    def _ran(self, name: str, *args) -> int:
        n = ctypes.c_uint64()
        nat.check(getattr(nat.lib(), "ssym_follower_" + name)(self.engine.ctx, self.ptr, *args, ctypes.byref(n)), self.engine.ctx)
        self.n_samples = int(n.value)
        return self.n_samples

    def _offsets(self, offsets, x, what: str) -> np.ndarray:
        if offsets is None:
            if self.n_lanes != 1:
                raise ValueError(f"push: {what} offsets are needed with more than one lane")
            return np.array([0, 0 if x is None else (int(x.numel()) if _is_device_tensor(x) else np.asarray(x).size)], dtype=np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if off.size != self.n_lanes + 1:
            raise ValueError(f"push: n_lanes + 1 {what} offsets")
        if off[0] != 0 or np.any(off[1:] < off[:-1]):
            raise ValueError(f"push: the {what} offsets must start at 0 and not decrease")
        return off

    def push(self, samples, sample_offsets=None, ref=None, ref_offsets=None) -> int:
        """ssym_follower_push: lane l consumes samples[sample_offsets[l]:sample_offsets[l+1]] of the resynthesis and
        ref[ref_offsets[l]:ref_offsets[l+1]] of the reference (a follower of one lane takes the bare arrays).  Either is a
        numpy array or f64 device memory (a contiguous torch CUDA tensor: Resynth.samples(on_device=True) passes straight
        in); None holds nothing.  Returns the number of samples released."""
        off, r_off = self._offsets(sample_offsets, samples, "sample"), self._offsets(ref_offsets, ref, "ref")
        y_ptr, y_dev, keep_y = _follow_samples(samples, int(off[-1]), "samples")
        x_ptr, x_dev, keep_x = _follow_samples(ref, int(r_off[-1]), "ref")
        flags = (nat.FOLLOW_SAMPLES_DEVICE if y_dev else 0) | (nat.FOLLOW_REF_DEVICE if x_dev else 0)
        n = self._ran("push", y_ptr, off.ctypes.data, x_ptr, r_off.ctypes.data, flags)
        del keep_y, keep_x
        return n

    def flush(self, lane: int = 0) -> int:
        """ssym_follower_flush: "the lane has ended" -- every remaining boundary is settled with the offline clipping, the
        rest of the resynthesis leaves, and the lane consumes nothing more until `reset`."""
        return self._ran("flush", self._lane(lane))

    def samples(self, want_pcm32: bool = False, want_gains: bool = False, on_device: bool = False):
        """What the last push / flush released: (lane_offsets uint64 [n_lanes + 1], samples f64 [n_samples]); with
        want_pcm32 the int32 samples too; with want_gains also (gain_offsets uint64 [n_lanes + 1], gains f64) -- the gains
        of the boundaries that call settled, lane by lane.  on_device: SSYM_OUT_DEVICE, samples, pcm and gains as torch
        tensors in device memory (the offsets stay numpy arrays)."""
        off, g_off = np.zeros(self.n_lanes + 1, dtype=np.uint64), np.zeros(self.n_lanes + 1, dtype=np.uint64)
        device = self.engine.device if on_device else None
        nat.check(nat.lib().ssym_follower_samples(self.engine.ctx, self.ptr, off.ctypes.data, None, None, g_off.ctypes.data, None, 0),
                  self.engine.ctx)
        n, n_gains = int(off[-1]), int(g_off[-1]) if want_gains else 0
        (out, po), (pcm, pp), (gain, pg) = (_output(device, (n,), np.float64), _output(device, (n,), np.int32),
                                            _output(device, (n_gains,), np.float64))
        if n or n_gains:
            nat.check(nat.lib().ssym_follower_samples(self.engine.ctx, self.ptr, None, po if n else None,
                                                      pp if want_pcm32 and n else None, None, pg if n_gains else None,
                                                      0 if device is None else nat.OUT_DEVICE), self.engine.ctx)
        res = (off, out) + ((pcm,) if want_pcm32 else ())
        return res + ((g_off, gain) if want_gains else ())

    def counts(self):
        """(ny, nx, released): samples of the resynthesis and of the reference consumed, and samples released, per lane
        since its reset, uint64 [n_lanes] each."""
        ny, nx, rel = (np.zeros(self.n_lanes, dtype=np.uint64) for _ in range(3))
        nat.check(nat.lib().ssym_follower_counts(self.ptr, ny.ctypes.data, nx.ctypes.data, rel.ctypes.data), self.engine.ctx)
        return ny, nx, rel

    def reset(self, lane: int = 0) -> None:
        """One lane back to "nothing consumed"."""
        nat.check(nat.lib().ssym_follower_reset(self.engine.ctx, self.ptr, self._lane(lane)), self.engine.ctx)

    def close(self):
        if self.ptr and self.engine.ctx:
            nat.lib().ssym_follower_destroy(self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """One rank of a source-sharded run: an RCCL communicator bound to an Engine (ssym_comm)."""

    def __init__(self, engine: "Engine", ptr: int, rank: int, world: int):
        self.engine, self.ptr, self.rank, self.world = engine, ptr, rank, world

    def set_timeout(self, milliseconds: int) -> None:
        """ssym_comm_set_timeout: the deadline of one match_sharded step (a rank that never arrives)."""
        nat.check(nat.lib().ssym_comm_set_timeout(self.ptr, int(milliseconds)), self.engine.ctx)

    @property
    def dead(self) -> bool:
        """ssym_comm_is_dead: aborted by a failure; every further step raises SSYM_E_COMM."""
        return bool(self.ptr) and nat.lib().ssym_comm_is_dead(self.ptr) == 1

    def inject_fault(self, phase: int, kind: int) -> None:
        """ssym_comm_inject_fault (containment tests): the next step fails in `phase`; kind 0 = the local work
        reports an error and the rank takes part, kind 1 = the rank leaves the step without its collectives."""
        nat.check(nat.lib().ssym_comm_inject_fault(self.ptr, phase, kind), self.engine.ctx)

    def replay_bounds(self, bounds) -> None:
        """ssym_comm_replay_bounds (measurement hook, needs SSYM_TEST_HOOKS=1): a device tensor of per-target bounds
        (f64, one per target) that joins every following step's bound exchange; None clears.  The tensor is kept alive."""
        self._replay = bounds
        if bounds is None:
            nat.check(nat.lib().ssym_comm_replay_bounds(self.ptr, None, 0), self.engine.ctx)
        else:
            nat.check(nat.lib().ssym_comm_replay_bounds(self.ptr, bounds.data_ptr(), int(bounds.numel())), self.engine.ctx)

    def close(self):
        if self.ptr and self.engine.ctx:
            nat.lib().ssym_comm_destroy(self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_available() -> bool:
    """ssym_comm_available: the library itself could bind every RCCL symbol it calls (what the ranks of a job agree
    on before any of them enters comm_create)."""
    try:
        nat.load_rccl()
    except ImportError:
        pass                  # (the library still looks for librccl.so.1 / $SSYM_RCCL_LIB by itself)
    return nat.lib().ssym_comm_available() == 1


class LocalGroup:
    """The ranks of one process without RCCL (ssym_local_group): a thread per rank, every rank its own Engine.
    RCCL refuses two ranks on one device; this is how the multi-rank logic of ssym_match_sharded runs on a one-GPU
    box.  Every rank's thread must be inside match_sharded at the same time (ctypes releases the GIL)."""

    def __init__(self, world: int):
        out = ctypes.c_void_p()
        nat.check(nat.lib().ssym_local_group_create(world, ctypes.byref(out)), None)
        self.ptr, self.world = out.value, world

    def close(self):
        if self.ptr:
            nat.lib().ssym_local_group_destroy(self.ptr)
        self.ptr = None


def comm_unique_id() -> bytes:
    """ssym_comm_unique_id: the 128-byte RCCL id rank 0 hands to the other ranks."""
    nat.load_rccl()
    buf = ctypes.create_string_buffer(nat.COMM_ID_BYTES)
    nat.check(nat.lib().ssym_comm_unique_id(buf), None)
    return buf.raw


def pitch_lags(rate: float, f_min: float, f_max: float, voicing: float = 0.2):
    """The lag range (tau_lo, tau_hi) of ssym_sound_descriptors / ssym_pitch_track, or ValueError for arguments outside
    their limits -- checked on the host, before anything reaches the device."""
    import math
    vals = [float(rate), float(f_min), float(f_max), float(voicing)]
    if not all(math.isfinite(v) for v in vals) or not (vals[0] > 0 and 0 < vals[1] < vals[2]):
        raise ValueError("need a finite rate > 0, 0 < f_min < f_max and a finite voicing threshold")
    lo, hi = math.ceil(vals[0] / vals[2]), math.floor(vals[0] / vals[1])
    if not (2 <= lo <= hi <= nat.PITCH_WINDOW // 3):
        raise ValueError(f"need 2 <= ceil(rate / f_max) <= floor(rate / f_min) <= {nat.PITCH_WINDOW // 3}, "
                         f"got {lo} and {hi}")
    return lo, hi


class Engine:
    """One ssym_ctx: one GPU, one stream, one metric / dtype configuration."""

    def __init__(self, metric: str = "dtw", dtype: str = "f32", device: int = 0, band: int = -1,
                 squared: bool = False, stream: Optional[int] = None, prune: bool = False):
        self.metric, self.dtype = metric, dtype
        self.np_dtype = {"f64": np.float64, "f32": np.float32}[dtype]
        self.ctx = None
        cfg = nat.Config(ctypes.sizeof(nat.Config), device,
                         {"refcos": nat.METRIC_REFCOS, "dtw": nat.METRIC_DTW}[metric],
                         {"f64": nat.DTYPE_F64, "f32": nat.DTYPE_F32}[dtype], band,
                         1 if squared else 0, stream, 1 if prune else 0, 0)
        out = ctypes.c_void_p()
        nat.check(nat.lib().ssym_ctx_create(ctypes.byref(cfg), ctypes.byref(out)), None)
        self.ctx = out.value
        self.device = device

    def close(self):
        if self.ctx:
            nat.lib().ssym_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- resident segment sets ---------------------------------------------------------------
    def _make(self, kind: str, feats, offsets, dim: int) -> _Handle:
        L = nat.lib()
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = off.size - 1
        if n < 0:
            raise ValueError("offsets must hold n+1 entries")
        out = ctypes.c_void_p()
        if _is_device_tensor(feats):
            want = {"f64": "torch.float64", "f32": "torch.float32"}[self.dtype]
            if str(feats.dtype) != want or not feats.is_contiguous():
                raise ValueError(f"device features must be contiguous {want}")
            fn = L.ssym_dict_create_device if kind == "dict" else L.ssym_queries_create_device
            fptr = feats.data_ptr()
            keep = feats
        else:
            keep = np.ascontiguousarray(feats, dtype=self.np_dtype).reshape(-1)
            fn = L.ssym_dict_create if kind == "dict" else L.ssym_queries_create
            fptr = keep.ctypes.data
        rc = fn(self.ctx, fptr, off.ctypes.data, n, dim, ctypes.byref(out))
        del keep
        nat.check(rc, self.ctx)
        h = _Handle(self, out.value, n, dim, kind)
        h.offsets = off - off[0] if n > 0 else np.zeros(1, dtype=np.uint64)      # frames before every segment
        return h

    def dictionary(self, feats, offsets, dim: int) -> _Handle:
        return self._make("dict", feats, offsets, dim)

    def queries(self, feats, offsets, dim: int) -> _Handle:
        return self._make("queries", feats, offsets, dim)

    def dictionary_append(self, d: _Handle, feats, offsets) -> None:
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        f = np.ascontiguousarray(feats, dtype=self.np_dtype).reshape(-1)
        nat.check(nat.lib().ssym_dict_append(self.ctx, d.ptr, f.ctypes.data, off.ctypes.data,
                                             off.size - 1), self.ctx)
        d.n += off.size - 1

    # -- the hot path ------------------------------------------------------------------------
    def match(self, d: _Handle, q: _Handle, distance=None, index_base: int = 0,
              force_exact: bool = False, out_idx=None, out_cost=None, prune: bool = False,
              step: str = "symmetric") -> Tuple[np.ndarray, np.ndarray]:
        """argmin per target.  With torch CUDA tensors in out_idx (int32/uint32 storage, n
        entries) and out_cost (float64) the results stay on the device.  prune=True asks for
        early abandoning (SSYM_DTW_PRUNE): same results, data-dependent time.  step="paced":
        ssym_match_queries_step with SSYM_STEP_PACED ("Paced matching": the cost is ssym_dtw_align_step's paced cost,
        +inf for a pair whose shape has no paced path; costs stay sums; force_exact and prune mean nothing there);
        "symmetric" is ssym_match_queries itself."""
        which = _spot_step(step)
        L = nat.lib()
        m = q.n
        dist_p = None
        if distance is not None:
            dist = np.ascontiguousarray(distance, dtype=np.float64)
            if dist.size != m:
                raise ValueError("distance must have one entry per target")
            dist_p = dist.ctypes.data
        flags = (nat.DTW_FORCE_EXACT if force_exact else 0) | (nat.DTW_PRUNE if prune else 0)
        if which == nat.STEP_SYMMETRIC:
            call = lambda oi, oc, fl: L.ssym_match_queries(self.ctx, d.ptr, q.ptr, dist_p, index_base, oi, oc, fl)
        else:
            call = lambda oi, oc, fl: L.ssym_match_queries_step(self.ctx, d.ptr, q.ptr, dist_p, index_base, which, oi, oc, fl)
        if out_idx is not None and _is_device_tensor(out_idx):
            flags |= nat.OUT_DEVICE
            rc = call(out_idx.data_ptr(), out_cost.data_ptr() if out_cost is not None else None, flags)
            nat.check(rc, self.ctx)
            return out_idx, out_cost
        idx = np.zeros(m, dtype=np.uint32)
        cost = np.zeros(m, dtype=np.float64)
        rc = call(idx.ctypes.data, cost.ctypes.data, flags)
        nat.check(rc, self.ctx)
        return idx, cost

    def match_begin(self, d: _Handle, q: _Handle, bounds, distance=None, index_base: int = 0) -> None:
        """ssym_match_begin: filter + per-target bound into `bounds` (torch CUDA float64 [m])."""
        dist_p = None
        if distance is not None:
            dist = np.ascontiguousarray(distance, dtype=np.float64)
            if dist.size != q.n:
                raise ValueError("distance must have one entry per target")
            dist_p = dist.ctypes.data
        nat.check(nat.lib().ssym_match_begin(self.ctx, d.ptr, q.ptr, dist_p, index_base, bounds.data_ptr()),
                  self.ctx)

    def match_candidates(self, d: _Handle, q: _Handle, costs) -> None:
        """ssym_match_candidates: exact cost of this shard's candidate pair per target into `costs`
        (torch CUDA float64 [m]); all-reduce(MIN) it, then match_begin(..., candidate_costs=costs)."""
        nat.check(nat.lib().ssym_match_candidates(self.ctx, d.ptr, q.ptr, costs.data_ptr()), self.ctx)

    def match_begin_pruned(self, d: _Handle, q: _Handle, bounds, candidate_costs, index_base: int = 0) -> None:
        """ssym_match_begin_pruned: match_begin whose filter abandons pairs above the reduced costs."""
        nat.check(nat.lib().ssym_match_begin_pruned(self.ctx, d.ptr, q.ptr, index_base, candidate_costs.data_ptr(),
                                                    bounds.data_ptr()), self.ctx)

    def match_finish(self, bounds, out_idx, out_cost):
        """ssym_match_finish with device outputs (torch CUDA tensors)."""
        nat.check(nat.lib().ssym_match_finish(self.ctx, bounds.data_ptr(), out_idx.data_ptr(),
                                              out_cost.data_ptr() if out_cost is not None else None,
                                              nat.OUT_DEVICE), self.ctx)
        return out_idx, out_cost

    # -- source-sharded runs: the collectives inside the library (RCCL on the context's stream) ----------
    def comm_create(self, unique_id: bytes, rank: int, world: int) -> Comm:
        """ssym_comm_create: collective over all `world` ranks (ncclCommInitRank on this engine's GPU)."""
        nat.load_rccl()
        if len(unique_id) != nat.COMM_ID_BYTES:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        out = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(unique_id), nat.COMM_ID_BYTES)
        nat.check(nat.lib().ssym_comm_create(self.ctx, buf, rank, world, ctypes.byref(out)), self.ctx)
        return Comm(self, out.value, rank, world)

    def comm_create_local(self, group: LocalGroup, rank: int) -> Comm:
        """ssym_comm_create_local: this engine as rank `rank` of an in-process group (no RCCL)."""
        out = ctypes.c_void_p()
        nat.check(nat.lib().ssym_comm_create_local(self.ctx, group.ptr, rank, ctypes.byref(out)), self.ctx)
        return Comm(self, out.value, rank, group.world)

    def match_sharded(self, comm: Comm, d: _Handle, q: _Handle, distance=None, index_base: int = 0,
                      out_idx=None, out_cost=None, prune: bool = False, force_exact: bool = False):
        """ssym_match_sharded: this rank's shard `d` (global indices from index_base) against all targets `q`;
        every rank returns the merged answer.  Outputs as for match()."""
        L = nat.lib()
        m = q.n
        dist_p = None
        if distance is not None:
            dist = np.ascontiguousarray(distance, dtype=np.float64)
            if dist.size != m:
                raise ValueError("distance must have one entry per target")
            dist_p = dist.ctypes.data
        flags = (nat.DTW_FORCE_EXACT if force_exact else 0) | (nat.DTW_PRUNE if prune else 0)
        if out_idx is not None and _is_device_tensor(out_idx):
            rc = L.ssym_match_sharded(self.ctx, comm.ptr, d.ptr, q.ptr, dist_p, index_base, out_idx.data_ptr(),
                                      out_cost.data_ptr() if out_cost is not None else None, flags | nat.OUT_DEVICE)
            nat.check(rc, self.ctx)
            return out_idx, out_cost
        idx = np.zeros(m, dtype=np.uint32)
        cost = np.zeros(m, dtype=np.float64)
        rc = L.ssym_match_sharded(self.ctx, comm.ptr, d.ptr, q.ptr, dist_p, index_base, idx.ctypes.data,
                                  cost.ctypes.data, flags)
        nat.check(rc, self.ctx)
        return idx, cost

    def match_topk(self, d: _Handle, q: _Handle, k: int, distance=None, index_base: int = 0,
                   force_exact: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """ssym_match_topk: (idx [m][k] uint32, cost [m][k] f64); rows are ordered by
        (|value - distance|, index); missing entries are nat.NO_MATCH / NaN."""
        m = q.n
        dist_p = None
        if distance is not None:
            dist = np.ascontiguousarray(distance, dtype=np.float64)
            if dist.size != m:
                raise ValueError("distance must have one entry per target")
            dist_p = dist.ctypes.data
        idx = np.zeros((m, k), dtype=np.uint32)
        cost = np.zeros((m, k), dtype=np.float64)
        rc = nat.lib().ssym_match_topk(self.ctx, d.ptr, q.ptr, dist_p, k, index_base, idx.ctypes.data,
                                       cost.ctypes.data, nat.DTW_FORCE_EXACT if force_exact else 0)
        nat.check(rc, self.ctx)
        return idx, cost

    def match_batch(self, d: _Handle, feats, offsets, distance=None):
        """ssym_match_batch: pack host targets, match, release."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        f = np.ascontiguousarray(feats, dtype=self.np_dtype).reshape(-1)
        m = off.size - 1
        idx = np.zeros(m, dtype=np.uint32)
        cost = np.zeros(m, dtype=np.float64)
        dist_p = None
        if distance is not None:
            dist = np.ascontiguousarray(distance, dtype=np.float64)
            dist_p = dist.ctypes.data
        rc = nat.lib().ssym_match_batch(self.ctx, d.ptr, f.ctypes.data, off.ctypes.data, m, dist_p,
                                        idx.ctypes.data, cost.ctypes.data)
        nat.check(rc, self.ctx)
        return idx, cost

    def match_one(self, d: _Handle, feats, distance: float):
        f = np.ascontiguousarray(feats, dtype=self.np_dtype).reshape(-1)
        if f.size % d.dim:
            raise ValueError("query is not a whole number of frames")
        idx = ctypes.c_uint32(0)
        cost = ctypes.c_double(0.0)
        rc = nat.lib().ssym_match_one(self.ctx, d.ptr, f.ctypes.data, f.size // d.dim,
                                      float(distance), ctypes.byref(idx), ctypes.byref(cost))
        nat.check(rc, self.ctx)
        return int(idx.value), float(cost.value)

    def chain(self, d: _Handle, start_feats, distances) -> Tuple[np.ndarray, np.ndarray]:
        """ssym_chain: from_distances (src/sound.rs:405-417) without a host round trip per step.
        Returns (idx [n_steps], cost [n_steps]); idx[i] is the dictionary entry matched at step i."""
        f = np.ascontiguousarray(start_feats, dtype=self.np_dtype).reshape(-1)
        if f.size % d.dim:
            raise ValueError("start is not a whole number of frames")
        dist = np.ascontiguousarray(distances, dtype=np.float64).reshape(-1)
        idx = np.zeros(dist.size, dtype=np.uint32)
        cost = np.zeros(dist.size, dtype=np.float64)
        rc = nat.lib().ssym_chain(self.ctx, d.ptr, f.ctypes.data, f.size // d.dim, dist.ctypes.data, dist.size,
                                  idx.ctypes.data, cost.ctypes.data)
        nat.check(rc, self.ctx)
        return idx, cost

    def pair_matrix(self, d: _Handle, q: _Handle, exact: bool = False, step: str = "symmetric") -> np.ndarray:
        """ssym_pair_matrix; step="paced": ssym_pair_matrix_step with SSYM_STEP_PACED, the [n_sources][n_targets] costs
        of "Paced matching" (always exact: `exact` is not looked at)."""
        which = _spot_step(step)
        out = np.zeros((d.n, q.n), dtype=np.float64)
        if which == nat.STEP_SYMMETRIC:
            rc = nat.lib().ssym_pair_matrix(self.ctx, d.ptr, q.ptr, 1 if exact else 0, out.ctypes.data)
        else:
            rc = nat.lib().ssym_pair_matrix_step(self.ctx, d.ptr, q.ptr, which, out.ctypes.data)
        nat.check(rc, self.ctx)
        return out

    def dtw_align_sizes(self, d: _Handle, q: _Handle, src_idx, tgt_idx=None, index_base: int = 0, spans=None):
        """ssym_dtw_align_sizes: (path_offsets, map_offsets), n_pairs + 1 uint64 each -- the room a pair's path
        (Fa + Fb - 1 cells) and map (Fb entries) can need.  Host arithmetic.  spans=(first, last):
        ssym_dtw_align_spans_sizes, Fa the span's frames."""
        src, tgt = _align_indices(src_idx, tgt_idx)
        spans = _align_spans(spans, src.size)
        p_off = np.zeros(src.size + 1, dtype=np.uint64)
        m_off = np.zeros(src.size + 1, dtype=np.uint64)
        if spans is None:
            rc = nat.lib().ssym_dtw_align_sizes(d.ptr, q.ptr, src.ctypes.data, tgt.ctypes.data if tgt is not None else None,
                                                src.size, index_base, p_off.ctypes.data, m_off.ctypes.data)
        else:
            rc = nat.lib().ssym_dtw_align_spans_sizes(d.ptr, q.ptr, src.ctypes.data, tgt.ctypes.data if tgt is not None else None,
                                                      spans[0].ctypes.data, spans[1].ctypes.data, src.size, index_base,
                                                      p_off.ctypes.data, m_off.ctypes.data)
        if rc == nat.SSYM_E_EMPTY_DICT:
            raise nat.EmptyDictionaryError(rc, "empty dictionary")
        if rc != nat.SSYM_OK:
            raise nat.SsymError(rc, "ssym_dtw_align_sizes: an index is outside its set, the sets do not go together, or a "
                                    "span is not inside its segment")
        return p_off, m_off

    def _align_call(self, which, head, tail, spans=None):
        """ssym_dtw_align for the symmetric pattern, ssym_dtw_align_step for any other; with spans ssym_dtw_align_spans,
        which takes the spans behind the indices and the step behind index_base."""
        if spans is not None:
            return nat.lib().ssym_dtw_align_spans(*head[:5], spans[0].ctypes.data, spans[1].ctypes.data, *head[5:], which, *tail)
        if which == nat.STEP_SYMMETRIC:
            return nat.lib().ssym_dtw_align(*head, *tail)
        return nat.lib().ssym_dtw_align_step(*head, which, *tail)

    def dtw_align(self, d: _Handle, q: _Handle, src_idx, tgt_idx=None, index_base: int = 0, want_map: bool = True,
                  step: str = "symmetric", spans=None):
        """ssym_dtw_align: the optimal warping path of every listed pair (source src_idx[p] - index_base, target
        tgt_idx[p], or target p without tgt_idx), by the definition in include/soundsym_amd.h.  Returns (cost f64
        [n], lengths uint32 [n], paths, maps): paths[p] is an (L, 2) uint32 array of (source frame, target frame)
        cells in forward order, maps[p] a (Fb,) uint32 array with the smallest source frame of every target frame (or
        None without want_map).  A pair without a finite cost has length 0, an empty path and an empty map.  The
        arrays are views into one buffer each.  step="paced": ssym_dtw_align_step with SSYM_STEP_PACED ("Paced
        alignment": one cell per target frame, steps of 0, 1 or 2 source frames, never two 0 steps in a row; a pair
        whose shape admits no such path has length 0); "symmetric" is ssym_dtw_align itself.  spans=(first, last), one
        inclusive range of source frames per pair: ssym_dtw_align_spans -- the pair is (those frames of the segment,
        target), cells and maps count from the span's first frame, and first = last = NO_MATCH is a pair without a path."""
        which = _spot_step(step)
        src, tgt = _align_indices(src_idx, tgt_idx)
        n = src.size
        spans = _align_spans(spans, n)
        p_off, m_off = (self.dtw_align_sizes(d, q, src, tgt, index_base) if spans is None else
                        self.dtw_align_sizes(d, q, src, tgt, index_base, spans))
        cost = np.zeros(n, dtype=np.float64)
        length = np.zeros(n, dtype=np.uint32)
        path = np.zeros((int(p_off[-1]), 2), dtype=np.uint32)
        fmap = np.zeros(int(m_off[-1]), dtype=np.uint32) if want_map else None
        head = (self.ctx, d.ptr, q.ptr, src.ctypes.data, tgt.ctypes.data if tgt is not None else None, n, index_base)
        tail = (cost.ctypes.data, length.ctypes.data, p_off.ctypes.data, path.ctypes.data,
                m_off.ctypes.data if want_map else None, fmap.ctypes.data if want_map else None, 0)
        nat.check(Engine._align_call(self, which, head, tail, spans), self.ctx)
        paths = [path[int(p_off[p]):int(p_off[p]) + int(length[p])] for p in range(n)]
        maps = None
        if want_map:
            maps = [fmap[int(m_off[p]):int(m_off[p + 1])] if length[p] else fmap[0:0] for p in range(n)]
        return cost, length, paths, maps

    def dtw_align_device(self, d: _Handle, q: _Handle, src_idx, tgt_idx=None, index_base: int = 0, step: str = "symmetric",
                         spans=None):
        """ssym_dtw_align with SSYM_OUT_DEVICE: the outputs stay in device memory (torch tensors; torch only owns the
        memory).  Returns (cost f64 [n], lengths i32 [n], paths i32 [cells * 2], maps i32 [map entries], path_offsets,
        map_offsets); the 32-bit tensors hold the call's u32 values.  maps, lengths and map_offsets are what
        reconstruct_warped takes.  step and spans as for dtw_align; the maps of a spans call go with windows= there."""
        which = _spot_step(step)
        src, tgt = _align_indices(src_idx, tgt_idx)
        n = src.size
        spans = _align_spans(spans, n)
        p_off, m_off = (self.dtw_align_sizes(d, q, src, tgt, index_base) if spans is None else
                        self.dtw_align_sizes(d, q, src, tgt, index_base, spans))
        (cost, pc), (length, pl), (path, pp), (fmap, pm) = (
            _output(self.device, (rows,), t) for rows, t in ((n, np.float64), (n, np.uint32), (2 * int(p_off[-1]), np.uint32),
                                                            (int(m_off[-1]), np.uint32)))
        head = (self.ctx, d.ptr, q.ptr, src.ctypes.data, tgt.ctypes.data if tgt is not None else None, n, index_base)
        tail = (pc, pl, p_off.ctypes.data, pp, m_off.ctypes.data, pm, nat.OUT_DEVICE)
        nat.check(Engine._align_call(self, which, head, tail, spans), self.ctx)
        return cost, length, path, fmap, p_off, m_off

    def _dtw_spot(self, d, q, src_idx, tgt_idx, index_base, step, on_device):
        """dtw_spot and, with on_device, dtw_spot_device.  The argument checks come before self is touched, and the public
        methods call this through the class: a call with bad arguments fails as ValueError whatever self is."""
        which = _spot_step(step)
        src, tgt = _align_indices(src_idx, tgt_idx)
        n, device = src.size, self.device if on_device else None
        (cost, pc), (start, ps), (end, pe) = (_output(device, (n,), t) for t in (np.float64, np.uint32, np.uint32))
        head = (self.ctx, d.ptr, q.ptr, src.ctypes.data, tgt.ctypes.data if tgt is not None else None, n, index_base)
        tail = (pc, ps, pe, 0 if device is None else nat.OUT_DEVICE)
        if which == nat.STEP_SYMMETRIC:
            rc = nat.lib().ssym_dtw_spot(*head, *tail)
        else:
            rc = nat.lib().ssym_dtw_spot_step(*head, which, *tail)
        nat.check(rc, self.ctx)
        return cost, start, end

    def _dtw_spot_all(self, d, q, src_idx, tgt_idx, index_base, max_spots, max_cost, step, on_device):
        """dtw_spot_all and, with on_device, dtw_spot_all_device; called as _dtw_spot is."""
        which = _spot_step(step)
        src, tgt = _align_indices(src_idx, tgt_idx)
        k, mc = _spot_all_args(src, max_spots, max_cost)
        n, device = src.size, self.device if on_device else None
        (count, pn), (cost, pc), (start, ps), (end, pe) = (
            _output(device, shape, t) for shape, t in (((n,), np.uint32), ((n, k), np.float64), ((n, k), np.uint32),
                                                       ((n, k), np.uint32)))
        head = (self.ctx, d.ptr, q.ptr, src.ctypes.data, tgt.ctypes.data if tgt is not None else None, n, index_base)
        tail = (k, mc.ctypes.data if mc is not None else None, pn, pc, ps, pe, 0 if device is None else nat.OUT_DEVICE)
        if which == nat.STEP_SYMMETRIC:
            rc = nat.lib().ssym_dtw_spot_all(*head, *tail)
        else:
            rc = nat.lib().ssym_dtw_spot_all_step(*head, which, *tail)
        nat.check(rc, self.ctx)
        return count, cost, start, end

    def dtw_spot(self, d: _Handle, q: _Handle, src_idx, tgt_idx=None, index_base: int = 0, step: str = "symmetric"):
        """ssym_dtw_spot (subsequence DTW; dtw engines without a band): for every listed pair (source src_idx[p] -
        index_base, target tgt_idx[p], or target p without tgt_idx) the span of the source's frames the target aligns
        with best, by the definition in include/soundsym_amd.h.  Returns (cost f64 [n], start uint32 [n], end uint32
        [n]); end is inclusive; a pair without a spot has cost +inf and start = end = NO_MATCH.  The cost is not
        normalised by any length.  step="paced": ssym_dtw_spot_step with SSYM_STEP_PACED ("Paced spotting": every path
        has as many cells as the target has frames, so cost / frames is a mean per-frame distance); "symmetric" is
        ssym_dtw_spot itself."""
        return Engine._dtw_spot(self, d, q, src_idx, tgt_idx, index_base, step, on_device=False)

    def dtw_spot_device(self, d: _Handle, q: _Handle, src_idx, tgt_idx=None, index_base: int = 0, step: str = "symmetric"):
        """ssym_dtw_spot with SSYM_OUT_DEVICE: (cost f64 [n], start i32 [n], end i32 [n]) as torch tensors in device
        memory (torch only owns the memory; the 32-bit tensors hold the call's u32 values).  step as for dtw_spot."""
        return Engine._dtw_spot(self, d, q, src_idx, tgt_idx, index_base, step, on_device=True)

    def dtw_spot_all(self, d: _Handle, q: _Handle, src_idx, tgt_idx=None, index_base: int = 0, max_spots: int = 8,
                     max_cost=None, step: str = "symmetric"):
        """ssym_dtw_spot_all: for every listed pair (as in dtw_spot) up to max_spots (1 ... 64) pairwise disjoint spans
        of the source the target aligns with, best first, by the definition in include/soundsym_amd.h ("Occurrences").
        max_cost: a scalar or one value per pair; an occurrence costs at most that.  Returns (count uint32 [n], cost f64
        [n, K], start uint32 [n, K], end uint32 [n, K]); slots from count[p] on hold +inf and NO_MATCH.  step="paced":
        ssym_dtw_spot_all_step with SSYM_STEP_PACED (costs and max_cost stay sums); "symmetric" is ssym_dtw_spot_all
        itself."""
        return Engine._dtw_spot_all(self, d, q, src_idx, tgt_idx, index_base, max_spots, max_cost, step, on_device=False)

    def dtw_spot_all_device(self, d: _Handle, q: _Handle, src_idx, tgt_idx=None, index_base: int = 0, max_spots: int = 8,
                            max_cost=None, step: str = "symmetric"):
        """ssym_dtw_spot_all with SSYM_OUT_DEVICE: (count i32 [n], cost f64 [n, K], start i32 [n, K], end i32 [n, K]) as
        torch tensors in device memory (torch only owns the memory; the 32-bit tensors hold the call's u32 values).  step as
        for dtw_spot_all."""
        return Engine._dtw_spot_all(self, d, q, src_idx, tgt_idx, index_base, max_spots, max_cost, step, on_device=True)

    def spot_queries(self, d: _Handle, q: _Handle, index_base: int = 0, step: str = "symmetric"):
        """ssym_spot_queries: every dictionary segment spotted against every target, then the first least cost per
        target over ascending segment index.  Returns (idx uint32 [m] (+ index_base; NO_MATCH where no segment has a
        spot), cost f64 [m], start uint32 [m], end uint32 [m]) -- the span is the winning segment's.  step="paced":
        ssym_spot_queries_step with SSYM_STEP_PACED; "symmetric" is ssym_spot_queries itself."""
        which = _spot_step(step)
        m = q.n
        idx = np.zeros(m, dtype=np.uint32)
        cost = np.zeros(m, dtype=np.float64)
        start = np.zeros(m, dtype=np.uint32)
        end = np.zeros(m, dtype=np.uint32)
        if which == nat.STEP_SYMMETRIC:
            rc = nat.lib().ssym_spot_queries(self.ctx, d.ptr, q.ptr, index_base, idx.ctypes.data, cost.ctypes.data,
                                             start.ctypes.data, end.ctypes.data, 0)
        else:
            rc = nat.lib().ssym_spot_queries_step(self.ctx, d.ptr, q.ptr, index_base, which, idx.ctypes.data,
                                                  cost.ctypes.data, start.ctypes.data, end.ctypes.data, 0)
        nat.check(rc, self.ctx)
        return idx, cost, start, end

    def dtw_cover(self, d: _Handle, q: _Handle, piece_penalty: float = 0.0, on_device: bool = False, gap_cost=None):
        """ssym_dtw_cover (dtw engines without a band): every target tiled by dictionary segments, cut points and
        segments chosen together so that the paced costs of the pieces sum to the least total over every tiling, by the
        definition in include/soundsym_amd.h ("Cover").  piece_penalty >= 0 is added per piece.  Returns (count uint32
        [m], total f64 [m], src uint32 [F], start uint32 [F], end uint32 [F], cost f64 [F]) with F the target frames of
        the whole query set: target t's pieces lie in slots q.offsets[t] ... q.offsets[t] + count[t] - 1 in ascending
        start, start / end count frames inside the target (end inclusive), unused slots hold NO_MATCH and +inf, a
        target without a cover has count 0 and total +inf.  Costs are sums.  on_device: SSYM_OUT_DEVICE, the six arrays
        as torch tensors in device memory (the 32-bit tensors hold the call's u32 values).
        gap_cost (None: ssym_dtw_cover as it is): ssym_dtw_cover_gaps, "Cover with gaps" -- a target frame may stay
        uncovered at gap_cost >= 0 per frame (+inf: never, the results of None).  A gap frame is reported frame by frame
        as the piece (nat.COVER_GAP, e, e, gap_cost); no piece_penalty is charged on it and a piece wins a tie.  With a
        finite gap_cost every target with a frame has a cover."""
        penalty, gap = _cover_penalty(piece_penalty), _cover_gap_cost(gap_cost)
        m, frames = q.n, int(q.offsets[-1])
        device = self.device if on_device else None
        (count, pn), (total, pt), (src, ps), (start, pa), (end, pe), (cost, pc) = (
            _output(device, (rows,), t) for rows, t in ((m, np.uint32), (m, np.float64), (frames, np.uint32),
                                                        (frames, np.uint32), (frames, np.uint32), (frames, np.float64)))
        flags = 0 if device is None else nat.OUT_DEVICE
        if gap is None:
            rc = nat.lib().ssym_dtw_cover(self.ctx, d.ptr, q.ptr, penalty, flags, pn, pt, ps, pa, pe, pc)
        else:
            rc = nat.lib().ssym_dtw_cover_gaps(self.ctx, d.ptr, q.ptr, penalty, gap, flags, pn, pt, ps, pa, pe, pc)
        nat.check(rc, self.ctx)
        return count, total, src, start, end, cost

    def dtw_mosaic(self, d: _Handle, q: _Handle, piece_penalty: float = 0.0, gap_cost=None, on_device: bool = False):
        """ssym_dtw_mosaic (dtw engines without a band): every target tiled by pieces, each piece any span of any
        dictionary segment aligned under the paced pattern; cuts, segments, spans and paths chosen together, by the
        definition in include/soundsym_amd.h ("Mosaic").  Neither side needs cutting beforehand and a segment may be
        as long as a dictionary holds.  piece_penalty >= 0 is charged once per piece; gap_cost (None: no gaps) >= 0
        is the price of a target frame left uncovered.  Returns (count uint32 [m], total f64 [m], start uint32 [F],
        src uint32 [F], frame uint32 [F], frame_cost f64 [F]) with F the target frames of the whole query set: target
        t's piece and gap-frame starts lie in start[q.offsets[t] ... q.offsets[t] + count[t] - 1], ascending (unused
        slots NO_MATCH); src / frame / frame_cost hold the segment, the frame within it and c for every target frame
        (a gap frame: nat.COVER_GAP, NO_MATCH, gap_cost; without a mosaic NO_MATCH, NO_MATCH, +inf: count 0, total
        +inf).  on_device: SSYM_OUT_DEVICE, the six arrays as torch tensors in device memory."""
        penalty, gap = _cover_penalty(piece_penalty), _cover_gap_cost(gap_cost)
        m, frames = q.n, int(q.offsets[-1])
        device = self.device if on_device else None
        (count, pn), (total, pt), (start, pa), (src, ps), (frame, pf), (cost, pc) = (
            _output(device, (rows,), t) for rows, t in ((m, np.uint32), (m, np.float64), (frames, np.uint32),
                                                        (frames, np.uint32), (frames, np.uint32), (frames, np.float64)))
        flags = 0 if device is None else nat.OUT_DEVICE
        rc = nat.lib().ssym_dtw_mosaic(self.ctx, d.ptr, q.ptr, penalty, float("inf") if gap is None else gap, flags,
                                       pn, pt, pa, ps, pf, pc)
        nat.check(rc, self.ctx)
        return count, total, start, src, frame, cost

    # -- feature front-end (F3) --------------------------------------------------------------
    def mfcc(self, samples, sample_rate: float, ncoeffs: int = 12, f_lo: float = 100.0, f_hi: float = 8000.0,
             pad_tail: bool = False, want_mean: bool = False):
        """ssym_mfcc: [frames][ncoeffs] f64 (analyze_mfccs, src/sound.rs:215-242; parity unpinned),
        optionally with the per-coefficient mean (analyze_mean_mfccs, :271-286)."""
        x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        flags = nat.MFCC_PAD_TAIL if pad_tail else 0
        t = ctypes.c_uint64(0)
        nat.check(nat.lib().ssym_mfcc_num_frames(x.size, flags, ctypes.byref(t)), self.ctx)
        out = np.zeros((int(t.value), ncoeffs), dtype=np.float64)
        mean = np.zeros(ncoeffs, dtype=np.float64)
        rc = nat.lib().ssym_mfcc(self.ctx, x.ctypes.data if x.size else None, x.size, float(sample_rate), ncoeffs,
                                 float(f_lo), float(f_hi), flags, out.ctypes.data if out.size else None,
                                 mean.ctypes.data if want_mean else None)
        nat.check(rc, self.ctx)
        return (out, mean) if want_mean else out

    def mfcc_batch(self, samples, sample_offsets, sample_rate: float, ncoeffs: int = 12, f_lo: float = 100.0,
                   f_hi: float = 8000.0, pad_tail: bool = False, want_mean: bool = False, out=None):
        """ssym_mfcc_batch: the MFCCs of the sounds samples[sample_offsets[i]:sample_offsets[i+1]] in one call,
        each bit for bit what `mfcc` gives for that sound alone.  Returns (feats [F][ncoeffs], frame_offsets [n+1]
        u64), plus the per-sound means [n][ncoeffs] (NaN for a sound without frames) when asked.  `out`: a caller's
        contiguous f64 device tensor of F * ncoeffs values (SSYM_OUT_DEVICE), returned in place of feats."""
        x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        off = np.ascontiguousarray(sample_offsets, dtype=np.uint64).reshape(-1)
        if off.size < 1 or np.any(np.diff(off.astype(np.int64)) < 0) or int(off[-1]) > x.size:
            raise ValueError("sample_offsets: n_sounds + 1 non-decreasing sample offsets within `samples`")
        n = off.size - 1
        flags = nat.MFCC_PAD_TAIL if pad_tail else 0
        nframes = sum(self.mfcc_num_frames(int(off[i + 1] - off[i]), pad_tail) for i in range(n))
        fo = np.zeros(n + 1, dtype=np.uint64)
        mean = np.zeros((n, ncoeffs), dtype=np.float64)
        if out is not None:
            if not _is_device_tensor(out) or not out.is_contiguous() or out.numel() != nframes * ncoeffs or \
                    str(out.dtype) != "torch.float64":
                raise ValueError(f"out: a contiguous f64 device tensor of {nframes * ncoeffs} values")
            feats, dst, flags = out, out.data_ptr() if nframes else None, flags | nat.OUT_DEVICE
        else:
            feats = np.zeros((nframes, ncoeffs), dtype=np.float64)
            dst = feats.ctypes.data if nframes else None
        nat.check(nat.lib().ssym_mfcc_batch(self.ctx, x.ctypes.data if x.size else None, off.ctypes.data, n,
                                            float(sample_rate), ncoeffs, float(f_lo), float(f_hi), flags,
                                            fo.ctypes.data, dst, mean.ctypes.data if want_mean and n else None),
                  self.ctx)
        return (feats, fo, mean) if want_mean else (feats, fo)

    def stream(self, n_lanes: int, sample_rate: float, ncoeffs: int = 12, f_lo: float = 100.0, f_hi: float = 8000.0,
               capacity: int = 0) -> Stream:
        """ssym_stream_create: `n_lanes` growing sounds with resident analysis; `capacity`: samples reserved per lane."""
        out = ctypes.c_void_p()
        nat.check(nat.lib().ssym_stream_create(self.ctx, int(n_lanes), float(sample_rate), int(ncoeffs), float(f_lo),
                                               float(f_hi), int(capacity), ctypes.byref(out)), self.ctx)
        return Stream(self, out.value, int(n_lanes), int(ncoeffs), float(sample_rate))

    def spotter(self, q: _Handle, n_lanes: int = 1, max_cost=None, step: str = "symmetric") -> Spotter:
        """ssym_spotter_create: the targets of `q` watched in `n_lanes` growing sources (dtw engines without a band).
        max_cost: a scalar or one value per target; an event costs at most that (a sum, whatever the step).
        step="paced": ssym_spotter_create_step with SSYM_STEP_PACED ("Paced watching": slope-bounded spans, targets of
        at most 2048 frames); "symmetric" is ssym_spotter_create itself."""
        which = _spot_step(step)
        lanes, mc = _spotter_args(q, n_lanes, max_cost)
        out = ctypes.c_void_p()
        head = (self.ctx, q.ptr, lanes, mc.ctypes.data if mc is not None else None)
        if which == nat.STEP_SYMMETRIC:
            rc = nat.lib().ssym_spotter_create(*head, ctypes.byref(out))
        else:
            rc = nat.lib().ssym_spotter_create_step(*head, which, ctypes.byref(out))
        nat.check(rc, self.ctx)
        return Spotter(self, out.value, q, lanes, step)

    def coverer(self, d: _Handle, n_lanes: int = 1, piece_penalty: float = 0.0, gap_cost=None) -> Coverer:
        """ssym_coverer_create: `n_lanes` growing targets covered live by the segments of `d` (dtw engines without a
        band; "Live cover").  piece_penalty >= 0 is added per piece, as for dtw_cover.  gap_cost (None:
        ssym_coverer_create as it is): ssym_coverer_create_gaps -- frames may stay uncovered at gap_cost each, as for
        dtw_cover; a NaN or infinite frame then becomes a gap frame and the lane goes on."""
        penalty, gap = _cover_penalty(piece_penalty), _cover_gap_cost(gap_cost)
        lanes = int(n_lanes)
        if lanes < 1:
            raise ValueError("n_lanes must be at least 1")
        out = ctypes.c_void_p()
        if gap is None:
            rc = nat.lib().ssym_coverer_create(self.ctx, d.ptr, lanes, penalty, ctypes.byref(out))
        else:
            rc = nat.lib().ssym_coverer_create_gaps(self.ctx, d.ptr, lanes, penalty, gap, ctypes.byref(out))
        nat.check(rc, self.ctx)
        return Coverer(self, out.value, d, lanes, penalty, gap)

    def mosaicker(self, d: _Handle, n_lanes: int = 1, piece_penalty: float = 0.0, gap_cost=None) -> Mosaicker:
        """ssym_mosaicker_create: `n_lanes` growing targets tiled live by free spans of the recordings of `d` (dtw engines
        without a band; "Live mosaic").  piece_penalty >= 0 is added per piece and gap_cost (None or +inf: no gaps) per
        frame left uncovered, as for dtw_mosaic; with a gap_cost a NaN frame becomes a gap frame and the lane goes on."""
        penalty, gap = _cover_penalty(piece_penalty), _cover_gap_cost(gap_cost)
        lanes = int(n_lanes)
        if lanes < 1:
            raise ValueError("n_lanes must be at least 1")
        out = ctypes.c_void_p()
        nat.check(nat.lib().ssym_mosaicker_create(self.ctx, d.ptr, lanes, penalty, float("inf") if gap is None else gap,
                                                  ctypes.byref(out)), self.ctx)
        return Mosaicker(self, out.value, d, lanes, penalty, gap)

    def resynth(self, samples_store, n_lanes: int = 1, search: int = 0) -> Resynth:
        """ssym_resynth_create: `n_lanes` lanes of live resynthesis from the resident samples `samples_store` (Engine.samples;
        "Live resynthesis").  search: reconstruct_wsola's, 0 ... 512 samples; 0 is the plain warp."""
        search = _wsola_search(search)
        lanes = int(n_lanes)
        if lanes < 1:
            raise ValueError("n_lanes must be at least 1")
        out = ctypes.c_void_p()
        nat.check(nat.lib().ssym_resynth_create(self.ctx, samples_store.ptr, lanes, search, ctypes.byref(out)), self.ctx)
        return Resynth(self, out.value, samples_store, lanes, search)

    def follower(self, n_lanes: int = 1, max_gain=FOLLOW_MAX_GAIN) -> Follower:
        """ssym_follower_create: `n_lanes` lanes (1 ... 16 384) of live envelope following ("Live envelope following");
        max_gain as follow_envelope's, finite and at least 1.  Any engine: nothing here aligns."""
        gain = _follow_max_gain(max_gain)
        lanes = int(n_lanes)
        if lanes < 1 or lanes != n_lanes or isinstance(n_lanes, bool):
            raise ValueError("n_lanes must be a whole number, at least 1")
        if lanes > FOLLOWER_MAX_LANES:
            raise ValueError(f"n_lanes must be at most {FOLLOWER_MAX_LANES}")
        out = ctypes.c_void_p()
        nat.check(nat.lib().ssym_follower_create(self.ctx, lanes, gain, ctypes.byref(out)), self.ctx)
        return Follower(self, out.value, lanes, gain)

    @staticmethod
    def mfcc_num_frames(n_samples: int, pad_tail: bool = False) -> int:
        """ssym_mfcc_num_frames (host arithmetic, no device)."""
        t = ctypes.c_uint64(0)
        nat.check(nat.lib().ssym_mfcc_num_frames(int(n_samples), nat.MFCC_PAD_TAIL if pad_tail else 0,
                                                 ctypes.byref(t)))
        return int(t.value)

    def sequence_distances(self, feats, frame_offsets, dim: int, want_mean: bool = False, want_sim: bool = False):
        """ssym_sequence_distances: SoundSequence::new's distances (src/sound.rs:392-398), cosine_sim_angular of the
        mean features of each pair of neighbouring blocks: dist [n-1], plus the means [n][dim] and the clamped
        similarities [n-1] when asked.  feats: host array or f64 device tensor, frame-major."""
        off = np.ascontiguousarray(frame_offsets, dtype=np.uint64).reshape(-1)
        if off.size < 1:
            raise ValueError("frame_offsets: n_sounds + 1 offsets")
        n = off.size - 1
        flags = 0
        if _is_device_tensor(feats):
            if not feats.is_contiguous() or str(feats.dtype) != "torch.float64":
                raise ValueError("feats: a contiguous f64 device tensor")
            ptr, flags = feats.data_ptr() if feats.numel() else None, nat.OUT_DEVICE
        else:
            x = np.ascontiguousarray(feats, dtype=np.float64).reshape(-1)
            ptr = x.ctypes.data if x.size else None
        npairs = max(n - 1, 0)
        mean, sim, dist = np.zeros((n, dim)), np.zeros(npairs), np.zeros(npairs)
        nat.check(nat.lib().ssym_sequence_distances(self.ctx, ptr, off.ctypes.data, n, dim, flags,
                                                    mean.ctypes.data if want_mean and n else None,
                                                    sim.ctypes.data if want_sim and npairs else None,
                                                    dist.ctypes.data if npairs else None), self.ctx)
        res = (dist,)
        if want_mean:
            res += (mean,)
        if want_sim:
            res += (sim,)
        return res if len(res) > 1 else dist

    # -- reconstruction tail (F2) ------------------------------------------------------------
    # partitioner (own definitions, parity unpinned) ------------------------------------------------
    def standardize(self, feats, dim: int) -> np.ndarray:
        """ssym_standardize: per column (x - mean) / sample std, fitted on `feats` itself ([frames][dim] f64)."""
        x = np.ascontiguousarray(feats, dtype=np.float64).reshape(-1)
        n = x.size // dim
        out = np.zeros((n, dim))
        nat.check(nat.lib().ssym_standardize(self.ctx, x.ctypes.data if n else None, n, dim, 0,
                                             out.ctypes.data if n else None), self.ctx)
        return out

    def gmm_train(self, feats, dim: int, init_rows, eps: float = 0.1, max_iters: int = 5,
                  standardize: bool = True) -> "Gmm":
        """ssym_gmm_train: a Gaussian mixture with K = len(init_rows) components started at those frames."""
        x = np.ascontiguousarray(feats, dtype=np.float64).reshape(-1)
        rows = np.ascontiguousarray(init_rows, dtype=np.uint64)
        out = ctypes.c_void_p()
        flags = nat.GMM_STANDARDIZE if standardize else 0
        nat.check(nat.lib().ssym_gmm_train(self.ctx, x.ctypes.data, x.size // dim, dim, rows.size, rows.ctypes.data,
                                           float(eps), int(max_iters), flags, ctypes.byref(out)), self.ctx)
        return Gmm(self, out.value, rows.size, dim)

    def gmm_predict(self, gmm: "Gmm", feats, standardize: bool = True, want_post: bool = False):
        """ssym_gmm_predict: letters [frames] u8 (and the posteriors [frames][K] when asked).  feats: a host array, or
        f64 frames in device memory (a DeviceFrames view or a contiguous device tensor)."""
        if _is_device_tensor(feats):
            return self._gmm_predict_device(gmm, feats, standardize, want_post)
        x = np.ascontiguousarray(feats, dtype=np.float64).reshape(-1)
        n = x.size // gmm.dim
        let = np.zeros(n, dtype=np.uint8)
        post = np.zeros((n, gmm.k)) if want_post else None
        flags = nat.GMM_STANDARDIZE if standardize else 0
        nat.check(nat.lib().ssym_gmm_predict(self.ctx, gmm.ptr, x.ctypes.data if n else None, n, flags,
                                             post.ctypes.data if want_post and n else None,
                                             let.ctypes.data if n else None), self.ctx)
        return (let, post) if want_post else let

    def vote_segments(self, symbols, alphabet: int, depth: int = 5, threshold: int = 4, want_votes: bool = False):
        """ssym_vote_segments: segment lengths (symbols) of a symbol string, optionally with the votes
        ([2][n+1]: frequency expert, entropy expert)."""
        s = np.ascontiguousarray(symbols, dtype=np.uint8).reshape(-1)
        n = s.size
        seg = np.zeros(max(n, 1), dtype=np.uint64)
        votes = np.zeros((2, n + 1), dtype=np.uint32) if want_votes else None
        m = ctypes.c_uint64()
        nat.check(nat.lib().ssym_vote_segments(self.ctx, s.ctypes.data if n else None, n, alphabet, depth, threshold,
                                               0, votes.ctypes.data if want_votes else None, seg.ctypes.data,
                                               ctypes.byref(m)), self.ctx)
        out = seg[:m.value].astype(np.int64)
        return (out, votes) if want_votes else out

    def partition(self, gmm: "Gmm", feats, depth: int = 5, threshold: int = 4, standardize: bool = True) -> np.ndarray:
        """ssym_partition: predict + vote in one call; segment lengths in frames.  feats: a host array, or f64 frames
        in device memory (a DeviceFrames view or a contiguous device tensor), read in place."""
        flags = nat.GMM_STANDARDIZE if standardize else 0
        if _is_device_tensor(feats):
            n, ptr = self._device_frames(feats, gmm.dim)
            flags |= nat.OUT_DEVICE
        else:
            x = np.ascontiguousarray(feats, dtype=np.float64).reshape(-1)
            n = x.size // gmm.dim
            ptr = x.ctypes.data if n else None
        seg = np.zeros(max(n, 1), dtype=np.uint64)
        m = ctypes.c_uint64()
        nat.check(nat.lib().ssym_partition(self.ctx, gmm.ptr, ptr, n, depth, threshold,
                                           flags, seg.ctypes.data, ctypes.byref(m)), self.ctx)
        return seg[:m.value].astype(np.int64)

    @staticmethod
    def _device_frames(feats, dim: int):
        if str(feats.dtype) != "torch.float64" or not feats.is_contiguous() or feats.numel() % dim:
            raise ValueError(f"device features must be contiguous torch.float64 frames of {dim} values")
        n = feats.numel() // dim
        return n, (feats.data_ptr() if n else None)

    def _gmm_predict_device(self, gmm: "Gmm", feats, standardize: bool, want_post: bool):
        """gmm_predict on frames in device memory: with SSYM_OUT_DEVICE the call's outputs are device memory too, so
        they land in torch tensors (torch only owns the memory) and come back as host arrays."""
        import torch
        n, ptr = self._device_frames(feats, gmm.dim)
        dev = torch.device("cuda", self.device)
        let = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        post = torch.empty(max(n, 1) * gmm.k, dtype=torch.float64, device=dev) if want_post else None
        flags = nat.OUT_DEVICE | (nat.GMM_STANDARDIZE if standardize else 0)
        nat.check(nat.lib().ssym_gmm_predict(self.ctx, gmm.ptr, ptr, n, flags,
                                             post.data_ptr() if want_post and n else None,
                                             let.data_ptr() if n else None), self.ctx)
        self.synchronize()
        letters = let[:n].cpu().numpy()
        return (letters, post[:n * gmm.k].cpu().numpy().reshape(n, gmm.k)) if want_post else letters

    # sound descriptors (the pitch side is an own definition, parity unpinned) -------------------------
    def _descriptor_inputs(self, samples, offsets, rate, f_min, f_max, voicing):
        pitch_lags(rate, f_min, f_max, voicing)
        x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if off.size < 1 or np.any(np.diff(off.astype(np.int64)) < 0) or int(off[-1]) > x.size:
            raise ValueError("offsets: n_sounds + 1 non-decreasing sample offsets within `samples`")
        return x, off

    def sound_descriptors(self, samples, offsets, rate: float = 44100.0, f_min: float = 100.0, f_max: float = 500.0,
                          voicing: float = 0.2, voiced_only: bool = False):
        """ssym_sound_descriptors: (max_power [n], pitch_conf [n]) of the sounds samples[offsets[i]:offsets[i+1]]
        (analyze_max_power / analyze_pitch_confidence, src/sound.rs:244-269), one call for the whole batch."""
        x, off = self._descriptor_inputs(samples, offsets, rate, f_min, f_max, voicing)
        n = off.size - 1
        mp, pc = np.zeros(n), np.zeros(n)
        flags = nat.PITCH_VOICED if voiced_only else 0
        nat.check(nat.lib().ssym_sound_descriptors(self.ctx, x.ctypes.data if x.size else None, off.ctypes.data, n,
                                                   float(rate), float(f_min), float(f_max), float(voicing), flags,
                                                   mp.ctypes.data if n else None, pc.ctypes.data if n else None),
                  self.ctx)
        return mp, pc

    def pitch_track(self, samples, offsets, rate: float = 44100.0, f_min: float = 100.0, f_max: float = 500.0,
                    voicing: float = 0.2, voiced_only: bool = False):
        """ssym_pitch_track: (freq, strength, unvoiced, window_offsets): per window the best voiced candidate's
        frequency and strength (0 and 0 without one) and the unvoiced candidate's strength, sound-major; the windows of
        sound i are [window_offsets[i], window_offsets[i+1])."""
        x, off = self._descriptor_inputs(samples, offsets, rate, f_min, f_max, voicing)
        n = off.size - 1
        woff = np.zeros(n + 1, dtype=np.int64)
        w = ctypes.c_uint64(0)
        for i in range(n):
            nat.check(nat.lib().ssym_pitch_num_windows(int(off[i + 1] - off[i]), ctypes.byref(w)))
            woff[i + 1] = woff[i] + int(w.value)
        nw = int(woff[-1])
        freq, strength, unvoiced = np.zeros(nw), np.zeros(nw), np.zeros(nw)
        flags = nat.PITCH_VOICED if voiced_only else 0
        nat.check(nat.lib().ssym_pitch_track(self.ctx, x.ctypes.data if x.size else None, off.ctypes.data, n,
                                             float(rate), float(f_min), float(f_max), float(voicing), flags,
                                             freq.ctypes.data if nw else None, strength.ctypes.data if nw else None,
                                             unvoiced.ctypes.data if nw else None), self.ctx)
        return freq, strength, unvoiced, woff

    def samples(self, samples, sample_offsets):
        """Make the dictionary sounds' samples resident (ssym_samples_create)."""
        smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        off = np.ascontiguousarray(sample_offsets, dtype=np.uint64)
        out = ctypes.c_void_p()
        nat.check(nat.lib().ssym_samples_create(self.ctx, smp.ctypes.data, off.ctypes.data, off.size - 1,
                                                ctypes.byref(out)), self.ctx)
        return _SamplesHandle(self, out.value, off.size - 1)

    def reconstruct(self, smp, idx, out_offsets, want_pcm32: bool = False):
        """Length-fitted, concatenated samples of the matched sounds (ssym_reconstruct)."""
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        off = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        total = int(off[-1])
        out = np.zeros(total, dtype=np.float64)
        pcm = np.zeros(total, dtype=np.int32) if want_pcm32 else None
        nat.check(nat.lib().ssym_reconstruct(self.ctx, smp.ptr, idx.ctypes.data, off.ctypes.data, idx.size,
                                             out.ctypes.data, pcm.ctypes.data if pcm is not None else None),
                  self.ctx)
        return (out, pcm) if want_pcm32 else out

    def reconstruct_warped(self, smp, idx, out_offsets, maps, map_offsets, map_frames, pair_len=None,
                           want_pcm32: bool = False, windows=None):
        """ssym_reconstruct_warped: the matched sounds resynthesised along target-frame -> source-frame maps
        (definition in include/soundsym_amd.h), concatenated.  maps: u32 source frame per target frame, target t from
        map_offsets[t] on, map_frames[t] of them; pair_len: optional, 0 marks a target that takes reconstruct's
        length fit (dtw_align's lengths).  maps and pair_len are numpy arrays, or both device memory (torch CUDA
        tensors of a 32-bit integer type, DeviceFrames-style pointers): dtw_align_device's maps and lengths pass
        straight in.  windows=(first, len), in samples, one per target: ssym_reconstruct_warped_spans -- sound idx[t] is
        only its samples first[t] ... first[t] + len[t] - 1, and the map counts frames from the window's start (what
        dtw_align(spans=) returns).  dtw engines only."""
        out, pcm, _ = _warp_call(self, "reconstruct_warped", smp, idx, out_offsets, maps, map_offsets, map_frames, pair_len,
                                 None, want_pcm32, False, windows)
        return (out, pcm) if want_pcm32 else out

    def reconstruct_wsola(self, smp, idx, out_offsets, maps, map_offsets, map_frames, pair_len=None, search: int = 0,
                          want_pcm32: bool = False, want_pos: bool = False, windows=None):
        """ssym_reconstruct_wsola: reconstruct_warped with every source frame moved by up to `search` samples (0 ... 512)
        to where it continues the frame before it best (definition in include/soundsym_amd.h).  Arguments as
        reconstruct_warped.  Returns the samples, with want_pcm32 also their 32-bit conversion, with want_pos also the
        u64 sample start of every source frame, laid out by map_offsets (slots of targets without a path and slack
        slots hold 2^64 - 1).  search = 0 gives reconstruct_warped's samples bit for bit.  windows as for
        reconstruct_warped (ssym_reconstruct_wsola_spans): lags stay inside the window and the positions count from its
        first sample.  dtw engines only."""
        out, pcm, pos = _warp_call(self, "reconstruct_wsola", smp, idx, out_offsets, maps, map_offsets, map_frames, pair_len,
                                   search, want_pcm32, want_pos, windows)
        res = (out,) + ((pcm,) if want_pcm32 else ()) + ((pos,) if want_pos else ())
        return res if len(res) > 1 else out

    def follow_envelope(self, samples, out_offsets, ref, ref_offsets, max_gain=FOLLOW_MAX_GAIN, want_pcm32: bool = False,
                        want_gains: bool = False, on_device: bool = False):
        """ssym_follow_envelope: reconstructions scaled hop by hop to the loudness of their references (definition in
        include/soundsym_amd.h).  samples: the reconstructions packed by out_offsets; ref: the targets' own samples packed
        by ref_offsets; each a numpy array or f64 device memory (a torch CUDA tensor), as reconstruct_warped accepts maps.
        max_gain: the greatest gain, finite and at least 1.  Returns the samples, with want_pcm32 also their 32-bit
        conversion, with want_gains also the gains g(b) of all targets packed in target order (follow_boundaries gives
        their offsets); numpy arrays, or with on_device torch tensors on the engine's GPU.  Any engine, refcos included."""
        gain = _follow_max_gain(max_gain)
        off = np.ascontiguousarray(out_offsets, dtype=np.uint64).reshape(-1)
        r_off = np.ascontiguousarray(ref_offsets, dtype=np.uint64).reshape(-1)
        if off.size < 1 or r_off.size != off.size:
            raise ValueError("follow_envelope: n + 1 out_offsets and n + 1 ref_offsets for n targets")
        if off[0] != 0 or r_off[0] != 0 or np.any(off[1:] < off[:-1]) or np.any(r_off[1:] < r_off[:-1]):
            raise ValueError("follow_envelope: out_offsets and ref_offsets must start at 0 and not decrease")
        total, n_gains = int(off[-1]), int(follow_boundaries(off)[-1])
        y_ptr, y_dev, keep_y = _follow_samples(samples, total, "samples")
        x_ptr, x_dev, keep_x = _follow_samples(ref, int(r_off[-1]), "ref")
        device = self.device if on_device else None
        (out, p_out), (pcm, p_pcm), (gains, p_gains) = (_output(device, (rows,), t) for rows, t in (
            (total, np.float64), (total if want_pcm32 else 0, np.int32), (n_gains if want_gains else 0, np.float64)))
        flags = ((nat.FOLLOW_SAMPLES_DEVICE if y_dev else 0) | (nat.FOLLOW_REF_DEVICE if x_dev else 0)
                 | (nat.OUT_DEVICE if on_device else 0))
        nat.check(nat.lib().ssym_follow_envelope(self.ctx, y_ptr, off.ctypes.data, off.size - 1, x_ptr, r_off.ctypes.data, gain,
                                                 flags, p_out if total else None, p_pcm if want_pcm32 and total else None,
                                                 p_gains if want_gains and n_gains else None), self.ctx)
        del keep_y, keep_x
        res = (out,) + ((pcm,) if want_pcm32 else ()) + ((gains,) if want_gains else ())
        return res if len(res) > 1 else out

    def merge_shards(self, costs, idx, out_idx, out_cost, distance=None) -> None:
        """costs [G, M] f64, idx [G, M] 32-bit, outputs [M]: torch CUDA tensors on this GPU; distance:
        the per-target distances the shards matched with (host array), or None."""
        g, m = costs.shape
        dist_p = None
        if distance is not None:
            dist = np.ascontiguousarray(distance, dtype=np.float64)
            dist_p = dist.ctypes.data
        nat.check(nat.lib().ssym_merge_shards_at(self.ctx, g, m, costs.data_ptr(), idx.data_ptr(), dist_p,
                                                 out_idx.data_ptr(), out_cost.data_ptr()), self.ctx)

    def timings(self) -> dict:
        t = nat.Timings()
        nat.check(nat.lib().ssym_get_timings(self.ctx, ctypes.byref(t)), self.ctx)
        return t.as_dict()

    def synchronize(self) -> None:
        nat.check(nat.lib().ssym_ctx_synchronize(self.ctx), self.ctx)
