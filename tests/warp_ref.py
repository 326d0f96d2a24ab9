"""Plain restatement of warped reconstruction (ssym_reconstruct_warped; DESIGN.md section 2, the comment in
include/soundsym_amd.h) -- test infrastructure, what the GPU is held to bit for bit.

HOP = 256, BIN = 1024, w[m] = 0.5 - 0.5 cos(2 pi m / 1024) built with math.cos.  For one target: n output samples,
x the matched sound's samples, map[0 .. F) its source frame per target frame (any u32 values).  Output sample k has
the taps j with j * HOP <= k < j * HOP + BIN and j < F, visited in ascending j: m = k - j * HOP, p = map[j] * HOP + m,
valid when p < len(x).  num = sum of w[m] * x[p], den = sum of w[m] over the valid taps, both from +0.0, every product
and sum rounded on its own (Python floats are IEEE doubles; nothing here can be contracted).  out[k] = num / den when
den > 0, else +0.0.  F = 0 or a pair without a path: the length fit of src/sound.rs:456-465.
"""
import math

import numpy as np

HOP, BIN = 256, 1024
WINDOW = [0.5 - 0.5 * math.cos(2.0 * math.pi * float(m) / float(BIN)) for m in range(BIN)]
I32_MAX = 2147483647


def length_fit(x, n):
    out = np.zeros(n, dtype=np.float64)
    m = min(len(x), n)
    out[:m] = np.asarray(x, dtype=np.float64)[:m]
    return out


def warp_one_scalar(x, n, fmap, valid=True):
    """One target, sample by sample in Python floats: the definition read aloud (slow; the CPU tests hold warp_one
    to it)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    F = len(fmap)
    if F == 0 or not valid:
        return length_fit(x, n)
    xs, s_len = x.tolist(), int(x.size)
    fm = [int(v) for v in fmap]
    out = np.zeros(n, dtype=np.float64)
    for k in range(n):
        num, den = 0.0, 0.0
        for j in range(max(0, k // HOP - (BIN // HOP - 1)), min(k // HOP, F - 1) + 1):      # ascending target frames
            m = k - j * HOP
            p = fm[j] * HOP + m                                               # Python ints: no wrap
            if p < s_len:
                num = num + WINDOW[m] * xs[p]
                den = den + WINDOW[m]
        out[k] = num / den if den > 0.0 else 0.0
    return out


def warp_one(x, n, fmap, valid=True):
    """One target: n output samples of the sound x warped along fmap (non-negative ints below 2^32).  All samples
    at once, tap slot by tap slot in ascending target frame; numpy rounds `w * x` and `num + ...` separately."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    F = len(fmap)
    if F == 0 or not valid:
        return length_fit(x, n)
    s_len = int(x.size)
    fm = np.asarray(fmap).astype(np.int64)
    win = np.asarray(WINDOW, dtype=np.float64)
    k = np.arange(n, dtype=np.int64)
    num, den = np.zeros(n), np.zeros(n)
    for i in range(BIN // HOP):
        j = k // HOP - (BIN // HOP - 1) + i                   # the i-th frame that can reach sample k, ascending
        m = k - j * HOP                                       # in [0, BIN) whatever j
        ok = (j >= 0) & (j < F)
        p = fm[np.clip(j, 0, F - 1)] * HOP + m                # int64: below 2^41
        ok &= p < s_len
        w = win[m]
        xv = x[np.where(ok, p, 0)] if s_len else np.zeros(n)
        num = np.where(ok, num + w * xv, num)
        den = np.where(ok, den + w, den)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, num / den, 0.0)


def warp(sounds, idx, out_offsets, maps, map_offsets, map_frames, pair_len=None):
    """The whole call: sounds a list of sample arrays, maps one flat array indexed through map_offsets."""
    out_offsets = [int(v) for v in out_offsets]
    out = np.zeros(out_offsets[-1], dtype=np.float64)
    for t in range(len(idx)):
        n = out_offsets[t + 1] - out_offsets[t]
        F = int(map_frames[t])
        m0 = int(map_offsets[t])
        valid = pair_len is None or int(pair_len[t]) != 0
        fmap = maps[m0:m0 + F] if (F and valid) else []
        out[out_offsets[t]:out_offsets[t + 1]] = warp_one(sounds[int(idx[t])], n, fmap, valid)
    return out


def pcm32(samples):
    """`(i32::max_value() as f64 * sample) as i32` (src/sound.rs:139): truncating, saturating, NaN -> 0."""
    x = np.float64(I32_MAX) * np.asarray(samples, dtype=np.float64)
    out = np.zeros(x.shape, dtype=np.int64)
    ok = ~np.isnan(x)
    out[ok] = np.trunc(np.clip(x[ok], -2147483648.0, 2147483647.0)).astype(np.int64)
    return out.astype(np.int32)
