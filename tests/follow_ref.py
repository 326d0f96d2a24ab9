"""Plain restatement of envelope following (ssym_follow_envelope; DESIGN.md section 2 "Envelope following", the comment in
include/soundsym_amd.h) -- test infrastructure, what the GPU is held to bit for bit.

For one target: y[0 .. n) the reconstruction, x[0 .. nx) the reference; x[k] reads +0.0 for k >= nx and x[k] for k >= n is
never read.  HOP = 256, BIN = 1024, w[] the window of warp_ref (mfcc_frame.hpp's table).  J = ceil(n / HOP); boundaries
b = 0 ... J when n > 0, none when n = 0.

  energy  E_s(b) = sum over m = 0 ... 1023 ascending, from +0.0, of w[m] * (s[k] * s[k]), k = (b - 2) * HOP + m, only the m
          with 0 <= k < n; t = s * s; t = w[m] * t; acc = acc + t, each rounded on its own
  gain    g(b) = sqrt(E_x(b) / E_y(b)); NaN: 1.0; else above max_gain: max_gain
  sample  j = k // HOP, f = (k - j * HOP) / 256.0, a = g(j) * (1.0 - f), c = g(j + 1) * f, out[k] = y[k] * (a + c)
  pcm     warp_ref.pcm32(out)

energies_scalar reads that aloud in Python floats.  energies does all boundaries at once: a term outside [0, n) is put in
as +0.0 instead of being left out -- the sum starts at +0.0 and every term is >= +0.0 or NaN, so acc is never -0.0 and
acc + (+0.0) has acc's bits; np.cumsum along an axis is a serial sum.

What follows from the definition (tests/test_follow_ref.py holds the restatement to it, tests/test_gpu_follow_shapes.py
the GPU):
  1. x = y: g = 1 everywhere, out has y's bits.  y = x / 2^p with max_gain >= 2^p: g = 2^p, out has x's bits (scaling by a
     power of two is exact in every term as long as nothing is subnormal).  y = x / 32, max_gain = 8: g = 8 everywhere.
  2. n = 8192, y = x / 2 below sample 4096 and x / 16 from it, max_gain = 32: g(b) = 2 for b <= 14, 16 for b >= 18; out[k]
     has x[k]'s bits for k <= 3584 and k >= 4608.
  3. y = c x with 1 / max_gain < c: |out - x| <= 2^-40 |x| (two sums of at most 1024 non-negative terms, a division, a
     square root and three products: under 1100 units of roundoff, 1100 * 2^-53 < 2^-42).
  4. y = 0 under a sounding x: g = max_gain, out = +0.0.  x = 0: g = 0, out = +-0.0.  Both silent: g = 1.
  5. A NaN in y: g = 1 on the at most four boundaries whose window holds it, out NaN at that sample alone.  An infinity
     in x: max_gain on those boundaries -- but for the one whose window starts at that very sample, if there is one:
     w[0] = 0 and 0 * inf is NaN, so g = 1 there.  No other target's samples matter.
"""
import numpy as np

import warp_ref
from warp_ref import BIN, HOP, WINDOW, pcm32  # noqa: F401

MAX_GAIN = 8.0
LENGTHS = (0, 1, 2, 255, 256, 257, 511, 512, 513, 1000, 4097)      # the lengths the CPU tests run
BOUND = 2.0 ** -40                                                   # consequence 3


def boundaries(n) -> int:
    """B of a target of n samples."""
    n = int(n)
    return (n + HOP - 1) // HOP + 1 if n > 0 else 0


def gain_offsets(out_offsets) -> np.ndarray:
    """Where target t's gains start in the packed gain array: n + 1 int64."""
    off = [int(v) for v in out_offsets]
    return np.concatenate([[0], np.cumsum([boundaries(b - a) for a, b in zip(off[:-1], off[1:])])]).astype(np.int64)


def fitted(x, n) -> np.ndarray:
    """x as the definition reads it beside n samples of y: +0.0 from len(x) on, nothing at or beyond n."""
    return warp_ref.length_fit(np.ascontiguousarray(x, dtype=np.float64).reshape(-1), int(n))


def energies_scalar(s) -> np.ndarray:
    """E_s(b), b = 0 ... J, of n = len(s) samples: the definition read aloud (slow; the CPU tests hold energies to it)."""
    v = np.ascontiguousarray(s, dtype=np.float64).tolist()
    n = len(v)
    out = np.zeros(boundaries(n), dtype=np.float64)
    for b in range(out.size):
        acc = 0.0
        for m in range(BIN):
            k = (b - 2) * HOP + m
            if 0 <= k < n:
                t = v[k] * v[k]
                t = WINDOW[m] * t
                acc = acc + t
        out[b] = acc
    return out


def energies(s) -> np.ndarray:
    """E_s(b), b = 0 ... J, of n = len(s) samples, all boundaries at once."""
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
    n, B = int(s.size), boundaries(s.size)
    if B == 0:
        return np.zeros(0, dtype=np.float64)
    k = (np.arange(B, dtype=np.int64)[:, None] - 2) * HOP + np.arange(BIN, dtype=np.int64)[None, :]
    ok = (k >= 0) & (k < n)
    v = s[np.clip(k, 0, n - 1)]
    with np.errstate(all="ignore"):
        t = v * v
        t = np.asarray(WINDOW, dtype=np.float64)[None, :] * t
        t = np.where(ok, t, 0.0)
        return np.cumsum(np.concatenate([np.zeros((B, 1)), t], axis=1), axis=1)[:, -1]


def gains(y, x, max_gain=MAX_GAIN) -> np.ndarray:
    """g(b), b = 0 ... J."""
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    ey, ex = energies(y), energies(fitted(x, y.size))
    with np.errstate(all="ignore"):
        g = np.sqrt(ex / ey)
    return np.where(np.isnan(g), 1.0, np.where(g > max_gain, np.float64(max_gain), g))


def apply(y, g) -> np.ndarray:
    """out[k] of the samples y under the gains g."""
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if y.size == 0:
        return np.zeros(0, dtype=np.float64)
    k = np.arange(y.size, dtype=np.int64)
    j = k // HOP
    f = (k - j * HOP).astype(np.float64) / 256.0
    with np.errstate(all="ignore"):
        a = g[j] * (1.0 - f)
        c = g[j + 1] * f
        return y * (a + c)


def follow_one(y, x, max_gain=MAX_GAIN):
    """One target: (out, g)."""
    g = gains(y, x, max_gain)
    return apply(y, g), g


def follow(samples, out_offsets, ref, ref_offsets, max_gain=MAX_GAIN):
    """The whole call: (out_samples, out_pcm32, out_gain)."""
    samples = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
    ref = np.ascontiguousarray(ref, dtype=np.float64).reshape(-1)
    off, r_off = [int(v) for v in out_offsets], [int(v) for v in ref_offsets]
    out = np.zeros(off[-1], dtype=np.float64)
    g = []
    for t in range(len(off) - 1):
        out[off[t]:off[t + 1]], gt = follow_one(samples[off[t]:off[t + 1]], ref[r_off[t]:r_off[t + 1]], max_gain)
        g.append(gt)
    return out, pcm32(out), (np.concatenate(g) if g else np.zeros(0))


# ---- the planted cases -------------------------------------------------------------------------------------------------

def sounding(n, seed=0x0F0110) -> np.ndarray:
    """n samples that sound everywhere: a normal value of about 0.1, none of them zero or small enough for a square to
    go subnormal."""
    rng = np.random.default_rng(seed + int(n))
    x = 0.1 * rng.standard_normal(int(n))
    return np.where(np.abs(x) < 1e-6, 0.05, x)


def step_case():
    """Consequence 2: (y, x, max_gain)."""
    x = sounding(8192)
    y = np.concatenate([x[:4096] / 2.0, x[4096:] / 16.0])
    return y, x, 32.0


def window_boundaries(p, n):
    """The boundaries of a target of n samples whose window holds sample p."""
    return [b for b in range(boundaries(n)) if (b - 2) * HOP <= p < (b + 2) * HOP]


def ragged_case(lengths, seed=0x0F0111, ref_lengths=None):
    """A batch: (samples, out_offsets, ref, ref_offsets) with target t of lengths[t] samples, its reference of
    ref_lengths[t] (default: the same), the reconstruction at another level in every target and moving inside it."""
    rng = np.random.default_rng(seed)
    ref_lengths = list(lengths) if ref_lengths is None else list(ref_lengths)
    ys, xs = [], []
    for n, nx in zip(lengths, ref_lengths):
        x = 0.1 * rng.standard_normal(max(n, nx))
        level = np.exp(rng.uniform(-3.0, 1.0)) * (1.0 + 0.8 * np.sin(np.arange(n) / 97.0 + rng.uniform(0, 6.0)))
        ys.append(x[:n] * level + 0.01 * rng.standard_normal(n))
        xs.append(x[:nx])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    r_off = np.concatenate([[0], np.cumsum(ref_lengths)]).astype(np.uint64)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)      # noqa: E731
    return cat(ys), off, cat(xs), r_off
