"""Plain restatement of WSOLA reconstruction (ssym_reconstruct_wsola; DESIGN.md section 2, the comment in
include/soundsym_amd.h) -- test infrastructure, what the GPU is held to bit for bit.

HOP, BIN, the window, x, F and map as in warp_ref; S the search width.  pos[0] = map[0] * HOP.  For j >= 1: nom = map[j] *
HOP; tmpl[n] = x[pos[j-1] + HOP + n], n < BIN; for every lag d in -S .. S with 0 <= nom + d < len(x): cand[n] = x[nom + d +
n] (in both, a sample at or beyond len(x) reads +0.0); c = sum of tmpl[n] * cand[n], e = sum of cand[n] * cand[n], both
from +0.0 in ascending n, every product and sum rounded on its own (np.cumsum is a serial sum); score = c / sqrt(e), 0
when e = 0.  pos[j] = nom + d*, d* the lag of the greatest score, ties to the smaller |d|, then to the negative d; a NaN
score never wins; d* = 0 when no lag is admissible or none has a score that is a number.  Synthesis: warp_ref's taps and
value with p = pos[j] + m.  F = 0 or a pair without a path: the length fit.
"""
import numpy as np

import warp_ref
from warp_ref import BIN, HOP, WINDOW, length_fit, pcm32  # noqa: F401

UNSET = np.iinfo(np.uint64).max


def _padded(x, start, count):
    """x[start : start + count] with +0.0 wherever the index is outside x (Python ints: no wrap)."""
    out = np.zeros(count, dtype=np.float64)
    a, b = max(start, 0), min(start + count, x.size)
    if a < b:
        out[a - start:b - start] = x[a:b]
    return out


def lag_scores(x, prev, nom, S):
    """(lo, c, e, score) of one step's admissible lags lo, lo + 1, ...; None when no lag is admissible."""
    s_len = int(x.size)
    lo, hi = max(-S, -nom), min(S, s_len - 1 - nom)
    if lo > hi:
        return None
    tmpl = _padded(x, prev + HOP, BIN)
    span = _padded(x, nom + lo, hi - lo + BIN)
    cand = np.lib.stride_tricks.sliding_window_view(span, BIN)            # [lag, n] = x[nom + lo + lag + n]
    zero = np.zeros((cand.shape[0], 1))
    with np.errstate(all="ignore"):
        c = np.cumsum(np.concatenate([zero, tmpl[None, :] * cand], axis=1), axis=1)[:, -1]
        e = np.cumsum(np.concatenate([zero, cand * cand], axis=1), axis=1)[:, -1]
        score = np.where(e == 0.0, 0.0, c / np.sqrt(e))
    return lo, c, e, score


def best_lag(x, prev, nom, S):
    """d* of one step: prev = pos[j-1], nom = map[j] * HOP."""
    return pick(lag_scores(x, prev, nom, S))


def pick(scored):
    """d* from lag_scores' result."""
    if scored is None:
        return 0
    lo, _, _, score = scored
    best, best_score = None, 0.0
    for i, sc in enumerate(score.tolist()):
        d = lo + i
        if sc != sc:
            continue
        if best is None or sc > best_score or (sc == best_score and (abs(d), d) < (abs(best), best)):
            best, best_score = d, sc
    return 0 if best is None else best


def positions(x, fmap, S):
    """pos[0 .. F) of one target (Python ints)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    fm = [int(v) for v in fmap]
    pos = [fm[0] * HOP] if fm else []
    for j in range(1, len(fm)):
        nom = fm[j] * HOP
        pos.append(nom + (best_lag(x, pos[-1], nom, S) if S else 0))
    return pos


def synth_one(x, n, pos):
    """warp_ref.warp_one with the frame positions given in samples."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    F, s_len = len(pos), int(x.size)
    ps = np.asarray([min(int(p), 1 << 62) for p in pos], dtype=np.int64)
    win = np.asarray(WINDOW, dtype=np.float64)
    k = np.arange(n, dtype=np.int64)
    num, den = np.zeros(n), np.zeros(n)
    for i in range(BIN // HOP):
        j = k // HOP - (BIN // HOP - 1) + i
        m = k - j * HOP
        ok = (j >= 0) & (j < F)
        p = ps[np.clip(j, 0, F - 1)] + m
        ok &= p < s_len
        w = win[m]
        xv = x[np.where(ok, p, 0)] if s_len else np.zeros(n)
        num = np.where(ok, num + w * xv, num)
        den = np.where(ok, den + w, den)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, num / den, 0.0)


def wsola_one(x, n, fmap, S, valid=True):
    """One target: (n output samples, positions)."""
    if len(fmap) == 0 or not valid:
        return length_fit(x, n), []
    pos = positions(x, fmap, S)
    return synth_one(x, n, pos), pos


def wsola(sounds, idx, out_offsets, maps, map_offsets, map_frames, pair_len=None, search=0):
    """The whole call: (samples, positions laid out by map_offsets with UNSET in every slot the call leaves alone)."""
    out_offsets = [int(v) for v in out_offsets]
    out = np.zeros(out_offsets[-1], dtype=np.float64)
    pos = np.full(int(map_offsets[-1]), UNSET, dtype=np.uint64)
    for t in range(len(idx)):
        n = out_offsets[t + 1] - out_offsets[t]
        F, m0 = int(map_frames[t]), int(map_offsets[t])
        valid = pair_len is None or int(pair_len[t]) != 0
        fmap = maps[m0:m0 + F] if (F and valid) else []
        out[out_offsets[t]:out_offsets[t + 1]], p = wsola_one(sounds[int(idx[t])], n, fmap, search, valid)
        pos[m0:m0 + len(p)] = np.asarray(p, dtype=np.uint64)
    return out, pos


def purity(y, freq, rate):
    """Share of y's energy that a least-squares sine + cosine at freq explains."""
    y = np.asarray(y, dtype=np.float64)
    ph = 2.0 * np.pi * freq * np.arange(y.size) / rate
    basis = np.stack([np.sin(ph), np.cos(ph)], axis=1)
    coef, *_ = np.linalg.lstsq(basis, y, rcond=None)
    return float(np.sum((basis @ coef) ** 2) / np.sum(y * y))
