"""Independent numpy restatement of DESIGN.md 5.9: the per-sound descriptors max_power and pitch_confidence
(src/sound.rs:244-269), with the same summation orders as csrc/pitch.hip where they matter:

  * every sum of squares and every autocorrelation lag is a sequential fold in ascending sample order (np.cumsum is a
    sequential left-to-right accumulation, so its last element is exactly that fold);
  * maxima skip NaN and start from 0 (f64::max folded from 0).

Test infrastructure only: the product never imports it.
"""
from __future__ import annotations

import functools
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

W = 2048            # SSYM_PITCH_WINDOW
H = 1024            # SSYM_PITCH_HOP
KAPPA = 0.01        # SSYM_PITCH_OCTAVE_COST
SIGMA = 0.03        # SSYM_PITCH_SILENCE
PW, PH = 128, 64    # SSYM_POWER_WINDOW, SSYM_POWER_HOP


def num_windows(n: int) -> int:
    return max(0, (int(n) - W) // H + 1)


def lag_range(rate: float, f_min: float, f_max: float):
    """(tau_lo, tau_hi); raises ValueError outside the limits of 5.9."""
    if not (math.isfinite(rate) and rate > 0 and math.isfinite(f_min) and math.isfinite(f_max)
            and 0 < f_min < f_max):
        raise ValueError("need rate > 0 and 0 < f_min < f_max")
    lo, hi = math.ceil(rate / f_max), math.floor(rate / f_min)
    if lo < 2 or hi > W // 3 or lo > hi:
        raise ValueError("need 2 <= ceil(rate/f_max) <= floor(rate/f_min) <= 682")
    return lo, hi


@functools.lru_cache(maxsize=None)
def _hann() -> np.ndarray:
    n = np.arange(W, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / float(W))


def hann() -> np.ndarray:
    return _hann().copy()


def _seq_sum_rows(p: np.ndarray) -> np.ndarray:
    return np.cumsum(p, axis=-1)[..., -1]


def _lag_sums(y: np.ndarray, lags: np.ndarray) -> np.ndarray:
    """a(tau) = sum_{n < W - tau} y[n] y[n + tau], n ascending, for every tau in lags (terms past the end are +-0)."""
    ypad = np.concatenate([y, np.zeros(W)])
    view = sliding_window_view(ypad, W)[lags]          # view[i, n] = y[n + lags[i]]
    return _seq_sum_rows(y[None, :] * view)


@functools.lru_cache(maxsize=None)
def _window_norm(lo: int, hi: int) -> np.ndarray:
    h = _hann()
    hh = h * h
    b = _lag_sums(hh, np.concatenate([[0], np.arange(lo, hi + 1)]))
    return b[1:] / b[0]


def window_norm(lags: np.ndarray) -> np.ndarray:
    """b(tau) / b(0) of the effective window h^2, for consecutive lags."""
    return _window_norm(int(lags[0]), int(lags[-1])).copy()


def _lag_sums_batch(Y: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """a[b, tau - lo] for tau in [lo, hi] of every row of Y: each lag a sequential sum over n ascending (the loop runs
    over n, the lags and rows of one step are independent sums)."""
    B = Y.shape[0]
    pad = np.concatenate([Y, np.zeros((B, hi + 1))], axis=1)
    acc = np.zeros((B, hi - lo + 1))
    for n in range(W):
        acc = acc + Y[:, n:n + 1] * pad[:, n + lo:n + hi + 1]
    return acc


def windows(X, G, rate: float, f_min: float, f_max: float, voicing: float):
    """Full windows X [B][W] of sounds with peaks G [B] -> dict of arrays: freq, strength, unvoiced, tau (-1: the
    unvoiced candidate won), score, score_voiced, gap (the distance between the two best candidates' scores)."""
    lo, hi = lag_range(rate, f_min, f_max)
    X = np.asarray(X, dtype=np.float64).reshape(-1, W)
    G = np.broadcast_to(np.asarray(G, dtype=np.float64), (X.shape[0],))
    B = X.shape[0]
    bad = ~np.all(np.isfinite(X), axis=1)
    h = _hann()
    C = np.where(bad[:, None], 0.0, X) * h
    Y = C * h
    L = np.fmax.reduce(np.abs(C), axis=1, initial=0.0)
    a0 = np.cumsum(Y * Y, axis=1)[:, -1]
    a = _lag_sums_batch(Y, lo - 1, hi + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (a / a0[:, None]) / _window_norm(lo - 1, hi + 1)[None, :]
        rm, r0, rp = r[:, :-2], r[:, 1:-1], r[:, 2:]
        cand = (r0 > rm) & (r0 >= rp) & (a0 != 0.0)[:, None]
        d = (rm - 2.0 * r0) + rp
        delta = np.where(d < 0.0, (rm - rp) / (2.0 * np.where(d < 0.0, d, -1.0)), 0.0)
        R = r0 - ((rm - rp) * delta) / 4.0
        taus = np.arange(lo, hi + 1, dtype=np.float64)[None, :]
        S = R - KAPPA * np.log2((f_min * (taus + delta)) / rate)   # lags that are no candidate may give NaN here
        Sc = np.where(cand, S, -np.inf)
        k = np.argmax(Sc, axis=1)                                    # the first maximum: the smaller tau wins ties
        rows = np.arange(B)
        has = np.any(cand, axis=1)
        strength = np.where(has, S[rows, k], 0.0)
        freq = np.where(has, rate / (taus[0, k] + delta[rows, k]), 0.0)
        t = (L / G) / (SIGMA / np.float64(1.0 + voicing))      # v = -1: sigma / 0 = inf, as on the device
    u = voicing + np.fmax(0.0, 2.0 - t)                   # Rust's max: NaN (G = 0) gives u = voicing
    voiced = has & (strength >= u)
    score = np.where(voiced, strength, u)
    score_voiced = np.where(has, strength, 0.0)
    tau = np.where(voiced, lo + k, -1)
    top2 = -np.sort(-np.concatenate([Sc, u[:, None]], axis=1), axis=1)[:, :2]
    gap = top2[:, 0] - top2[:, 1]
    nan = np.full(B, np.nan)
    out = dict(freq=freq, strength=strength, unvoiced=u, score=score, score_voiced=score_voiced)
    out = {key: np.where(bad, nan, v) for key, v in out.items()}
    out["tau"] = np.where(bad, -1, tau)
    out["gap"] = np.where(bad, np.inf, gap)
    return out


def window(x, G: float, rate: float, f_min: float, f_max: float, voicing: float):
    """One full window -> dict of scalars (see windows)."""
    o = windows(np.asarray(x, dtype=np.float64)[None, :], np.array([G]), rate, f_min, f_max, voicing)
    return {key: (int(v[0]) if key == "tau" else float(v[0])) for key, v in o.items()}


def peak(x) -> float:
    return float(np.fmax.reduce(np.abs(np.asarray(x, dtype=np.float64)), initial=0.0))


def max_power(x) -> float:
    """analyze_max_power: the largest sqrt((sum of squares, sequential) / 128) over full 128 / 64 windows, from 0."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size < PW:
        return 0.0
    n = (x.size - PW) // PH + 1
    win = sliding_window_view(x, PW)[::PH][:n]
    rms = np.sqrt(_seq_sum_rows(win * win) / float(PW))
    return float(np.fmax.reduce(rms, initial=0.0))


def track(x, rate=44100.0, f_min=100.0, f_max=500.0, voicing=0.2):
    """Every window of one sound, in order: the dict of arrays of windows()."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    nw = num_windows(x.size)
    X = sliding_window_view(x, W)[::H][:nw] if nw else np.zeros((0, W))
    return windows(X, peak(x), rate, f_min, f_max, voicing)


def fold(values) -> float:
    return float(np.fmax.reduce(np.asarray(values, dtype=np.float64), initial=0.0))


def descriptors(samples, offsets, rate=44100.0, f_min=100.0, f_max=500.0, voicing=0.2):
    """(max_power[n], pitch_conf[n], pitch_conf_voiced_only[n], tracks[n]) for a ragged batch, all windows of the
    batch evaluated together."""
    lag_range(rate, f_min, f_max)
    samples = np.asarray(samples, dtype=np.float64)
    n = len(offsets) - 1
    xs = [samples[int(offsets[i]):int(offsets[i + 1])] for i in range(n)]
    nws = [num_windows(x.size) for x in xs]
    X = np.concatenate([sliding_window_view(x, W)[::H][:nw] for x, nw in zip(xs, nws) if nw] or [np.zeros((0, W))])
    G = np.concatenate([np.full(nw, peak(x)) for x, nw in zip(xs, nws)] or [np.zeros(0)])
    allw = windows(X, G, rate, f_min, f_max, voicing)
    woff = np.concatenate([[0], np.cumsum(nws)]).astype(np.int64)
    tracks = [{key: v[woff[i]:woff[i + 1]] for key, v in allw.items()} for i in range(n)]
    mp = np.array([max_power(x) for x in xs])
    pc = np.array([fold(t["score"]) for t in tracks])
    pv = np.array([fold(t["score_voiced"]) for t in tracks])
    return mp, pc, pv, tracks
