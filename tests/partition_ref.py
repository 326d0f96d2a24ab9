"""An independent numpy restatement of the partitioner's definitions.

Written from the definitions, not from the kernels: plain loops and numpy reductions, f64 throughout.  The GPU tests
compare ssym_standardize / ssym_gmm_* / ssym_vote_segments / ssym_partition against it.  The product never imports it.
"""
from __future__ import annotations

import numpy as np

HOP = 256


def standardize(x: np.ndarray) -> np.ndarray:
    """Per column (x - mean) / sample std (n - 1); a column whose std is 0 (or n < 2) maps to 0."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if n == 0:
        return x.copy()
    mean = x.sum(axis=0) / n
    if n < 2:
        return np.zeros_like(x)
    sd = np.sqrt(((x - mean) ** 2).sum(axis=0) / (n - 1))
    out = np.zeros_like(x)
    ok = sd > 0
    out[:, ok] = (x[:, ok] - mean[ok]) / sd[ok]
    return out


def _log_terms(x, weights, means, covs):
    """a_ik = log pi_k - 1/2 log det S_k - 1/2 (x_i - mu_k)^T S_k^-1 (x_i - mu_k), the (2 pi)^(d/2) dropped."""
    n, K = x.shape[0], weights.shape[0]
    a = np.empty((n, K))
    with np.errstate(divide="ignore"):
        logw = np.log(weights)
    for k in range(K):
        L = np.linalg.cholesky(covs[k])
        y = np.linalg.solve(L, (x - means[k]).T)            # forward substitution L y = (x - mu)
        maha = (y * y).sum(axis=0)
        a[:, k] = logw[k] - np.log(np.diag(L)).sum() - 0.5 * maha
    return a


def posteriors(x, weights, means, covs):
    """(posteriors [n][K], log-likelihood per frame): log-sum-exp with the row maximum subtracted."""
    a = _log_terms(x, weights, means, covs)
    m = a.max(axis=1, keepdims=True)
    e = np.exp(a - m)
    s = e.sum(axis=1, keepdims=True)
    return e / s, (m + np.log(s))[:, 0]


def gmm_train(x, init_rows, eps=0.1, max_iters=5):
    """EM as DESIGN.md 5.8 states it.  Returns dict(weights, means, covs, log_lik, iters, totals): totals[j] is the
    log-likelihood computed at step j (the last one is the step that stopped the loop, when it converged)."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    K = len(init_rows)
    means = x[np.asarray(init_rows, dtype=np.int64)].copy()
    mu = x.mean(axis=0)
    c0 = (x - mu).T @ (x - mu) / (n - 1) + eps * np.eye(d)
    covs = np.repeat(c0[None], K, axis=0)
    weights = np.full(K, 1.0 / K)
    log_lik, iters, totals = 0.0, 0, []
    for _ in range(max_iters):
        r, ll = posteriors(x, weights, means, covs)
        total = ll.sum()
        totals.append(total)
        if abs(total - log_lik) < 1e-15:
            break
        log_lik = total
        iters += 1
        Nk = r.sum(axis=0)
        for k in range(K):
            if Nk[k] == 0.0:
                weights[k] = 0.0                     # keeps its mean and covariance
                continue
            weights[k] = Nk[k] / n
            means[k] = (r[:, k:k + 1] * x).sum(axis=0) / Nk[k]
            dx = x - means[k]
            covs[k] = (r[:, k:k + 1] * dx).T @ dx / Nk[k] + eps * np.eye(d)
    return dict(weights=weights, means=means, covs=covs, log_lik=log_lik, iters=iters, totals=totals)


def max_index(row) -> int:
    """src/sound.rs:486-495: the first strict maximum, starting from (0, 0.0)."""
    best, bv = 0, 0.0
    for k, v in enumerate(row):
        if v > bv:
            best, bv = k, v
    return best


def letters(post) -> np.ndarray:
    return np.array([max_index(r) for r in post], dtype=np.uint8)


# ---- voting experts ----------------------------------------------------------------------------------------------

def _codes(s, n, A):
    """Base-A code of every window s[i..i+n), the first symbol most significant."""
    N = len(s)
    c = np.zeros(N - n + 1, dtype=np.int64)
    for q in range(n):
        c = c * A + s[q:N - n + 1 + q]
    return c


def vote_details(s, depth):
    """(frequency-expert votes [N+1], entropy-expert votes [N+1], entropy top-2 margin per window, zf per length)."""
    s = np.asarray(s, dtype=np.int64)
    N = len(s)
    vf = np.zeros(N + 1, dtype=np.int64)
    vh = np.zeros(N + 1, dtype=np.int64)
    if N < depth:
        return vf, vh, np.zeros(0), []
    A = int(s.max()) + 1 if N else 1
    A = max(A, 2)
    assert A ** depth < 2 ** 63
    uniq, inv, cnt = [], [], []
    for n in range(1, depth + 1):
        u, i, c = np.unique(_codes(s, n, A), return_inverse=True, return_counts=True)
        uniq.append(u)
        inv.append(i.reshape(-1))
        cnt.append(c)
    zf, zh = [], []
    for n in range(1, depth):
        # frequency: from the exact integer sums S1 = sum c, S2 = sum c^2
        c = cnt[n - 1]
        D = len(c)
        S1, S2 = int(c.sum()), int((c.astype(object) ** 2).sum())
        mean = float(S1) / float(D)
        var = float(S2) / float(D) - mean * mean
        sd = np.sqrt(var) if var > 0.0 else 0.0
        zf.append((c.astype(np.float64) - mean) / sd if sd > 0.0 else np.zeros(D))
        # boundary entropy over the successors g.c, p first, then the sum in ascending symbol order
        pos = np.searchsorted(uniq[n - 1], uniq[n] // A)        # the n-gram each (n+1)-gram extends
        total = np.bincount(pos, weights=cnt[n], minlength=D)
        p = cnt[n] / total[pos]
        h = -np.bincount(pos, weights=p * np.log(p), minlength=D)   # in code order: ascending symbol per n-gram
        hm = h.mean()
        hs = np.sqrt(((h - hm) ** 2).mean())
        zh.append((h - hm) / hs if hs > 0.0 else np.zeros(D))
    W = N - depth + 1
    sf = np.empty((W, depth - 1))
    sh = np.empty((W, depth - 1))
    for i in range(1, depth):
        j = depth - i
        sf[:, i - 1] = zf[i - 1][inv[i - 1][:W]] + zf[j - 1][inv[j - 1][i:i + W]]
        sh[:, i - 1] = zh[i - 1][inv[i - 1][:W]]
    np.add.at(vf, np.arange(W) + 1 + np.argmax(sf, axis=1), 1)      # argmax: the first maximum
    np.add.at(vh, np.arange(W) + 1 + np.argmax(sh, axis=1), 1)
    srt = np.sort(sh, axis=1)
    margins = srt[:, -1] - srt[:, -2] if depth > 2 else np.full(W, np.inf)
    return vf, vh, margins, zf


def boundaries(votes, threshold):
    """p in 1..N-1 with votes[p] >= t, votes[p] > votes[p-1], votes[p] >= votes[p+1] (votes[N] counts as 0)."""
    v = np.asarray(votes, dtype=np.int64).copy()
    N = len(v) - 1
    if N < 2:
        return []
    v[N] = 0
    p = np.arange(1, N)
    ok = (v[p] >= threshold) & (v[p] > v[p - 1]) & (v[p] >= v[p + 1])
    return [int(q) for q in p[ok]]


def segments(s, depth, threshold):
    """Segment lengths (frames) of the symbol string."""
    N = len(s)
    if N == 0:
        return []
    vf, vh, _, _ = vote_details(s, depth)
    b = [0] + boundaries(vf + vh, threshold) + [N]
    return [b[i + 1] - b[i] for i in range(len(b) - 1)]


def partition(feats, weights, means, covs, depth=5, threshold=4, standardise=True):
    """Partitioner::partition_other in frames: standardise with the data's own statistics, letters, segments."""
    x = standardize(feats) if standardise else np.asarray(feats, dtype=np.float64)
    post, _ = posteriors(x, weights, means, covs)
    return segments(letters(post), depth, threshold)
