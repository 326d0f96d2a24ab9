"""Inputs of the WSOLA search whose winning lag is known by construction -- test infrastructure shared by
tests/test_wsola_ref.py (which holds every case to the restatement on the CPU) and tests/test_gpu_wsola_search.py (which
holds the GPU to both).

Planted cases.  The source is +0.0 except unit pulses; prev = pos[0] = map[0] * HOP and x[prev + HOP] = 1 make the
template one pulse at n = 0, so c(d) = x[nom + d] is 0 or 1 and e(d) counts the pulses in x[nom + d .. nom + d + BIN):
every sum is a small integer, hence exact, and score(d) = 1 / sqrt(e(d)) at a pulse, 0 elsewhere.  One pulse at nom + d
makes d the single winner.  Pulses at several lags tie once their windows hold the same number of pulses; a later
window has lost the earlier lags' pulses, so levelling pulses go where only the later windows hold them -- and beyond
nom + S, where no admissible lag reads them as c (nom + d1 + BIN is such a place for every pair but d1 = -S at S = 512,
where it is lag +S itself; the next sample is used then).  The winner of a tie is the rule's: the smaller |d|, then the
negative d.  The map is [0, 8]: nom - 512 >= HOP + BIN, so no window of a candidate reaches the template's pulse.

The lag indices planted at (thread tid of wsola_search_kernel owns the indices i = tid + 256 r, d = i - S, L = 2 S + 1):
the first and last lane of every wave in every round, i = S (d = 0), L - 2 and L - 1; ties between the same thread's
rounds, two lanes of a wave (every step of the butterfly among them), two waves of a round, another wave in another
round, d against -d, the first lag against the last, and three lags at once.

Odd samples.  Noisy sinusoids of at least 8000 samples with one oddity each (ODD_KINDS) under monotone maps with mild
repeats and skips; test_wsola_ref.py asserts on the restatement what steps they must contain.
"""
import collections
import functools

import numpy as np

import warp_ref
import wsola_ref as ref
from wsola_ref import BIN, HOP

Case = collections.namedtuple("Case", "kind name source fmap n_out expected")

M = 8                                                  # the searched frame of a planted case: nom = M * HOP
PLANT_WIDTHS = (1, 31, 32, 127, 128, 255, 256, 383, 384, 511, 512)
EDGE_WIDTHS = (200, 512)
ODD_WIDTHS = (0, 64, 512)
ODD_KINDS = ("nan", "+inf", "-inf", "-0.0 run", "subnormal run", "1e-170 stretch", "1e160 stretch")
ODD_SEED = 0x0DD5


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint64)


def plant_indices(S):
    """The lag indices i = d + S every width is planted at: owner edges, the centre, the last two."""
    L = 2 * S + 1
    own = {256 * r + 64 * w + lane for r in range((L + 255) // 256) for w in range(4) for lane in (0, 63)}
    return sorted(i for i in own | {S, L - 2, L - 1} if 0 <= i < L)


def tie_sets(S):
    """(kind, lag indices) of the ties planted at width S, every set once."""
    L = 2 * S + 1
    rounds = (L + 255) // 256
    first, last = (lambda r, w: 256 * r + 64 * w), (lambda r, w: 256 * r + 64 * w + 63)
    sets = [("first against last", (0, L - 1))]
    sets += [("same thread, two rounds", (i, i + 256)) for i in plant_indices(S)]
    sets += [("two lanes of a wave", (first(r, w), last(r, w))) for r in range(rounds) for w in range(4)]
    sets += [("two lanes of a wave", (64, 64 ^ step)) for step in (1, 2, 4, 8, 16, 32)]
    for r in range(rounds):
        sets += [("two waves of a round", (first(r, w), first(r, v))) for w, v in ((0, 1), (0, 3), (1, 2), (2, 3))]
        sets.append(("two waves of a round", (last(r, 0), last(r, 3))))
    for r in range(rounds - 1):
        sets += [("another wave and round", pair) for pair in ((first(r, 1), last(r + 1, 2)), (last(r, 3), first(r + 1, 0)),
                                                                 (first(r, 0), first(r + 1, 3)), (last(r, 2), first(r + 1, 1)))]
    if rounds > 1:
        sets.append(("another wave and round", (first(0, 3), last(rounds - 1, 0))))
    sets += [("d against -d", (i, 2 * S - i)) for i in plant_indices(S) + [S - 1, S - S // 2] if i < S]
    sets += [("around the centre", pair) for pair in ((S - 1, S), (S, S + 1))]
    sets += [("three lags", trio) for trio in ((0, S, L - 1), (0, 256, 512), (64, 128, 192), (63, 64, 320), (S - 1, S + 1, L - 1))]
    seen, out = set(), []
    for kind, idx in sets:
        key = frozenset(idx)
        if len(key) == len(idx) and all(0 <= i < L for i in idx) and key not in seen:
            seen.add(key)
            out.append((kind, tuple(sorted(idx))))
    return out


def planted(S, lags, kind, prev_frame=0, nom_frame=M, s_len=4096):
    """The two-frame case whose step scores 1 / sqrt(e) with one e at every lag of `lags` and 0 at every other lag."""
    lags = sorted(set(int(d) for d in lags))
    prev, nom = prev_frame * HOP, nom_frame * HOP
    x = np.zeros(s_len)
    x[prev + HOP] = 1.0
    for d in lags:
        assert -S <= d <= S and 0 <= nom + d < s_len, (S, d)
        x[nom + d] = 1.0

    def energy(d):
        return int(x[nom + d:nom + d + BIN].sum())

    for a, b in zip(lags, lags[1:]):
        q = max(nom + a + BIN, nom + S + 1)          # in b's window and every later one, in no earlier one, no lag's c
        while energy(b) < energy(lags[0]):
            if q >= min(nom + b + BIN, s_len):
                raise ValueError("no room to level lags %d and %d at S = %d" % (a, b, S))
            x[q] = 1.0
            q += 1
    assert len({energy(d) for d in lags}) == 1, (S, lags)
    # the template's window holds its own pulse alone, no candidate's window holds it
    assert x[prev + HOP:prev + HOP + BIN].sum() == 1.0 and (prev + HOP < max(nom - S, 0) or prev + HOP >= nom + S + BIN)
    winner = min(lags, key=lambda d: (abs(d), d))
    return Case(kind, "S %d %s %s" % (S, kind, lags), x, [prev_frame, nom_frame], HOP + BIN + 20, [prev, nom + winner])


def plant_cases(S):
    """Single winners at every planted index, then the ties."""
    cases = [planted(S, [i - S], "single winner") for i in plant_indices(S)]
    cases += [planted(S, [i - S for i in idx], "tie: " + kind) for kind, idx in tie_sets(S)]
    return cases


def edge_cases(S):
    """The edges of the admissible range lo .. hi (S >= 78)."""
    nom = M * HOP
    cases = []
    # map[1] * HOP < S: lo = -nom, the pulse at source sample 0 (the template from frame 12, clear of every candidate)
    m1 = (S - 1) // HOP
    cases.append(planted(S, [-m1 * HOP], "lo = -nom", prev_frame=12, nom_frame=m1))
    if m1:
        cases.append(planted(S, [-m1 * HOP, m1 * HOP], "lo = -nom against +nom", prev_frame=12, nom_frame=m1))
    # the source ends inside the search range, the pulse is its last sample: the winner is hi
    h = S // 2
    cases.append(planted(S, [h], "hi inside the range", s_len=nom + h + 1))
    # nom >= sLen, nom - S < sLen: only negative lags; a pulse at the first of them, and none (every score 0: hi wins)
    g = S // 3
    cases.append(planted(S, [-S], "only negative lags, lo", s_len=nom - g))
    x = np.zeros(nom - g)
    x[HOP] = 1.0
    cases.append(Case("only negative lags, all tied", "S %d only negative lags, all tied" % S, x, [0, M], HOP + BIN + 20,
                      [0, nom - g - 1]))
    # a step without an admissible lag between two searched steps; the step after it has a template wholly beyond the
    # source: all zeros, every score 0, the admissible lag of least |d| wins -- 0, or hi where nom >= sLen
    for s_len, last, want in ((4096, 9, 9 * HOP), (16 * HOP - 77, 16, 16 * HOP - 78)):
        x = np.zeros(s_len)
        x[[HOP, nom - h]] = 1.0
        cases.append(Case("no admissible lag mid-chain", "S %d no admissible lag mid-chain, sLen %d" % (S, s_len), x,
                          [0, M, 40, last, M], 4 * HOP + BIN + 20, [0, nom - h, 40 * HOP, want, nom]))
    # a template wholly beyond the source although a pulse lies in the range
    x = np.zeros(4096)
    x[nom + 5] = 1.0
    cases.append(Case("template beyond the source", "S %d template beyond the source" % S, x, [20, M], HOP + BIN + 20,
                      [20 * HOP, nom]))
    return cases


def flat_cases(S):
    """Constant and silent sources: every score ties (or e = 0), so lag 0 wins wherever it is admissible."""
    cases = []
    for label, value in (("constant", 0.25), ("silent", 0.0)):
        for fmap in ([0, 0, 1, 1, 2, 5, 9, 9, 20], [10, 3, 3, 17], [2, 2, 3, 5, 5, 6, 8, 11, 12, 12, 13, 0]):
            cases.append(Case(label, "S %d %s %s" % (S, label, fmap), np.full(9000, value), fmap, (len(fmap) - 1) * HOP + BIN + 20,
                              [v * HOP for v in fmap]))
    return cases


def pack(cases):
    """One call's arguments, every case a target with a source of its own: (sounds, idx, out offsets, maps, map
    offsets, map frames, None) as test_gpu_wsola._check takes them, and the expected positions laid out as the maps."""
    frames = [len(c.fmap) for c in cases]
    maps = np.concatenate([np.asarray(c.fmap, dtype=np.uint32) for c in cases])
    want = np.concatenate([np.asarray(c.expected, dtype=np.uint64) for c in cases])
    call = ([c.source for c in cases], np.arange(len(cases), dtype=np.uint32), _offsets([c.n_out for c in cases]), maps,
            _offsets(frames), np.asarray(frames, dtype=np.uint32), None)
    return call, want


@functools.lru_cache(maxsize=None)
def odd_call(seed=ODD_SEED, frames=24):
    """One target per kind of ODD_KINDS: (sounds, idx, out offsets, maps, map offsets, map frames, None)."""
    rng = np.random.default_rng(seed)
    sounds, maps, lens = [], [], []
    for kind in ODD_KINDS:
        n = int(rng.integers(8000, 9000))
        k = np.arange(n)
        x = 0.6 * np.sin(2 * np.pi * rng.uniform(80, 500) * k / 44100.0 + rng.uniform(0, 6)) + 0.02 * rng.standard_normal(n)
        p = int(rng.integers(1500, 5000))
        if kind == "nan":
            x[p] = np.nan
        elif kind in ("+inf", "-inf"):
            x[p] = np.inf if kind == "+inf" else -np.inf
        elif kind == "-0.0 run":
            x[p:p + int(rng.integers(200, 1400))] = -0.0
        elif kind == "subnormal run":
            run = int(rng.integers(200, 1400))
            x[p:p + run] = rng.integers(1, 1 << 20, size=run) * 5e-324 * rng.choice([-1.0, 1.0], size=run)
        elif kind == "1e-170 stretch":
            x[p:p + int(rng.integers(1400, 2200))] *= 1e-170            # the squares underflow: e == 0, samples != 0
        else:
            x[p:p + int(rng.integers(1400, 2200))] *= 1e160             # the squares overflow: e = +inf
        fmap = np.minimum(int(rng.integers(0, 3)) + np.cumsum(rng.choice([0, 1, 1, 1, 2], size=frames)), n // HOP - 1)
        sounds.append(x)
        maps.append(fmap.astype(np.uint32))
        lens.append(frames * HOP + int(rng.integers(0, 700)))
    nf = [frames] * len(sounds)
    return (sounds, np.arange(len(sounds), dtype=np.uint32), _offsets(lens), np.concatenate(maps), _offsets(nf),
            np.asarray(nf, dtype=np.uint32), None)


@functools.lru_cache(maxsize=None)
def odd_reference(S):
    """The restatement on odd_call(): (samples, positions) of WSOLA at width S; S = None: the plain warp's samples."""
    sounds, idx, off, maps, m_off, frames, _ = odd_call()
    if S is None:
        return warp_ref.warp(sounds, idx, off, maps, m_off, frames)
    return ref.wsola(sounds, idx, off, maps, m_off, frames, None, S)


def odd_walk(S, seed=ODD_SEED):
    """The restatement's chain over odd_call() step by step: (how many searched steps are of each kind the odd samples
    are there for, NaN output samples, output samples)."""
    sounds, idx, off, maps, m_off, frames, _ = odd_call(seed)
    kinds = collections.Counter()
    nans = 0
    for t, x in enumerate(sounds):
        fmap = [int(v) for v in maps[int(m_off[t]):int(m_off[t]) + int(frames[t])]]
        pos = [fmap[0] * HOP]
        for j in range(1, len(fmap)):
            nom = fmap[j] * HOP
            scored = ref.lag_scores(x, pos[-1], nom, S)
            best = ref.pick(scored)
            pos.append(nom + best)
            if scored is None:
                continue
            lo, _, e, score = scored
            nan = np.isnan(score)
            kinds["searched"] += 1
            kinds["every score NaN"] += int(nan.all() and best == 0)
            kinds["some scores NaN, winner off lag 0"] += int(nan.any() and not nan.all() and best != 0)
            kinds["e == 0 on non-zero samples"] += int(any(np.any(x[nom + lo + i:nom + lo + i + BIN] != 0.0)
                                                           for i in np.flatnonzero(e == 0.0)))
            kinds["e = +inf"] += int(np.isposinf(e).any())
        nans += int(np.isnan(ref.synth_one(x, int(off[t + 1]) - int(off[t]), pos)).sum())
    return kinds, nans, int(off[-1])
