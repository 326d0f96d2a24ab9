"""The restatement of WSOLA reconstruction (tests/wsola_ref.py) held to its definition on the CPU: the two consequences
the contract names (no search = the plain warp; a diagonal map keeps its positions), the tie rule, the source's edges, a
sample-by-sample reading of the score, the property the feature exists for -- a sinusoid stays a sinusoid under
stretching and squeezing maps -- and the inputs the GPU's lag search is held to (tests/wsola_cases.py): every planted
winner is the restatement's winner, and the odd-sample sources contain the steps they are there for."""
import collections
import math

import numpy as np
import pytest

import warp_ref
import wsola_cases as wc
import wsola_ref as ref
from wsola_ref import BIN, HOP


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint64)


def test_no_search_is_the_plain_warp_bit_for_bit():
    rng = np.random.default_rng(0x5A0)
    sounds = [rng.uniform(-1, 1, size=int(v)) for v in (9000, 300, 0, 5000, 2049)]
    n = 12
    idx = rng.integers(0, len(sounds), size=n)
    frames = rng.integers(1, 30, size=n)
    frames[3] = 0
    plen = np.ones(n, dtype=np.uint32)
    plen[5] = 0
    lens = frames * HOP + rng.integers(0, 900, size=n)
    m_off = _offsets(frames + 2)
    maps = np.zeros(int(m_off[-1]), dtype=np.uint32)
    for t in range(n):
        sf = max(sounds[idx[t]].size // HOP, 1)
        m = np.sort(rng.integers(0, sf + 3, size=int(frames[t])))              # repeats, skips, frames past the source
        maps[int(m_off[t]):int(m_off[t]) + int(frames[t])] = m
    off = _offsets(lens)
    want = warp_ref.warp(sounds, idx, off, maps, m_off, frames, plen)
    got, pos = ref.wsola(sounds, idx, off, maps, m_off, frames, plen, search=0)
    assert np.array_equal(_bits(got), _bits(want))
    for t in range(n):
        a, f = int(m_off[t]), int(frames[t])
        if f and plen[t]:
            assert np.array_equal(pos[a:a + f], maps[a:a + f].astype(np.uint64) * HOP)
            assert (pos[a + f:int(m_off[t + 1])] == ref.UNSET).all()
        else:
            assert (pos[a:int(m_off[t + 1])] == ref.UNSET).all()


@pytest.mark.parametrize("S", [1, 64, 256])
def test_a_diagonal_map_on_noise_keeps_its_positions(S):
    rng = np.random.default_rng(0xD1A6)
    x = rng.standard_normal(24 * HOP + 123)
    fmap = np.arange(24)
    assert ref.positions(x, fmap, S) == [j * HOP for j in range(24)]
    out, _ = ref.wsola_one(x, x.size, fmap, S)
    assert np.array_equal(_bits(out), _bits(warp_ref.warp_one(x, x.size, fmap)))


def test_ties_go_to_lag_zero_on_constant_and_silent_sources():
    for x in (np.full(9000, 0.25), np.zeros(9000)):
        for fmap in ([0, 0, 1, 1, 2, 5, 9, 9, 20], [10, 3, 3, 17]):
            # (the constant source: away from the edges every candidate is the same vector, so every score is the same
            # number; near the end shorter candidates score less)
            assert ref.positions(x, fmap, 200) == [v * HOP for v in fmap]
    # the tie rule itself.  tmpl = x[HOP ...] is one pulse at n = 0, so c(d) = x[nom + d]; every sum below is a small
    # integer, hence exact.  Pulses at nom - 1 and nom + 1, and one at nom - 1 + BIN that only the later window holds:
    # c = 1, e = 2 at both lags -> the negative one
    nom = 8 * HOP
    x = np.zeros(6000)
    x[[HOP, nom - 1, nom + 1, nom - 1 + BIN]] = 1.0
    assert ref.positions(x, [0, 8], 4) == [0, nom - 1]
    # pulses at nom - 3 and nom + 1 (and nom - 3 + BIN ... nom + BIN for the later window): tied again -> the smaller |d|
    x = np.zeros(6000)
    x[[HOP, nom - 3, nom + 1, nom + BIN]] = 1.0
    assert ref.positions(x, [0, 8], 4) == [0, nom + 1]


def test_the_score_read_aloud_sample_by_sample():
    rng = np.random.default_rng(0x5C0)
    x = rng.uniform(-1, 1, size=3000)
    xs = x.tolist()
    for prev, nom, S in ((0, 512, 7), (256, 1792, 9), (1800, 2900, 12), (512, 0, 5)):
        best, best_sc = None, 0.0
        for d in range(-S, S + 1):
            if not 0 <= nom + d < len(xs):
                continue
            c, e = 0.0, 0.0
            for n in range(BIN):
                tv = xs[prev + HOP + n] if prev + HOP + n < len(xs) else 0.0
                cv = xs[nom + d + n] if nom + d + n < len(xs) else 0.0
                c = c + tv * cv
                e = e + cv * cv
            sc = c / math.sqrt(e) if e != 0.0 else 0.0
            if best is None or sc > best_sc or (sc == best_sc and (abs(d), d) < (abs(best), best)):
                best, best_sc = d, sc
        assert ref.best_lag(x, prev, nom, S) == best


def test_the_edges_of_the_source():
    rng = np.random.default_rng(0xED6E)
    x = rng.uniform(-1, 1, size=5 * HOP + 77)
    s_len = x.size
    # frames whose candidates run past sLen, frames with nom >= sLen, a frame at 0 (negative lags inadmissible)
    fmap = [3, 4, 5, 6, 0, 5, 4, 0xFFFFFFFF, 2]
    pos = ref.positions(x, fmap, 300)
    for j, p in enumerate(pos):
        nom = fmap[j] * HOP
        if nom - 300 >= s_len:
            assert p == nom                                    # no admissible lag: d* = 0
        else:
            assert 0 <= p < s_len and abs(p - nom) <= 300
    assert 6 * HOP >= s_len and pos[3] < s_len              # nom >= sLen, but lags down to -300 are admissible
    assert pos[7] == 0xFFFFFFFF * HOP
    out, _ = ref.wsola_one(x, 9 * HOP + 500, fmap, 300)
    assert np.isfinite(out).all() and np.abs(out).max() <= np.abs(x).max() * (1 + 1e-12)
    # a source shorter than BIN, an empty source, NaN samples: positions stay defined
    short = rng.uniform(-1, 1, size=300)
    pos = ref.positions(short, [0, 0, 1, 1], 512)
    assert all(0 <= p < 300 for p in pos)
    assert ref.positions(np.zeros(0), [0, 3, 1], 64) == [0, 3 * HOP, HOP]
    assert ref.positions(np.full(4000, np.nan), [0, 3, 1], 64) == [0, 3 * HOP, HOP]      # NaN scores never win


SINE_MAPS = {
    "stretch 2": lambda f: np.arange(f) // 2,
    "stretch 1.5": lambda f: (2 * np.arange(f)) // 3,
    "squeeze 2": lambda f: 2 * np.arange(f),
}


def sine_case(freq, kind, frames=40, rate=44100.0):
    """(source, map, output length): a pure sinusoid long enough for every map, 40 target frames."""
    fmap = SINE_MAPS[kind](frames)
    n_src = (int(fmap.max()) + 1) * HOP + BIN + 512
    x = np.sin(2.0 * np.pi * freq * np.arange(n_src) / rate)
    return x, fmap, (frames - 1) * HOP + BIN


def trimmed(y):
    return y[1024:y.size - 2048]


@pytest.mark.parametrize("freq", [97.0, 220.0, 313.0])
@pytest.mark.parametrize("kind", sorted(SINE_MAPS))
def test_a_sinusoid_stays_a_sinusoid(freq, kind):
    """Purity (wsola_ref.purity: the share of the output's energy that a least-squares sine + cosine at the source
    frequency explains) of the output without its first 1024 and last 2048 samples, S = 256.  Measured with the serial
    sums of the definition, over the nine cases: WSOLA 0.99411 (313 Hz, squeeze 2) ... 0.99997, the plain warp 0.00112
    ... 0.00331.  The bounds are conditions on the definition with room over those values, not a GPU tolerance."""
    x, fmap, n = sine_case(freq, kind)
    plain = warp_ref.warp_one(x, n, fmap)
    out, pos = ref.wsola_one(x, n, fmap, 256)
    p_plain, p_wsola = ref.purity(trimmed(plain), freq, 44100.0), ref.purity(trimmed(out), freq, 44100.0)
    print("%5.0f Hz %-12s plain %.5f wsola %.5f" % (freq, kind, p_plain, p_wsola))
    assert p_wsola >= 0.99
    assert p_plain <= 0.05
    assert all(abs(p - int(m) * HOP) <= 256 for p, m in zip(pos, fmap))


# ---- the inputs of tests/test_gpu_wsola_search.py: two statements of every answer, by construction and by the restatement

def _hold(cases, S):
    for c in cases:
        assert ref.positions(c.source, c.fmap, S) == c.expected, c.name
    kinds = collections.Counter(c.kind for c in cases)
    print("S %d: %d cases %s" % (S, len(cases), dict(kinds)))
    return kinds


@pytest.mark.parametrize("S", wc.PLANT_WIDTHS)
def test_planted_winners_and_ties_are_the_restatements(S):
    """Every case of the width, none sampled away (S = 512: 134 cases, 3.5 s)."""
    L = 2 * S + 1
    planted_at = set(wc.plant_indices(S))
    edges = {256 * r + 64 * w + lane for r in range(5) for w in range(4) for lane in (0, 63)}
    assert planted_at == {i for i in edges | {S, L - 2, L - 1} if i < L}
    kinds = _hold(wc.plant_cases(S), S)
    assert kinds["single winner"] == len(planted_at)
    assert kinds["tie: first against last"] == 1 and kinds["tie: three lags"] >= 1
    assert kinds["tie: d against -d"] >= 1 or S == 1                            # (S = 1: -1 against +1 is first against last)
    sets = dict((idx, kind) for kind, idx in wc.tie_sets(S))
    pairs = [idx for idx in sets if len(idx) == 2]
    assert (0, L - 1) in pairs and any(a + b == 2 * S and a for a, b in pairs) or S == 1
    assert any(a // 64 == b // 64 for a, b in pairs)                                            # two lanes of one wave
    assert any(a // 256 == b // 256 and a // 64 != b // 64 for a, b in pairs) or L <= 64        # two waves, one round
    assert any(b == a + 256 for a, b in pairs) or L <= 256                                      # one thread, two rounds
    assert any(a // 256 != b // 256 and (a // 64) % 4 != (b // 64) % 4 for a, b in pairs) or L <= 256
    assert all(b == a + 256 for a, b in pairs if sets[(a, b)] == "same thread, two rounds")
    assert all(a // 64 == b // 64 for a, b in pairs if sets[(a, b)] == "two lanes of a wave")
    assert all(a // 256 == b // 256 and a // 64 != b // 64 for a, b in pairs if sets[(a, b)] == "two waves of a round")
    assert all(a // 256 != b // 256 and (a // 64) % 4 != (b // 64) % 4 for a, b in pairs
               if sets[(a, b)] == "another wave and round")
    if S == 512:                                                                # the pair whose levelling pulse may not sit at lag +S
        with pytest.raises(ValueError):
            wc.planted(S, [-512, -511], "no room")
        assert sum(1 for idx in sets if idx[0] == 0 and idx[-1] != L - 1) >= 5


@pytest.mark.parametrize("S", wc.EDGE_WIDTHS)
def test_planted_edges_and_flat_sources_are_the_restatements(S):
    kinds = _hold(wc.edge_cases(S) + wc.flat_cases(S), S)
    for kind in ("lo = -nom", "hi inside the range", "only negative lags, lo", "only negative lags, all tied",
                 "no admissible lag mid-chain", "template beyond the source", "constant", "silent"):
        assert kinds[kind] >= 1, kind


@pytest.mark.parametrize("S", [s for s in wc.ODD_WIDTHS if s])
def test_the_odd_sample_sources_contain_the_steps_they_are_for(S):
    """On the restatement alone, at the seeds the GPU test uses.  Measured: S = 64: 161 searched steps, 28 with every
    score NaN, 1 with some NaN and a winner off lag 0, 3 with e == 0 on non-zero samples, 27 with e = +inf; S = 512: 14,
    22, 5, 34; 2 NaN samples of 45 919 at either width."""
    sounds = wc.odd_call()[0]
    assert len(sounds) == len(wc.ODD_KINDS) and all(x.size >= 8000 for x in sounds)
    assert np.isnan(sounds[0]).sum() == 1 and np.isposinf(sounds[1]).sum() == 1 and np.isneginf(sounds[2]).sum() == 1
    assert np.signbit(sounds[3][sounds[3] == 0.0]).sum() >= 200
    tiny = np.abs(sounds[4][sounds[4] != 0.0])
    assert (tiny < np.finfo(np.float64).tiny).sum() >= 200
    kinds, nans, total = wc.odd_walk(S)
    print("S %d: %s, %d NaN of %d samples" % (S, dict(kinds), nans, total))
    for kind in ("every score NaN", "some scores NaN, winner off lag 0", "e == 0 on non-zero samples", "e = +inf"):
        assert kinds[kind] >= 1, kind
    assert 2 * nans <= total
    plain = wc.odd_reference(None)
    assert 2 * int(np.isnan(plain).sum()) <= plain.size
