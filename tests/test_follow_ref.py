"""tests/follow_ref.py on the CPU: the vectorised restatement against the definition read aloud, and the consequences of the
definition that its docstring lists, at every length of follow_ref.LENGTHS."""
import numpy as np
import pytest

import follow_ref as fr
from follow_ref import HOP


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_the_geometry():
    assert [fr.boundaries(n) for n in (0, 1, 255, 256, 257, 512, 513)] == [0, 2, 2, 2, 3, 3, 4]
    assert fr.gain_offsets([0, 0, 1, 258, 258]).tolist() == [0, 0, 2, 5, 5]
    assert fr.window_boundaries(0, 4097) == [0, 1, 2] and fr.window_boundaries(300, 4097) == [0, 1, 2, 3]
    assert fr.window_boundaries(1024, 4097) == [3, 4, 5, 6] and fr.window_boundaries(4096, 4097) == [15, 16, 17]
    assert same_bits(fr.fitted([1.0, 2.0, 3.0], 2), np.array([1.0, 2.0])) and same_bits(fr.fitted([1.0], 3), np.array([1.0, 0.0, 0.0]))


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 513, 1000])
def test_the_vectorised_energies_are_the_definition_read_aloud(n):
    s = fr.sounding(n)
    assert same_bits(fr.energies(s), fr.energies_scalar(s))
    if n > 300:
        s[7], s[n - 1], s[256] = np.nan, np.inf, -0.0
        with np.errstate(all="ignore"):
            a, b = fr.energies(s), fr.energies_scalar(s)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("n", fr.LENGTHS)
def test_identity(n):
    """Consequence 1."""
    x = fr.sounding(n)
    out, g = fr.follow_one(x, x)
    assert g.size == fr.boundaries(n) and np.all(g == 1.0) and same_bits(out, x)
    out, g = fr.follow_one(x / 4.0, x, 4.0)
    assert np.all(g == 4.0) and same_bits(out, x)
    out, g = fr.follow_one(x / 4.0, x, 1024.0)
    assert np.all(g == 4.0) and same_bits(out, x)
    out, g = fr.follow_one(x / 32.0, x, 8.0)
    assert np.all(g == 8.0) and same_bits(out, x / 4.0)


def test_step():
    """Consequence 2."""
    y, x, max_gain = fr.step_case()
    out, g = fr.follow_one(y, x, max_gain)
    assert g.size == 33 and np.all(g[:15] == 2.0) and np.all(g[18:] == 16.0)
    assert np.all((g[15:18] > 2.0) & (g[15:18] < 16.0))
    differ = np.flatnonzero(bits(out) != bits(x))
    assert differ.size > 900 and differ.min() >= 3585 and differ.max() <= 4607
    assert same_bits(out[:3585], x[:3585]) and same_bits(out[4608:], x[4608:])


@pytest.mark.parametrize("n", [n for n in fr.LENGTHS if n])
@pytest.mark.parametrize("c", [0.13, 1.0 / 3.0, 0.999, 1.7, 41.0])
def test_any_constant_scale(n, c):
    """Consequence 3."""
    x = fr.sounding(n)
    out, g = fr.follow_one(c * x, x, 8.0)
    assert c > 1.0 / 8.0 and np.all(g < 8.0)
    err = np.abs(out - x)
    assert np.all(err <= fr.BOUND * np.abs(x)), float(np.max(err / np.abs(x)))


@pytest.mark.parametrize("n", fr.LENGTHS)
def test_silence(n):
    """Consequence 4."""
    x, zero = fr.sounding(n), np.zeros(n)
    out, g = fr.follow_one(zero, x, 8.0)
    assert np.all(g == 8.0) and same_bits(out, zero)
    out, g = fr.follow_one(x, zero, 8.0)
    assert np.all(g == 0.0) and np.all(out == 0.0) and same_bits(np.abs(out), zero)
    out, g = fr.follow_one(x, np.zeros(0), 8.0)          # a reference of no samples reads as silence
    assert np.all(g == 0.0) and np.all(out == 0.0)
    out, g = fr.follow_one(zero, zero, 8.0)
    assert np.all(g == 1.0) and same_bits(out, zero)
    out, g = fr.follow_one(-zero, zero, 8.0)
    assert np.all(g == 1.0) and same_bits(out, -zero)


@pytest.mark.parametrize("n", [n for n in fr.LENGTHS if n])
def test_non_finite_samples(n):
    """Consequence 5, the samples."""
    x = fr.sounding(n)
    y = x / 2.0
    for p in sorted({0, n // 2, n - 1, min(n - 1, 256), min(n - 1, 300)}):
        hit = fr.window_boundaries(p, n)
        assert 1 <= len(hit) <= 4
        bad = y.copy()
        bad[p] = np.nan
        out, g = fr.follow_one(bad, x, 8.0)
        clean = np.ones(g.size, dtype=bool)
        clean[hit] = False
        assert np.all(g[hit] == 1.0) and np.all(g[clean] == 2.0)
        assert np.isnan(out[p]) and np.isnan(out).sum() == 1
        far = np.ones(n, dtype=bool)
        far[max(0, (min(hit) - 1) * HOP):(max(hit) + 1) * HOP] = False
        assert same_bits(out[far], x[far])
        loud = x.copy()
        loud[p] = np.inf
        out, g = fr.follow_one(y, loud, 8.0)
        at_start = [b for b in hit if (b - 2) * HOP == p]            # w[0] = 0: 0 * inf is NaN, the gain 1
        assert np.all(g[[b for b in hit if b not in at_start]] == 8.0) and np.all(g[at_start] == 1.0)
        assert np.all(g[clean] == 2.0) and np.isfinite(out).all()


def test_no_read_leaves_a_target():
    """Consequence 5, the batch: every other target's samples NaN, a reference's surplus NaN."""
    lengths = list(fr.LENGTHS)
    ref_lengths = [n + 3 if t % 2 else n for t, n in enumerate(lengths)]
    y, off, x, r_off = fr.ragged_case(lengths, ref_lengths=ref_lengths)
    out, pcm, g = fr.follow(y, off, x, r_off, 8.0)
    g_off = fr.gain_offsets(off)
    assert g.size == g_off[-1] and np.isfinite(out).all() and out.size == pcm.size == int(off[-1])
    for t, n in enumerate(lengths):
        a, b, ra, rb = int(off[t]), int(off[t + 1]), int(r_off[t]), int(r_off[t + 1])
        y2, x2 = np.full(y.size, np.nan), np.full(x.size, np.nan)
        y2[a:b], x2[ra:ra + min(n, rb - ra)] = y[a:b], x[ra:ra + min(n, rb - ra)]
        out2, pcm2, g2 = fr.follow(y2, off, x2, r_off, 8.0)
        assert same_bits(out2[a:b], out[a:b]) and np.array_equal(pcm2[a:b], pcm[a:b])
        assert same_bits(g2[g_off[t]:g_off[t + 1]], g[g_off[t]:g_off[t + 1]])
        alone = fr.follow_one(y[a:b], x[ra:rb], 8.0)
        assert same_bits(alone[0], out[a:b]) and same_bits(alone[1], g[g_off[t]:g_off[t + 1]])


def test_a_short_reference_is_silence_from_its_end():
    y = fr.sounding(2000) / 2.0
    x = fr.sounding(2000)
    out, g = fr.follow_one(y, x[:1000], 8.0)
    want, gw = fr.follow_one(y, np.concatenate([x[:1000], np.zeros(1000)]), 8.0)
    assert same_bits(out, want) and same_bits(g, gw)
    # windows [-512, 512), [256, 1280) and [1536, 2000): inside the reference, across its end, beyond it
    assert g[0] == 2.0 and g[-1] == 0.0 and 0.0 < g[3] < 2.0
