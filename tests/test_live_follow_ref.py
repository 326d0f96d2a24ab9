"""tests/live_follow_ref.py against tests/follow_ref.py (CPU only): the release rule of live envelope following is safe and
tight.  The restatement renders the offline definition on the consumed prefix at every call and hands out the slice the
closed-form counts name; here the concatenation over random cuts is held to the offline render of the whole, bit for bit --
so a settled gain or a released sample that a later sample could still change would show."""
import numpy as np
import pytest

import follow_ref as fr
import live_follow_ref as lf
from follow_ref import HOP


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pair(n, nx, seed):
    y, _, x, _ = fr.ragged_case([n], seed, [nx])
    return y, x


def _ref_lengths(n):
    return sorted({n, 0, n // 2, n + 300})


@pytest.mark.parametrize("n", fr.LENGTHS + (20 * HOP, 20 * HOP + 100))
def test_concatenation_over_random_cuts_is_the_offline_render(n):
    rng = np.random.default_rng(0x11FE + n)
    for nx in _ref_lengths(n):
        y, x = _pair(n, nx, 0xF011 + n + nx)
        want_out, want_g = fr.follow_one(y, x)
        cut_sets = [[], [(n, 0)], [(0, nx)]] + [lf.random_cuts(rng, n, nx, top) for top in (300, 700, 2000)]
        cut_sets += [[(m, m)] * (max(n, nx) // m + 1) for m in (1, 255, 256, 257, 513) if max(n, nx) // m < 400]
        for cuts in cut_sets:
            out, g = lf.run_cuts(y, x, cuts)
            assert _same(out, want_out) and _same(g, want_g), (n, nx, cuts[:4])


def test_counts_are_the_closed_form_whatever_the_cuts():
    rng = np.random.default_rng(0x11FF)
    y, x = _pair(20 * HOP + 100, 20 * HOP + 100, 0xF012)
    f = lf.LiveFollower(1)
    ay = ax = 0
    for my, mx in lf.random_cuts(rng, y.size, x.size, 600):
        (out, g), = f.push([y[ay:ay + my]], [x[ax:ax + mx]])
        before = (lf.released_hops(ay, ax), lf.settled(ay, ax))
        ay, ax = ay + my, ax + mx
        assert out.size == (lf.released_hops(ay, ax) - before[0]) * HOP and g.size == lf.settled(ay, ax) - before[1]
        h = min(ay, ax) // HOP
        assert f.counts() == ([ay], [ax], [max(0, h - 2) * HOP])
    out, g = f.flush(0)
    assert out.size == y.size - max(0, y.size // HOP - 2) * HOP
    assert f.lanes[0].settled == fr.boundaries(y.size) and f.lanes[0].ended
    empty = lf.LiveFollower(1)
    assert [a.size for a in empty.flush(0)] == [0, 0]                         # a lane flushed at ny = 0 releases nothing


def test_releasing_one_hop_earlier_changes_bits():
    """The rule is tight: with one hop less of look-ahead a gain is computed from a window whose last hop has not arrived."""
    y, x = _pair(20 * HOP, 20 * HOP, 0xF013)
    cuts = [(HOP, HOP)] * 20
    want_out, want_g = fr.follow_one(y, x)
    out, g = lf.run_cuts(y, x, cuts)
    assert _same(out, want_out) and _same(g, want_g)
    early_out, early_g = lf.run_cuts(y, x, cuts, hold_back=-1)
    assert early_out.shape == want_out.shape and early_g.shape == want_g.shape
    assert not _same(early_g, want_g) and not _same(early_out, want_out)
    # ... while one hop more only delays
    late_out, late_g = lf.run_cuts(y, x, cuts, hold_back=1)
    assert _same(late_out, want_out) and _same(late_g, want_g)


def test_consequence_1_live_equal_signals_and_powers_of_two():
    x = fr.sounding(20 * HOP + 100)
    cuts = [(513, 257)] * 12
    out, g = lf.run_cuts(x, x, cuts)
    assert np.all(g == 1.0) and _same(out, x)
    out, g = lf.run_cuts(x / 4.0, x, cuts, max_gain=4.0)
    assert np.all(g == 4.0) and _same(out, x)
    out, g = lf.run_cuts(x / 32.0, x, cuts, max_gain=8.0)
    assert np.all(g == 8.0) and _same(out, x / 4.0)


def test_consequence_4_live_silence():
    x = fr.sounding(10 * HOP + 7)
    zero = np.zeros(x.size)
    cuts = [(300, 300)] * 9
    out, g = lf.run_cuts(zero, x, cuts)
    assert np.all(g == fr.MAX_GAIN) and np.all(out == 0.0) and not np.signbit(out).any()
    out, g = lf.run_cuts(x, zero, cuts)
    assert np.all(g == 0.0) and np.all(out == 0.0)
    out, g = lf.run_cuts(zero, zero, cuts)
    assert np.all(g == 1.0) and np.all(out == 0.0)


def test_consequence_5_live_non_finite_samples():
    n = 12 * HOP + 40
    x = fr.sounding(n)
    y = x / 2.0
    cuts = [(257, 255)] * 13
    p = 5 * HOP + 17
    bad = y.copy()
    bad[p] = np.nan
    out, g = lf.run_cuts(bad, x, cuts)
    hit = fr.window_boundaries(p, n)
    assert 1 <= len(hit) <= 4 and np.all(g[hit] == 1.0)
    assert np.isnan(out[p]) and np.isfinite(np.delete(out, p)).all()
    clean = np.setdiff1d(np.arange(g.size), hit)
    assert np.all(g[clean] == 2.0)
    # an infinity in x: max_gain on the boundaries whose window holds it, but 1.0 where the window starts at that very sample
    q = 6 * HOP
    inf = x.copy()
    inf[q] = np.inf
    out, g = lf.run_cuts(y, inf, cuts)
    hit = fr.window_boundaries(q, n)
    starts = [b for b in hit if (b - 2) * HOP == q]
    assert len(starts) == 1 and g[starts[0]] == 1.0
    assert all(g[b] == fr.MAX_GAIN for b in hit if b not in starts)
    assert np.isfinite(out).all()


def test_lanes_are_independent():
    rng = np.random.default_rng(0x1200)
    pairs = [_pair(n, n, 0xF014 + n) for n in (1000, 4097, 20 * HOP)]
    f = lf.LiveFollower(3)
    at = [0, 0, 0]
    outs, gs = [[], [], []], [[], [], []]
    while any(a < p[0].size for a, p in zip(at, pairs)):
        m = [int(rng.integers(0, 600)) for _ in pairs]
        res = f.push([p[0][a:a + k] for p, a, k in zip(pairs, at, m)], [p[1][a:a + k] for p, a, k in zip(pairs, at, m)])
        at = [min(a + k, p[0].size) for a, k, p in zip(at, m, pairs)]
        for l, (o, g) in enumerate(res):
            outs[l].append(o)
            gs[l].append(g)
    for l, (y, x) in enumerate(pairs):
        o, g = f.flush(l)
        want_out, want_g = fr.follow_one(y, x)
        assert _same(np.concatenate(outs[l] + [o]), want_out) and _same(np.concatenate(gs[l] + [g]), want_g)
    f.reset(1)
    assert f.counts() == ([1000, 0, 20 * HOP], [1000, 0, 20 * HOP], [1000, 0, 20 * HOP])
