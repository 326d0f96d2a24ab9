"""ssym_follower_* at the shapes where its kernels and its plan can go wrong, every call against tests/live_follow_ref.py bit
for bit: lane counts around the wave and the most lanes there are, one call settling 0 ... 65 boundaries on different lanes,
whole sounds flushed with nothing released before, every relation of nx to ny at the flush, the ring wrapped at its least
capacity, grown under a starved lane and reused, the logs grown and reused small, non-finite samples, a lane among NaN
neighbours, reset and reuse, a flush that releases nothing.

The ring holds at least RING_MIN = 2048 samples per lane and signal; the gain kernel gives one workgroup BLOCK = 32
boundaries; the apply kernel's chunk is 4096 samples."""
import numpy as np
import pytest

import follow_gpu as fg
import follow_ref as fr
import follower_gpu as wg
import live_follow_ref as lf
from follow_ref import HOP
from soundsym_amd import Engine
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="dtw", dtype="f64")
    yield e
    e.close()


def _pair(n, nx, seed):
    y, _, x, _ = fr.ragged_case([n], seed, [nx])
    return y, x


def _whole(live, pairs, lanes=None):
    """every lane's concatenation against the offline render of what it was fed"""
    for l in (range(len(pairs)) if lanes is None else lanes):
        out, gain = live.total(l)
        want_out, want_g = fr.follow_one(*pairs[l], live.ref.max_gain)
        assert fg.same_bits(out, want_out) and fg.same_bits(gain, want_g), l


@pytest.mark.parametrize("n_lanes", [1, 63, 64, 65, 300])
def test_lane_counts_around_the_wave(eng, n_lanes):
    base_y, base_x = _pair(6 * HOP + 90, 6 * HOP + 90, 0xF0121)
    pairs = [(base_y * (1.0 + l % 7), np.roll(base_x, l)) for l in range(n_lanes)]
    pairs = [(y[:y.size - (l % 5) * 100], x[:x.size - (l % 3) * 300]) for l, (y, x) in enumerate(pairs)]
    live = wg.Live(eng, n_lanes)
    wg.feed(live, pairs, [(700, 300), (0, 900), (513, 257)], "lanes")
    for l in sorted({0, n_lanes // 2, n_lanes - 1}):
        live.flush(l, "lanes flush")
    _whole(live, pairs, sorted({0, n_lanes // 2, n_lanes - 1}))
    live.close()


def test_the_most_lanes_with_three_of_them_fed(eng):
    n_lanes = lf.MAX_LANES
    fed = (0, 8191, n_lanes - 1)
    pairs = {l: _pair(5 * HOP + 30 * i, 5 * HOP + 30 * i, 0xF0122 + i) for i, l in enumerate(fed)}
    live = wg.Live(eng, n_lanes)
    empty = np.zeros(0)
    for a, b in ((0, 700), (700, 1400), (1400, 5000)):               # (each push within the least ring: there is no other at 16 384 lanes)
        live.push([pairs[l][0][a:b] if l in pairs else None for l in range(n_lanes)],
                  [pairs[l][1][a:b] if l in pairs else None for l in range(n_lanes)], "most lanes")
    for l in fed:
        live.flush(l, "most lanes flush")
        out, gain = live.total(l)
        want_out, want_g = fr.follow_one(*pairs[l])
        assert fg.same_bits(out, want_out) and fg.same_bits(gain, want_g)
    assert live.total(1)[0].size == 0 and empty.size == 0
    over = wg.Follower(eng, n_lanes + 1)
    assert over.rc == nat.SSYM_E_UNSUPPORTED and over.ptr is None and "16384" in over.message
    live.close()


def test_one_call_settles_0_1_31_32_33_64_and_65_boundaries(eng):
    counts = (0, 1, 31, 32, 33, 64, 65)
    pairs = [_pair((c + 1) * HOP + 5 if c else 300, (c + 1) * HOP + 77 if c else 100, 0xF0123 + c) for c in counts]
    live = wg.Live(eng, len(counts))
    live.push([y for y, _ in pairs], [x for _, x in pairs], "blocks")
    logs = live.fl.read()
    assert [int(b - a) for a, b in zip(logs.g_off[:-1], logs.g_off[1:])] == list(counts)
    assert [int(b - a) for a, b in zip(logs.off[:-1], logs.off[1:])] == [max(0, c - 1) * HOP for c in counts]
    for l in range(len(counts)):
        live.flush(l, "blocks flush")
    _whole(live, pairs)
    live.close()


def test_whole_sounds_flushed_with_nothing_released_before(eng):
    """every length of follow_ref.LENGTHS with only y fed (nothing settles before the flush), and with both fed short"""
    lengths = fr.LENGTHS
    pairs = [_pair(n, n, 0xF0124 + n) for n in lengths]
    live = wg.Live(eng, len(lengths))
    live.push([y for y, _ in pairs], [x[:min(x.size, 511)] for _, x in pairs], "whole y")
    assert live.fl.counts()[2] == [0] * len(lengths)
    live.push([None] * len(lengths), [x[min(x.size, 511):] if x.size < 1000 else None for _, x in pairs], "rest of short x")
    fed = [(y, x if x.size < 1000 else x[:511]) for y, x in pairs]
    for l in range(len(lengths)):
        live.flush(l, "whole flush")
    _whole(live, fed)
    live.close()


def test_every_relation_of_nx_to_ny_at_the_flush(eng):
    n = 9 * HOP + 130
    shapes = [(n, n - 1), (n, n - 700), (n, n + 900), (n, 0), (0, n), (0, 0), (n, n), (5, 3000), (300, 256), (256, 300)]
    pairs = [_pair(ny, nx, 0xF0125 + i) for i, (ny, nx) in enumerate(shapes)]
    for _, x in pairs:
        x[min(x.size, n):] = np.nan                      # x at or beyond n is dropped unread -- for the lanes that end at ny = n
    pairs[4] = (pairs[4][0], fr.sounding(n))             # (ny = 0: nothing is released whatever x holds)
    live = wg.Live(eng, len(shapes))
    wg.feed(live, pairs, [(600, 900), (900, 600), (1000, 1000)], "relations")
    for l in range(len(shapes)):
        live.flush(l, "relations flush")
    # the restatement reads x as the offline definition does; here the offline render itself, with the surplus cut away
    for l, (y, x) in enumerate(pairs):
        out, gain = live.total(l)
        want_out, want_g = fr.follow_one(y, x[:y.size])
        assert fg.same_bits(out, want_out) and fg.same_bits(gain, want_g), shapes[l]
    assert live.total(4)[0].size == live.total(5)[0].size == 0 and live.total(4)[1].size == 0
    live.close()


def test_a_flush_that_releases_nothing_and_a_push_of_nothing(eng):
    live = wg.Live(eng, 2)
    live.push([None, None], [None, None], "nothing")
    live.flush(0, "empty flush")
    logs = live.fl.read()
    assert list(logs.off) == [0, 0, 0] and list(logs.g_off) == [0, 0, 0]
    live.push([None, np.ones(10)], [None, None], "beside an ended lane")
    assert live.fl.counts() == ([0, 10], [0, 0], [0, 0])
    live.close()


def test_the_ring_wraps_at_its_least_capacity(eng):
    """40 pushes of 512 samples: 20 480 samples through a ring of 2048, ten times round, on two lanes with other phases"""
    n = 40 * 512
    pairs = [_pair(n, n, 0xF0126), _pair(n - 300, n - 300, 0xF0127)]
    live = wg.Live(eng, 2)
    wg.feed(live, pairs, [(512, 512)] * 40, "wrap")
    live.flush(0, "wrap flush")
    live.flush(1, "wrap flush")
    _whole(live, pairs)
    live.close()


def test_the_ring_grows_under_a_starved_lane_and_is_reused(eng):
    """lane 0 receives 10 000 samples of y and no x: the ring grows to 16 384 while lane 1 is in mid-flight and holds a
    stretch that wraps; then x arrives, everything settles at once (39 hops: two blocks), and both lanes go on"""
    pairs = [_pair(14000, 14000, 0xF0128), _pair(9000, 9000, 0xF0129)]
    y0, x0 = pairs[0]
    y1, x1 = pairs[1]
    live = wg.Live(eng, 2)
    for a in range(0, 3000, 500):
        live.push([None, y1[a:a + 500]], [None, x1[a:a + 500]], "before the growth")
    for a in range(0, 10000, 2500):
        live.push([y0[a:a + 2500], y1[3000 + a // 5:3500 + a // 5]], [None, x1[3000 + a // 5:3500 + a // 5]], "starved")
    assert live.fl.counts()[2][0] == 0
    live.push([None, None], [x0[:10000], None], "x arrives")
    assert live.fl.counts()[2][0] == 37 * HOP
    live.push([y0[10000:], y1[5000:]], [x0[10000:], x1[5000:]], "after the growth")
    live.flush(0, "grown flush")
    live.flush(1, "grown flush")
    _whole(live, pairs)
    # the lanes again, in the grown ring
    live.reset(0)
    live.reset(1)
    wg.feed(live, pairs, [(3000, 3000)] * 3, "reused ring")
    live.flush(0)
    live.flush(1)
    _whole(live, pairs)
    live.close()


def test_the_logs_grow_and_are_reused_small(eng):
    big, small = _pair(40000, 40000, 0xF012A), _pair(3 * HOP + 9, 3 * HOP + 9, 0xF012B)
    live = wg.Live(eng, 1)
    live.push([small[0][:2 * HOP]], [small[1][:2 * HOP]], "small")
    live.push([small[0][2 * HOP:]], [small[1][2 * HOP:]], "small")
    live.flush(0, "small flush")
    live.reset(0)
    live.push([big[0]], [big[1]], "big")                       # 154 hops and 155 boundaries in one call
    live.flush(0, "big flush")
    _whole(live, [big])
    live.reset(0)
    wg.feed(live, [small], [(300, 300)] * 2, "small again")
    live.flush(0, "small again flush")
    _whole(live, [small])
    live.close()


def test_non_finite_samples(eng):
    """consequence 5, live: a NaN in y costs the boundaries whose window holds it and that sample alone; an infinity in x
    meets max_gain -- and 1.0 where the window starts at that very sample"""
    n = 12 * HOP + 40
    x = fr.sounding(n)
    y = x / 2.0
    p, q = 5 * HOP + 17, 6 * HOP
    bad_y, bad_x = y.copy(), x.copy()
    bad_y[p] = np.nan
    bad_x[q] = np.inf
    neg = x.copy()
    neg[7 * HOP + 3] = -np.inf
    pairs = [(bad_y, x), (y, bad_x), (y, neg)]
    live = wg.Live(eng, 3)
    wg.feed(live, pairs, [(257, 255)] * 13, "non-finite")
    for l in range(3):
        live.flush(l, "non-finite flush")
    _whole(live, pairs)
    out, gain = live.total(0)
    hit = fr.window_boundaries(p, n)
    assert np.all(gain[hit] == 1.0) and np.isnan(out[p]) and np.isfinite(np.delete(out, p)).all()
    assert np.all(gain[np.setdiff1d(np.arange(gain.size), hit)] == 2.0)
    out, gain = live.total(1)
    hit = fr.window_boundaries(q, n)
    assert [gain[b] for b in hit] == [8.0 if (b - 2) * HOP != q else 1.0 for b in hit] and np.isfinite(out).all()
    live.close()


def test_a_lane_whose_neighbours_are_all_nan_keeps_its_bits(eng):
    pair = _pair(7 * HOP + 50, 7 * HOP + 50, 0xF012C)
    nan = (np.full(8 * HOP, np.nan), np.full(8 * HOP, np.nan))
    cuts = [(600, 450), (450, 600), (513, 513)]
    alone = wg.Live(eng, 1)
    wg.feed(alone, [pair], cuts, "alone")
    alone.flush(0)
    among = wg.Live(eng, 3)
    wg.feed(among, [nan, pair, nan], cuts, "among NaN")
    for l in range(3):
        among.flush(l)
    assert fg.same_bits(among.total(1)[0], alone.total(0)[0]) and fg.same_bits(among.total(1)[1], alone.total(0)[1])
    assert np.isnan(among.total(0)[0]).all() and np.all(among.total(2)[1] == 1.0)
    _whole(alone, [pair])
    alone.close()
    among.close()


def test_reset_and_reuse_of_a_lane(eng):
    first, second = _pair(2000, 2000, 0xF012D), _pair(5 * HOP + 1, 5 * HOP + 1, 0xF012E)
    other = _pair(3000, 3000, 0xF012F)
    live = wg.Live(eng, 2)
    wg.feed(live, [first, other], [(900, 900)], "first")          # lane 0 is reset in mid-flight, unflushed, with hops released
    assert live.fl.counts()[2][0] > 0
    live.reset(0)
    assert live.fl.counts() == ([0, 3000], [0, 3000], [0, 9 * HOP])
    live.push([second[0], None], [second[1], None], "second")
    live.flush(0, "second flush")
    live.flush(1, "other flush")
    _whole(live, [second, other])
    live.reset(0)                                                  # ... and after its flush
    live.push([first[0], None], [first[1], None], "first again")
    live.flush(0, "first again flush")
    _whole(live, [first], [0])
    live.close()
