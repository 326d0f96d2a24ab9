"""ssym_follow_envelope at the shapes where its two kernels can go wrong, against tests/follow_ref.py bit for bit: ragged
batches around every hop, window and chunk edge, the gain kernel's own block edge, empty targets, references of every
relation to their target, every target alone among NaN, the consequences of the definition on the GPU, the extremes of
max_gain, and batches of many short targets for the block table.

The gain kernel (csrc/follow.hip) gives one workgroup BLOCK = kFollowBlock = 32 consecutive boundaries; a target of n samples
has ceil(n / 256) + 1 boundaries, so the last length that fits one block is EDGE = (BLOCK - 1) * HOP = 7936 samples, and
3 * BLOCK boundaries end at (3 * BLOCK - 1) * HOP = 24320.  The apply kernel's chunk is 4096 samples."""
import numpy as np
import pytest

import follow_gpu as fg
import follow_ref as fr
from follow_ref import HOP
from soundsym_amd import Engine

pytestmark = pytest.mark.gpu

BLOCK = 32                                   # kFollowBlock of csrc/follow.hip
EDGE = (BLOCK - 1) * HOP                     # the longest target of one block
EDGE3 = (3 * BLOCK - 1) * HOP                # ... of three
MIXED = (0, 1, 2, 255, 256, 257, 511, 512, 513, 767, 1023, 1024, 1025, 4095, 4096, 4097)
PLACEMENTS = [(False, False, False), (True, True, True)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="dtw", dtype="f64")
    yield e
    e.close()


def check(eng, args, max_gain=8.0, placements=PLACEMENTS, want=None):
    want = fr.follow(*args, max_gain) if want is None else want
    for y_dev, x_dev, out_dev in placements:
        fg.assert_matches(fg.call(eng, *args, max_gain, y_dev, x_dev, out_dev), *want, what=(y_dev, x_dev, out_dev))
    return want


def test_the_edges_named_above():
    assert fr.boundaries(EDGE) == BLOCK and fr.boundaries(EDGE + 1) == BLOCK + 1
    assert fr.boundaries(EDGE3) == 3 * BLOCK and fr.boundaries(EDGE3 + 1) == 3 * BLOCK + 1


def test_a_ragged_batch_of_every_edge_length(eng):
    order = np.random.default_rng(0xF0111).permutation(len(MIXED))
    lengths = [MIXED[i] for i in order]
    _, _, g = check(eng, fr.ragged_case(lengths))
    assert g.size == sum(fr.boundaries(n) for n in MIXED)


def test_the_gain_kernels_block_edge_and_three_blocks_of_it(eng):
    lengths = [EDGE - 1, EDGE, EDGE + 1, 3, EDGE3 - 1, EDGE3, EDGE3 + 1]
    check(eng, fr.ragged_case(lengths, seed=0xF0112))


@pytest.mark.parametrize("lengths", [(0, 0, 513, 300), (513, 0, 0, 300, 0, 1), (513, 300, 0), (0, 700, 0), (0, 0, 0, 1)])
def test_empty_targets_first_in_the_middle_and_last(eng, lengths):
    check(eng, fr.ragged_case(list(lengths), seed=0xF0113))


def test_references_of_every_relation_to_their_target(eng):
    """Equal, none, one sample short, ending in the middle of a window, longer with a NaN surplus."""
    lengths = [1000, 1000, 1000, 1000, 1000, 4097, 4097, 1, 1]
    ref_lengths = [1000, 0, 999, 600, 1300, 4096, 5000, 0, 9]
    y, off, x, r_off = fr.ragged_case(lengths, seed=0xF0114, ref_lengths=ref_lengths)
    want = check(eng, (y, off, x, r_off))
    for t, (n, nx) in enumerate(zip(lengths, ref_lengths)):
        if nx > n:
            x[int(r_off[t]) + n:int(r_off[t + 1])] = np.nan             # what lies at or beyond n is never read
    check(eng, (y, off, x, r_off), want=want)
    g_off = fr.gain_offsets(off)
    assert np.all(want[2][g_off[1]:g_off[2]] == 0.0) and np.all(want[2][g_off[3]:g_off[4]] > 0.0)      # 600 of 1000: every window meets some


def test_every_target_alone_among_nan(eng):
    lengths = [MIXED[i] for i in np.random.default_rng(0xF0115).permutation(len(MIXED))]
    ref_lengths = [n + (t % 3) * 5 - 5 if n > 5 else n for t, n in enumerate(lengths)]
    y, off, x, r_off = fr.ragged_case(lengths, seed=0xF0115, ref_lengths=ref_lengths)
    want = check(eng, (y, off, x, r_off), placements=PLACEMENTS[:1])
    g_off = fr.gain_offsets(off)
    for t, n in enumerate(lengths):
        if n == 0:
            continue
        a, b, ra, rb = int(off[t]), int(off[t + 1]), int(r_off[t]), int(r_off[t + 1])
        y2, x2 = np.full(y.size, np.nan), np.full(x.size, np.nan)
        y2[a:b], x2[ra:ra + min(n, rb - ra)] = y[a:b], x[ra:ra + min(n, rb - ra)]
        res = fg.call(eng, y2, off, x2, r_off, 8.0, t % 2 == 0, t % 2 == 0, t % 2 == 0)
        assert res.rc == 0 and res.slack_intact
        assert fg.same_bits(res.out[a:b], want[0][a:b]) and np.array_equal(res.pcm[a:b], want[1][a:b]), t
        assert fg.same_bits(res.gain[g_off[t]:g_off[t + 1]], want[2][g_off[t]:g_off[t + 1]]), t
        alone = fg.call(eng, y[a:b], [0, n], x[ra:rb], [0, rb - ra], 8.0)
        assert fg.same_bits(alone.out, want[0][a:b]) and fg.same_bits(alone.gain, want[2][g_off[t]:g_off[t + 1]]), t


# ---- the consequences of the definition, on the GPU ---------------------------------------------------------------------

def batch(parts_y, parts_x):
    off = np.concatenate([[0], np.cumsum([p.size for p in parts_y])]).astype(np.uint64)
    r_off = np.concatenate([[0], np.cumsum([p.size for p in parts_x])]).astype(np.uint64)
    return np.concatenate(parts_y), off, np.concatenate(parts_x), r_off


def test_identity(eng):
    """Consequence 1, every length of the restatement's list and the block edges in one batch per scale."""
    xs = [fr.sounding(n) for n in fr.LENGTHS + (EDGE, EDGE + 1)]
    for scale, max_gain, g_want, out_scale in ((1.0, 8.0, 1.0, 1.0), (4.0, 4.0, 4.0, 1.0), (4.0, 1024.0, 4.0, 1.0), (32.0, 8.0, 8.0, 4.0)):
        args = batch([x / scale for x in xs], xs)
        res = fg.call(eng, *args, max_gain)
        fg.assert_matches(res, *fr.follow(*args, max_gain))
        assert np.all(res.gain == g_want) and fg.same_bits(res.out, args[2] / out_scale), scale


def test_step(eng):
    """Consequence 2."""
    y, x, max_gain = fr.step_case()
    res = fg.call(eng, y, [0, y.size], x, [0, x.size], max_gain, True, True, True)
    fg.assert_matches(res, *fr.follow(y, [0, y.size], x, [0, x.size], max_gain))
    assert np.all(res.gain[:15] == 2.0) and np.all(res.gain[18:] == 16.0)
    differ = np.flatnonzero(fg.bits(res.out) != fg.bits(x))
    assert differ.size and differ.min() >= 3585 and differ.max() <= 4607


def test_any_constant_scale(eng):
    """Consequence 3, to its bound of 2^-40."""
    xs = [fr.sounding(n) for n in fr.LENGTHS + (EDGE + 1,) if n]
    for c in (0.13, 1.0 / 3.0, 0.999, 1.7, 41.0):
        args = batch([c * x for x in xs], xs)
        res = fg.call(eng, *args, 8.0)
        fg.assert_matches(res, *fr.follow(*args, 8.0))
        err = np.abs(res.out - args[2])
        print("constant scale %g: worst relative error %.3g" % (c, float(np.max(err / np.abs(args[2])))))
        assert np.all(err <= fr.BOUND * np.abs(args[2])), c


def test_silence(eng):
    """Consequence 4."""
    xs = [fr.sounding(n) for n in fr.LENGTHS if n]
    zeros = [np.zeros(x.size) for x in xs]
    res = fg.call(eng, *batch(zeros, xs), 8.0)
    assert res.rc == 0 and np.all(res.gain == 8.0) and fg.same_bits(res.out, np.concatenate(zeros))
    res = fg.call(eng, *batch(xs, zeros), 8.0)
    assert res.rc == 0 and np.all(res.gain == 0.0) and np.all(res.out == 0.0) and np.all(res.pcm == 0)
    args = batch(xs, zeros)
    fg.assert_matches(res, *fr.follow(*args, 8.0))                    # the signs of the zeros too
    res = fg.call(eng, *batch(zeros, zeros), 8.0)
    assert res.rc == 0 and np.all(res.gain == 1.0) and fg.same_bits(res.out, np.concatenate(zeros))


def test_non_finite_samples(eng):
    """Consequence 5: a NaN in y, an infinity in x."""
    n = 4097
    x = fr.sounding(n)
    y = x / 2.0
    for p in (0, 300, 1024, 2500, 4095, 4096):
        hit = fr.window_boundaries(p, n)
        bad = y.copy()
        bad[p] = np.nan
        res = fg.call(eng, bad, [0, n], x, [0, n], 8.0)
        assert res.rc == 0 and fg.same_bits(res.gain, fr.gains(bad, x, 8.0))
        clean = np.ones(res.gain.size, dtype=bool)
        clean[hit] = False
        assert np.all(res.gain[hit] == 1.0) and np.all(res.gain[clean] == 2.0)
        assert np.isnan(res.out[p]) and np.isnan(res.out).sum() == 1 and res.pcm[p] == 0
        keep = np.arange(n) != p
        assert fg.same_bits(res.out[keep], fr.follow_one(bad, x, 8.0)[0][keep])
        loud = x.copy()
        loud[p] = np.inf
        res = fg.call(eng, y, [0, n], loud, [0, n], 8.0)
        at_start = [b for b in hit if (b - 2) * HOP == p]
        fg.assert_matches(res, *fr.follow(y, [0, n], loud, [0, n], 8.0))
        assert np.all(res.gain[[b for b in hit if b not in at_start]] == 8.0) and np.all(res.gain[at_start] == 1.0)
        assert np.all(res.gain[clean] == 2.0) and np.isfinite(res.out).all()


@pytest.mark.parametrize("max_gain", [1.0, 8.0, 2.0 ** 30])
def test_max_gain_at_its_ends(eng, max_gain):
    lengths = [1000, 4097, 300, 513]
    y, off, x, r_off = fr.ragged_case(lengths, seed=0xF0116)
    y[int(off[1]) + 1000:int(off[1]) + 3000] = 0.0                    # a silent stretch under a sounding target
    y[int(off[2]):int(off[3])] *= 1e-12
    y[:int(off[1])] *= 1000.0                                         # ... and a reconstruction far too loud
    want = check(eng, (y, off, x, r_off), max_gain)
    assert want[2].max() == max_gain and np.all(want[2] <= max_gain) and want[2].min() < max_gain


@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 700])
def test_many_short_targets(eng, count):
    """The block table: one entry per target, and two for those that reach past 32 boundaries (none here does)."""
    rng = np.random.default_rng(0xF0117 + count)
    lengths = rng.integers(1, 601, size=count).tolist()
    ref_lengths = [int(n + rng.integers(-3, 4)) if n > 3 else n for n in lengths]
    check(eng, fr.ragged_case(lengths, seed=0xF0118 + count, ref_lengths=ref_lengths))


def test_more_targets_than_one_launch_of_the_apply_kernel_takes(eng):
    """The apply kernel has the targets on its grid's y extent, kFollowGridY = 65535 of them per launch (csrc/follow.hip):
    65535 + 3 targets of 1 ... 3 samples are two launches.  The targets around the seam and at both ends against the
    restatement (a target's result does not depend on the batch: test_every_target_alone_among_nan), every sample written."""
    grid_y = 65535                               # kFollowGridY of csrc/follow.hip
    n = grid_y + 3
    rng = np.random.default_rng(0xF0119)
    lengths = rng.integers(1, 4, size=n)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    x = 0.1 * rng.standard_normal(int(off[-1]))
    y = x * np.repeat(np.exp(rng.uniform(-3.0, 1.0, size=n)), lengths)
    g_off = fr.gain_offsets(off)
    for dev in (False, True):
        res = fg.call(eng, y, off, x, off, 8.0, dev, dev, dev)
        assert res.rc == 0 and res.slack_intact
        assert not np.any(res.out == fg.SENTF) and not np.any(res.pcm == fg.SENT32) and not np.any(res.gain == fg.SENTG)
        for a, b in ((0, 40), (grid_y - 40, grid_y + 3)):
            sa, sb = int(off[a]), int(off[b])
            want = fr.follow(y[sa:sb], off[a:b + 1] - off[a], x[sa:sb], off[a:b + 1] - off[a], 8.0)
            assert fg.same_bits(res.out[sa:sb], want[0]) and np.array_equal(res.pcm[sa:sb], want[1]), (dev, a)
            assert fg.same_bits(res.gain[g_off[a]:g_off[b]], want[2]), (dev, a)
