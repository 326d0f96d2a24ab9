"""The conditions of every near-tie case (tests/near_tie_cases.py), held on the CPU oracle alone, so that no test of
tests/test_gpu_near_ties.py can be vacuous.  These are conditions on the INPUTS: where one fails, the builder or the seed
is wrong, not a kernel.

Counts: a first-minimum case has at least 24 blind targets, 8 of them with the nearer contender at the higher index and
8 at the lower one, and 24 inside targets, 4 in every decade it claims.  The case of sources of 150 and 300 frames
("long", 32 targets) holds half of each: 12 blind (4 and 4), 12 inside (2 per decade).  On the cases beyond the filter's
reach the filter is blind whatever the gap: their 32 targets are spread over the decades 1e-9 ... 1e-4, 4 in each, and
count as blind for the placement.  test_counts_per_rung prints the counts per rung.
"""
import numpy as np
import pytest

import near_tie_cases as ntc
import topk_ref as ref

NAMES = list(ntc.SPECS)


@pytest.fixture(params=NAMES)
def case(request, oracle):
    return ntc.build(request.param)


def test_counts_per_rung(case, capsys):
    c = case
    cnt, dec = c.counts(), c.decade_counts()
    with capsys.disabled():                               # shown whether or not output is captured
        print("\n%-12s %3d sources %2d targets  (rung: targets, nearer at the higher index, at the lower)  %s  "
              "inside/reach per decade %s" % (c.name, len(c.src), len(c.tgt), cnt, dec))
    assert "other" not in c.rung
    div = 2 if c.half else 1
    if c.reach:
        n, hi, lo = cnt["reach"]
        assert n == len(c.tgt) and hi >= 8 and lo >= 8
        assert all(v >= 4 for v in dec.values()), dec
        return
    n, hi, lo = cnt["blind"]
    assert n >= 24 // div
    if c.name in ntc.FIRST_MINIMUM:
        assert hi >= 8 // div and lo >= 8 // div, cnt
    assert cnt["inside"][0] >= 24 // div
    assert all(v >= 4 // div for v in dec.values()), dec
    # the rungs as they are defined, on the measured gap
    for t, g in enumerate(c.gap):
        if c.rung[t] == "blind":
            assert ntc.FLOOR < g < ntc.HALF_ULP
        elif c.rung[t] == "inside":
            assert ntc.HALF_ULP <= g < c.ceiling[t] and g < ntc.RESOLVED
            assert 1e-7 * 0.29 < g                       # (2^-25 = 0.298e-7: the first decade starts there at the latest)
        else:
            assert c.rung[t] == "resolved" and g >= ntc.RESOLVED


def test_separated_and_the_minimum_is_a_contender(case):
    c = case
    for k in range(1, c.k + 1):
        ref.assert_separated(c.mat, k, c.distance, rel=ntc.FLOOR)
    first, _ = ref.first(c.mat, c.distance, **ref.DTW)
    gap, pair = ntc.measure_gaps(c.mat, c.distance)
    for t in range(len(c.tgt)):
        assert first[t] in c.contenders[t], (t, first[t], c.contenders[t])
        assert set(pair[t]) <= set(c.contenders[t]), (t, pair[t], c.contenders[t])     # the two smallest keys: contenders
        assert np.isfinite(c.mat[list(c.contenders[t]), t]).all()
    if c.quads:
        idx, _ = ref.topk(c.mat, 6, c.distance, **ref.DTW)
        for t in range(len(c.tgt)):
            assert sorted(idx[t, :4]) == sorted(c.contenders[t]) and len(c.contenders[t]) == 4
            assert (idx[t, 4:] >= 4 * c.n0).all()                # ranks 5 and 6: the runners-up, no family's twins
        key = ref.keys(c.mat, None, 0.0)
        for t in range(len(c.tgt)):                              # all six gaps of the four on the target's rung
            ks = sorted(key[s, t] for s in c.contenders[t])
            gaps = [(ks[j] - ks[i]) / ks[j] for i in range(4) for j in range(i + 1, 4)]
            if c.rung[t] == "blind":
                assert all(ntc.FLOOR < g < ntc.HALF_ULP for g in gaps), (t, gaps)
            else:
                assert all(ntc.HALF_ULP <= g < c.ceiling[t] for g in gaps), (t, gaps)


def test_layout_in_whole_blocks(case):
    c = case
    if c.tied:
        assert c.blocks == 1 and len(c.src) == c.n0 and c.distance is not None
        return
    assert c.distance is None and len(c.src) == (c.blocks + (2 if c.quads else 0)) * c.n0
    for t, cont in enumerate(c.contenders):
        assert len({s % c.n0 for s in cont}) == 1                 # one family
        assert len({s // c.n0 for s in cont}) == len(cont)        # one member per block: a split set has them in different shards
        assert all(s < c.blocks * c.n0 for s in cont)
    for s in range(c.n0):                                         # twins keep their original's shape
        assert all(c.src[s + b * c.n0].shape == c.src[s].shape for b in range(1, c.blocks))


def test_each_case_takes_the_route_it_is_meant_for(case):
    c = case
    n, m = len(c.src), len(c.tgt)
    fs, ft = max(a.shape[0] for a in c.src), max(a.shape[0] for a in c.tgt)
    assert not (n * m <= 8192 and fs + ft <= 128)                 # few_pairs (csrc/match.hip)
    assert all(np.isfinite(a).all() for a in c.src + c.tgt)
    assert fs <= 4096 and min(a.shape[0] for a in c.src + c.tgt) >= 1
    assert all(a.dtype == c.np_dtype and a.shape[1] == c.dim for a in c.src + c.tgt)
    wide = c.name in ("reach64", "reach100_b3", "tied64")
    assert (c.dim > ntc.FILTER_DIM) == wide
    lens = sorted({a.shape[0] for a in c.src})
    spec = ntc.SPECS[c.name]
    if spec["kind"] == "ragged":
        assert spec["lo"] <= lens[0] and lens[-1] <= spec["hi"] and len(lens) > 8
    if c.name in ("sp", "f64", "squared", "band3", "band8", "tied", "quads"):
        assert lens[0] >= 16 and lens[-1] <= 40                   # the single-pass kernel's shape
    if c.name == "mid":
        assert lens[0] >= 49 and lens[-1] <= 128
    if c.name == "long":
        assert lens == [150, 300]                                 # several row passes
    if c.name.startswith("single"):
        assert lens == [30] and c.dim == 40
    if c.dtype == "f64":                                          # values no f32 holds
        flat = np.concatenate([a.reshape(-1) for a in c.src])
        assert (flat.astype(np.float32).astype(np.float64) != flat).mean() > 0.99


def test_twins_differ_only_where_the_case_says(case):
    c = case
    if c.tied:
        return
    for s in range(c.n0):
        for b in range(1, c.blocks):
            a, tw = c.src[s], c.src[s + b * c.n0]
            if c.reach:                                           # beyond the filter's reach: values 0...41 bit for bit
                bits = np.uint32
                assert np.array_equal(np.ascontiguousarray(a[:, :ntc.FILTER_DIM]).view(bits),
                                      np.ascontiguousarray(tw[:, :ntc.FILTER_DIM]).view(bits))
                assert not np.array_equal(a[:, ntc.FILTER_DIM:], tw[:, ntc.FILTER_DIM:])
            if c.name.startswith("single"):                       # only bits below 2^-11 of each value
                assert (np.abs(tw.astype(np.float64) - a) < 2.0 ** -11 * np.abs(a)).all()
            assert not np.array_equal(a, tw)


@pytest.mark.parametrize("name", ["sp", "f64", "reach64", "tied", "quads"])
def test_the_builder_is_deterministic(oracle, name):
    one, two = ntc.build(name), ntc.build.__wrapped__(name)
    assert one is not two
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
    assert len(one.src) == len(two.src) and len(one.tgt) == len(two.tgt)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(one.src + one.tgt, two.src + two.tgt))
    assert one.contenders == two.contenders and one.rung == two.rung
    if one.distance is not None:
        assert np.array_equal(bits(one.distance), bits(two.distance))
