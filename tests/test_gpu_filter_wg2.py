"""dtw_filter_wg2_kernel (csrc/dtw_filter_wg2_kernel.hpp): the two-pass sibling of dtw_filter_wg_kernel -- a pair's two row
passes at once on two waves, the hand-off through LDS -- and its gating in csrc/dtw_filter.hip run_kernel.

Every case runs the same search three times on one context (the knobs are read per filter call): with the product's
defaults, with SSYM_FILTER_WG2=0 (dtw_filter_wg_kernel on the same plan) and with SSYM_FILTER_WG=0 (dtw_filter_kernel).
The three filter matrices have the same bits, indices and costs are the same and the oracle's, the two process-wide
launch counters (ssym_debug_filter_wg_launches, ssym_debug_filter_wg2_launches) show which kernel ran in which leg, and
launches and cells are the same in all three.  Which kernel a case must take is read off the restated plan
(tests/filter_plan.py): the new kernel serves exactly the plan's wg launches of two passes.

Shapes (all sources of 65...128 frames, so that both passes hold rows of every pair):
  small_8, small_32      8 and 32 sources x 64 targets x 128 frames x 13 values, the headline shape in small.  Record slots
                         are padded to 32 sources and the plan gives a class with padding pairs to dtw_filter_kernel, so
                         of the two only small_32 reaches the sibling (four blocks of four pairs); small_8 pins the refusal.
  dim20, dim30, squared  one-piece records in two planes, three planes, squared local costs.
  ragged_targets         five target groups whose longest members have 1, 3, 5, 127 and 130 frames: one column, a last
                         group of three columns, of one, and targets longer than the sources and no multiple of four.
  unequal_pair           a pair of a 65-frame and a 128-frame source.
  groups10_8, groups10_32  320 targets, ten target groups: XCD ranges 0 and 1 hold two groups each, a stream crosses a
                         target-group change (8 sources: refused as above).
  blocks_24, blocks_96   24 sources (refused: padding pairs) and 96 sources: twelve blocks of four pairs per target group, a
                         stream chains many tasks inside one group.
  empty_group            a target group of 32 empty targets (record slots are padded to whole groups, so a group of padding
                         only does not occur; a group without a column is this one): nCols = 0, costs +inf.
"""
import ctypes
import os

import numpy as np
import pytest

from soundsym_amd import Engine, synth
from soundsym_amd import _native
from soundsym_amd.engine import pack_segments
from filter_plan import filter_plan, plan_cells
from filter_long_cases import _other_values, _resample, _values

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12
LEGS = {"wg2": {}, "wg": {"SSYM_FILTER_WG2": "0"}, "plain": {"SSYM_FILTER_WG": "0"}}


def _counter(name):
    f = getattr(_native.lib(), name)
    f.restype, f.argtypes = ctypes.c_ulonglong, []
    return int(f())


def counters():
    return _counter("ssym_debug_filter_wg_launches"), _counter("ssym_debug_filter_wg2_launches")


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _lens(segs):
    return [a.shape[0] for a in segs]


def _make(seed, dim, src_lens, tgt_lens, planted):
    """Sources of the given lengths; the first `planted` non-empty targets are sources resampled to their length."""
    st, sig = synth.Stream(seed), synth.sigma(dim)
    src = [_values(st, f, dim, sig) for f in src_lens]
    tgt = []
    for t, f in enumerate(tgt_lens):
        if t < planted and f > 0:
            tgt.append(_resample(st, src[int(st.integers(1, len(src))[0])], int(f), dim, sig))
        else:
            tgt.append(_values(st, f, dim, sig))
    return src, tgt


def _src_lens(seed, n):
    """n source lengths in 65...128, all but three of at least 112 frames (more short ones: the SKIP0 class)."""
    st = synth.Stream(seed)
    ls = [65, 80, 100] + [int(x) for x in 112 + st.integers(n - 3, 17)]
    return [ls[int(i)] for i in st.permutation(len(ls))]


def _grid(n, m, dim, squared=False):
    g = synth.make_grid(n, m, 128, dim, 0x5EED7100 + n + m + dim)
    return dim, squared, (list(g.sources), list(g.targets))


def _ragged_targets():
    st = synth.Stream(0x5EED7200)
    lt = [1] * 32 + [2] * 10 + [3] * 22 + [4] * 20 + [5] * 12
    lt += [int(x) for x in 100 + st.integers(31, 28)] + [127] + [int(x) for x in 128 + st.integers(31, 3)] + [130]
    lt = [lt[int(i)] for i in st.permutation(len(lt))]
    return 13, False, _make(0x5EED7201, 13, _src_lens(0x5EED7202, 32), lt, 24)


def _unequal_pair():
    st = synth.Stream(0x5EED7300)
    lt = [int(x) for x in 90 + st.integers(64, 39)]
    return 13, False, _make(0x5EED7301, 13, [128] * 20 + [65] + [128] * 11, lt, 16)


def _groups10(n):
    st = synth.Stream(0x5EED7400 + n)
    lt = [int(x) for x in 1 + st.integers(320, 128)]
    ls = [128] * n if n < 32 else _src_lens(0x5EED7402, n)
    return 13, False, _make(0x5EED7401 + n, 13, ls, lt, 40)


def _blocks(n):
    st = synth.Stream(0x5EED7500 + n)
    lt = [int(x) for x in 20 + st.integers(64, 50)]
    ls = [int(x) for x in 112 + st.integers(n, 17)]
    return 13, False, _make(0x5EED7501 + n, 13, ls, lt, 16)


def _empty_group():
    st = synth.Stream(0x5EED7600)
    lt = [0] * 32 + [int(x) for x in 30 + st.integers(32, 60)]
    lt = [lt[int(i)] for i in st.permutation(len(lt))]
    return 13, False, _make(0x5EED7601, 13, _src_lens(0x5EED7602, 32), lt, 12)


CASES = {
    "small_8": lambda: _grid(8, 64, 13),
    "small_32": lambda: _grid(32, 64, 13),
    "dim20": lambda: _grid(32, 64, 20),
    "dim30": lambda: _grid(32, 64, 30),
    "squared": lambda: _grid(32, 64, 13, True),
    "ragged_targets": _ragged_targets,
    "unequal_pair": _unequal_pair,
    "groups10_8": lambda: _groups10(8),
    "groups10_32": lambda: _groups10(32),
    "blocks_24": lambda: _blocks(24),
    "blocks_96": lambda: _blocks(96),
    "empty_group": _empty_group,
}
REACHES = {"small_8": False, "groups10_8": False, "blocks_24": False}      # (every other case: the sibling runs)


def _search(e, dim, src, tgt, leg, **match_kw):
    """One filter matrix and one search in the given leg; both counters' steps for each, launches and cells."""
    os.environ.update(LEGS[leg])
    try:
        sf, so = pack_segments(src, dim, np.float32)
        tf, to = pack_segments(tgt, dim, np.float32)
        d, q = e.dictionary(sf, so, dim), e.queries(tf, to, dim)
        c0 = counters()
        filt = e.pair_matrix(d, q, exact=False)
        c1 = counters()
        idx, cost = e.match(d, q, **match_kw)
        c2 = counters()
        tm = e.timings()
        d.close()
        q.close()
    finally:
        for k in LEGS[leg]:
            del os.environ[k]
    return dict(filt=filt, idx=idx, cost=cost, matrix=(c1[0] - c0[0], c1[1] - c0[1]), match=(c2[0] - c1[0], c2[1] - c1[1]),
                cells=int(tm["n_filter_cells"]), launches=int(tm["main_launches"]),
                used_filter=int(tm["used_filter"])), (sf, so, tf, to)


def _oracle(oracle, dim, squared, packed, band=-1):
    sf, so, tf, to = packed
    return oracle.dtw_match_all(sf.astype(np.float64), so, tf.astype(np.float64), to, dim, band=band, squared=squared,
                                nthreads=16)[:2]


def _check_search(res, want_idx, want_cost):
    assert np.array_equal(res["idx"], want_idx)
    have = np.isfinite(want_cost)
    assert np.array_equal(np.isfinite(res["cost"]), have)
    assert np.allclose(res["cost"][have], want_cost[have], rtol=EXACT_RTOL, atol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_three_kernels_same_bits_and_the_oracle(oracle, name):
    dim, squared, (src, tgt) = CASES[name]()
    assert 65 <= min(_lens(src)) and max(_lens(src)) <= 128
    plan, _ = filter_plan(_lens(src), _lens(tgt), dim, num_cus())
    assert [(x.kernel, x.nt, x.passes, x.skip, x.lo) for x in plan] == [("generic", 4, 2, False, 0)], plan
    reaches = REACHES.get(name, True)
    assert plan[0].wg == reaches, plan
    e = Engine(metric="dtw", dtype="f32", squared=squared)
    try:
        _search(e, dim, *_other_values(src, tgt, dim, 0x5EED7F11), leg="wg2")      # the scratch holds another search
        res = {leg: _search(e, dim, src, tgt, leg) for leg in LEGS}
        packed = res["wg2"][1]
        res = {leg: r[0] for leg, r in res.items()}
        print("launch counters (wg, wg2) %s: %s" % (name, {leg: (r["matrix"], r["match"]) for leg, r in res.items()}))
        one = int(reaches)
        assert res["wg2"]["matrix"] == (one, one)
        assert res["wg"]["matrix"] == (one, 0)
        assert res["plain"]["matrix"] == (0, 0)
        assert res["wg2"]["match"] == (res["wg2"]["match"][0],) * 2 and res["wg2"]["match"][1] >= one
        assert res["wg"]["match"][1] == 0 and res["wg"]["match"][0] >= one
        assert res["plain"]["match"] == (0, 0)
        for leg in LEGS:
            assert res[leg]["used_filter"] == 1
            assert res[leg]["launches"] == len(plan)
            assert res[leg]["cells"] == plan_cells(plan)
        for leg in ("wg", "plain"):
            assert np.array_equal(res["wg2"]["filt"], res[leg]["filt"]), leg
            assert np.array_equal(res["wg2"]["idx"], res[leg]["idx"]), leg
            assert np.array_equal(res["wg2"]["cost"], res[leg]["cost"]), leg
        want_idx, want_cost = _oracle(oracle, dim, squared, packed)
        for leg in LEGS:
            _check_search(res[leg], want_idx, want_cost)
    finally:
        e.close()


def _refusal_data(kind):
    st = synth.Stream(0x5EED7D00)
    if kind == "three_passes":
        ls = [150] * 32
    elif kind == "one_pass":
        ls = [int(x) for x in 49 + st.integers(32, 16)]             # 49...64 frames
    elif kind == "odd_blocks":
        ls = [int(x) for x in 112 + st.integers(30, 17)]            # fifteen pairs
    else:
        ls = [int(x) for x in 112 + st.integers(32, 17)]
    lt = [int(x) for x in 100 + st.integers(40, 29)] if kind == "band" else [int(x) for x in 1 + st.integers(40, 60)]
    return _make(0x5EED7D01 + len(kind), 13, ls, lt, 8)


@pytest.mark.parametrize("kind", ["three_passes", "one_pass", "band", "prune", "odd_blocks"])
def test_refusals_keep_the_other_kernels(oracle, kind):
    src, tgt = _refusal_data(kind)
    band = 24 if kind == "band" else -1
    e = Engine(metric="dtw", dtype="f32", band=band)
    try:
        res, packed = _search(e, 13, src, tgt, "wg2", **(dict(prune=True) if kind == "prune" else {}))
        assert res["used_filter"] == 1
        if kind == "prune":                               # the unpruned filter matrix may take the sibling, the pruned search not
            assert res["match"] == (0, 0)
        else:
            assert res["matrix"][1] == 0 and res["match"][1] == 0
            if kind in ("three_passes", "one_pass"):      # one launch of four-tile passes, but not two of them
                plan, _ = filter_plan(_lens(src), _lens(tgt), 13, num_cus())
                assert [(x.nt, x.passes) for x in plan] == [(4, 3 if kind == "three_passes" else 1)], plan
        want_idx, want_cost = _oracle(oracle, 13, False, packed, band=band)
        _check_search(res, want_idx, want_cost)
    finally:
        e.close()


def test_twice_on_one_context_and_after_another_kernel_same_bits():
    dim, _, (src, tgt) = _ragged_targets()
    dim_c, _, (src_c, tgt_c) = _grid(32, 64, 13)
    e = Engine(metric="dtw", dtype="f32")
    try:
        first, _ = _search(e, dim, src, tgt, "wg2")
        again, _ = _search(e, dim, src, tgt, "wg2")
        between, _ = _search(e, dim_c, src_c, tgt_c[:40], "plain")          # a search that takes another kernel
        third, _ = _search(e, dim, src, tgt, "wg2")
        assert first["matrix"] == again["matrix"] == third["matrix"] == (1, 1) and between["matrix"] == (0, 0)
        for k in ("filt", "idx", "cost"):
            assert np.array_equal(first[k], again[k]), k
            assert np.array_equal(first[k], third[k]), k
    finally:
        e.close()
