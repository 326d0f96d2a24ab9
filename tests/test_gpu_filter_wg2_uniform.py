"""dtw_filter_wg2_kernel<SQ, KU, UNIFORM = true> (csrc/dtw_filter_wg2_kernel.hpp): the instantiation of the two-pass kernel
for launches whose lengths do not differ, and its gate in csrc/dtw_filter.hip run_kernel.

Every positive case runs the same search twice on one context (the knobs are read per filter call), with the product's
defaults and with SSYM_FILTER_WG2U=0 (the general kernel on the same plan), after a search of OTHER lengths and values
has dirtied the context's scratch.  The two filter matrices have the same bits, as have indices and costs; the matrix is
within tests/bounds.py's per-pair bound of the oracle's, indices and costs are the oracle's; the process-wide launch
counters (ssym_debug_filter_wg2_launches, ssym_debug_filter_wg2u_launches) show which instantiation ran in which leg;
launches and cells are the restated plan's (tests/filter_plan.py) in both.

The gate sits behind the plan's: the plan gives a launch to the two-pass kernels only when its pairs come in whole blocks
of four without a padding pair, and record slots are padded to 32 sources -- so a set reaches them with a multiple of 32
sources.  The cases that must take the new instantiation therefore have 32, 96 or 4160 sources; the same shapes at 8 and 40
sources (tiny_8, sources_40) are kept as cases the PLAN refuses: counter 0, same bits.  Uniform sources of 65...111 frames
get three-tile passes or the SKIP0 kernel from the default plan; SSYM_FILTER_LONG_CLASSES=0 (the set's own shape, four
tiles, no skip) brings them to the two-pass kernel, in both legs.

  tiny, tiny_8        32 / 8 sources of 128 frames x 32 targets of 4 frames: one group per task, every tick a task boundary,
                      the two records alternate every tick.
  f8, f12, f128, f132 target lengths; 132 is past one turn of the ring within a task.
  groups10            320 targets: ten groups on eight XCD ranges, ranges 0 and 1 hold two groups, six are spent early.
  sources_96, _40     twelve blocks of four pairs per target group: a workgroup chains tasks; 40: refused by the plan.
  blocks_1040         4160 sources x 32 targets of 4 frames: 1040 blocks for the 512 workgroups of a 256-CU grid, all in
                      the one XCD range that holds a target group -- seven ranges are spent at once and every workgroup
                      chains tasks of one tick each.
  fa120, fa100, fa65  shorter sources: the leader's general set-up with the follower's fast column 0 (fa65: one real row
                      in the leader's pass).
  dim13 (the others), dim20, dim30, squared   two operand planes in two record layouts, three planes, squared local costs.
"""
import ctypes
import os

import numpy as np
import pytest

from soundsym_amd import Engine, synth
from soundsym_amd import _native
from soundsym_amd.engine import pack_segments
from bounds import pair_bound_matrix
from filter_plan import filter_plan, plan_cells
from filter_long_cases import _resample, _values

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12
LEGS = {"uniform": {}, "general": {"SSYM_FILTER_WG2U": "0"}}
OWN_SHAPE = {"SSYM_FILTER_LONG_CLASSES": "0"}


def _counter(name):
    f = getattr(_native.lib(), name)
    f.restype, f.argtypes = ctypes.c_ulonglong, []
    return int(f())


def counters():
    return _counter("ssym_debug_filter_wg2_launches"), _counter("ssym_debug_filter_wg2u_launches")


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _lens(segs):
    return [a.shape[0] for a in segs]


def _make(seed, dim, src_lens, tgt_lens, planted):
    """Sources of the given lengths; the first `planted` targets are sources resampled to their length."""
    st, sig = synth.Stream(seed), synth.sigma(dim)
    src = [_values(st, f, dim, sig) for f in src_lens]
    tgt = []
    for t, f in enumerate(tgt_lens):
        if t < planted:
            tgt.append(_resample(st, src[int(st.integers(1, len(src))[0])], int(f), dim, sig))
        else:
            tgt.append(_values(st, f, dim, sig))
    return src, tgt


# name: (sources, their frames, targets, their frames, values, squared, knobs of both legs, reaches the instantiation)
CASES = {
    "tiny": (32, 128, 32, 4, 13, False, {}, True),
    "tiny_8": (8, 128, 32, 4, 13, False, {}, False),
    "f8": (32, 128, 64, 8, 13, False, {}, True),
    "f12": (32, 128, 64, 12, 13, False, {}, True),
    "f128": (32, 128, 64, 128, 13, False, {}, True),
    "f132": (32, 128, 64, 132, 13, False, {}, True),
    "groups10": (32, 128, 320, 20, 13, False, {}, True),
    "sources_96": (96, 128, 64, 16, 13, False, {}, True),
    "sources_40": (40, 128, 64, 16, 13, False, {}, False),
    "blocks_1040": (4160, 128, 32, 4, 13, False, {}, True),
    "fa120": (32, 120, 64, 24, 13, False, {}, True),
    "fa100": (32, 100, 64, 24, 13, False, OWN_SHAPE, True),
    "fa65": (32, 65, 64, 24, 13, False, OWN_SHAPE, True),
    "dim20": (32, 128, 64, 16, 20, False, {}, True),
    "dim30": (32, 128, 64, 16, 30, False, {}, True),
    "squared": (32, 128, 64, 16, 13, True, {}, True),
}


def _case(name):
    n, fa, m, fb, dim, squared, knobs, reaches = CASES[name]
    k = list(CASES).index(name)
    return dim, squared, knobs, reaches, _make(0x5EED8100 + k, dim, [fa] * n, [fb] * m, min(m, 24))


def _dirt(seed, dim):
    """A search of other lengths and values, for the same context: ragged sources of 70...128 frames, ragged targets."""
    st = synth.Stream(seed)
    return _make(seed + 1, dim, [int(x) for x in 70 + st.integers(32, 59)], [int(x) for x in 1 + st.integers(40, 150)], 0)


def _search(e, dim, src, tgt, knobs, **match_kw):
    """One filter matrix and one search under the given knobs; both counters' steps for each, launches and cells."""
    os.environ.update(knobs)
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
        for k in knobs:
            del os.environ[k]
    return dict(filt=filt, idx=idx, cost=cost, matrix=(c1[0] - c0[0], c1[1] - c0[1]), match=(c2[0] - c1[0], c2[1] - c1[1]),
                cells=int(tm["n_filter_cells"]), launches=int(tm["main_launches"]),
                used_filter=int(tm["used_filter"])), (sf, so, tf, to)


def _oracle(oracle, dim, squared, packed, band=-1):
    sf, so, tf, to = packed
    return oracle.dtw_match_all(sf.astype(np.float64), so, tf.astype(np.float64), to, dim, band=band, squared=squared,
                                want_matrix=True, nthreads=16)


def _check_search(res, want_idx, want_cost):
    assert np.array_equal(res["idx"], want_idx)
    have = np.isfinite(want_cost)
    assert np.array_equal(np.isfinite(res["cost"]), have)
    assert np.allclose(res["cost"][have], want_cost[have], rtol=EXACT_RTOL, atol=0)


def _same_bits(a, b):
    for k in ("filt", "idx", "cost"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", list(CASES))
def test_uniform_and_general_same_bits_and_the_oracle(oracle, name):
    dim, squared, knobs, reaches, (src, tgt) = _case(name)
    plan, _ = filter_plan(_lens(src), _lens(tgt), dim, num_cus(), long_classes=not knobs)
    assert [(x.kernel, x.nt, x.passes, x.skip, x.lo) for x in plan] == [("generic", 4, 2, False, 0)], plan
    assert plan[0].wg == reaches, plan
    e = Engine(metric="dtw", dtype="f32", squared=squared)
    try:
        _search(e, dim, *_dirt(0x5EED8F00 + dim, dim), knobs={})            # the scratch holds another search
        res = {leg: _search(e, dim, src, tgt, dict(knobs, **LEGS[leg])) for leg in LEGS}
        packed = res["uniform"][1]
        res = {leg: r[0] for leg, r in res.items()}
        print("launch counters (wg2, wg2u) %s: %s" % (name, {leg: (r["matrix"], r["match"]) for leg, r in res.items()}))
        one = int(reaches)
        assert res["uniform"]["matrix"] == (one, one)
        assert res["general"]["matrix"] == (one, 0)
        assert res["uniform"]["match"] == (res["uniform"]["match"][0],) * 2 and res["uniform"]["match"][1] >= one
        assert res["general"]["match"][1] == 0 and res["general"]["match"][0] >= one
        for leg in LEGS:
            assert res[leg]["used_filter"] == 1
            assert res[leg]["launches"] == len(plan)
            assert res[leg]["cells"] == plan_cells(plan)
        _same_bits(res["uniform"], res["general"])
        want_idx, want_cost, mat = _oracle(oracle, dim, squared, packed)
        assert np.isfinite(mat).all() and np.isfinite(res["uniform"]["filt"]).all()
        if not squared:                                   # (squared costs have no restated bound)
            pb = pair_bound_matrix(src, tgt, min(dim, 42))[0]
            err, tol = np.abs(res["uniform"]["filt"] - mat), pb + 1e-5 * mat
            print("filter err/tol %s: %.4f" % (name, float((err / tol).max())))
            assert (err <= tol).all(), (int((err > tol).sum()), float((err / tol).max()))
        for leg in LEGS:
            _check_search(res[leg], want_idx, want_cost)
    finally:
        e.close()


def _refusal_lens(kind):
    ls, lt = [128] * 32, [16] * 64
    if kind == "short_target":
        lt[37] = 15
    elif kind == "f6":
        lt = [6] * 64
    elif kind == "m40":
        lt = [16] * 40
    elif kind == "source_127":
        ls[11] = 127
    elif kind == "odd_sources":
        ls = [128] * 31
    elif kind == "band":
        lt = [120] * 64
    return ls, lt


@pytest.mark.parametrize("kind", ["short_target", "f6", "m40", "source_127", "odd_sources", "prune", "band"])
def test_refusals_keep_the_general_kernel(oracle, kind):
    ls, lt = _refusal_lens(kind)
    src, tgt = _make(0x5EED8D00 + len(kind), 13, ls, lt, 8)
    band = 24 if kind == "band" else -1
    kw = dict(prune=True) if kind == "prune" else {}
    e = Engine(metric="dtw", dtype="f32", band=band)
    try:
        res, packed = _search(e, 13, src, tgt, LEGS["uniform"], **kw)
        off, _ = _search(e, 13, src, tgt, LEGS["general"], **kw)
        print("launch counters (wg2, wg2u) %s: %s %s" % (kind, res["matrix"], res["match"]))
        assert res["used_filter"] == 1
        assert res["match"][1] == 0
        if kind != "prune":                               # (the unpruned filter matrix of the prune case is a uniform call)
            assert res["matrix"][1] == 0
            assert res["matrix"] == off["matrix"] and res["match"] == off["match"]
        if kind in ("short_target", "f6", "m40", "source_127"):         # the general two-pass kernel ran
            assert res["matrix"][0] == 1 and res["match"][0] >= 1
        _same_bits(res, off)
        want_idx, want_cost, _ = _oracle(oracle, 13, False, packed, band=band)
        _check_search(res, want_idx, want_cost)
    finally:
        e.close()
