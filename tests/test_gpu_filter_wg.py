"""dtw_filter_wg_kernel (csrc/dtw_filter_wg_kernel.hpp): the sibling of the headline filter kernel whose four waves share
one ring of target columns, and its gating in csrc/dtw_filter_plan.hpp plan_filter.

Every case runs the same search with SSYM_FILTER_WG=1 and =0 (read per launch) on one context: the filter matrix of both
legs has the same bits, the sibling's is within tests/bounds.py's per-pair bound of the oracle after the scratch has been
filled by another search of the same lengths (a task never run would show), argmin and cost of every target are the
oracle's, the process-wide launch counter (ssym_debug_filter_wg_launches) proves which kernel ran in which leg, and the
timings' launch and cell counts are the same in both.

Shapes: the smallest that reach each thing that can go wrong.
  a  32 sources of 65...128 frames x 40 targets of 1...57, dim 13: two passes, at most one block of four pairs per XCD
     range, two target groups (six XCD ranges empty), one of them of 1-frame targets only (one column: the ring's minimum
     of one column group), the other's 57 columns no multiple of four.  All but three sources have at least 112 frames:
     with more short ones the class would run the SKIP0 instantiation (launch_dtw_filter), which the sibling does not serve.
  b  64 sources of 129...192 frames x 300 targets, dim 30: three passes (a middle pass: hand-off read AND written), three
     operand planes, ten target groups: XCD ranges of unequal length and helping across `hop`.
  c  128 x 128 segments of 128 frames, dim 13, plain and squared: the headline's code path in small.
  d  refusals -- a first pair whose first pass is not 0 (its members have 50 and 60 frames: pass 0 of the class holds none
     of their rows), 30 sources (a padding pair), a band, prune=True: the counter stays where it was, results are the oracle's.
  e  the sibling's search twice on one context with a search of another shape between: identical bits.
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
from filter_long_cases import _other_values, _resample, _values

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12


def wg_launches():
    f = _native.lib().ssym_debug_filter_wg_launches
    f.restype, f.argtypes = ctypes.c_ulonglong, []
    return int(f())


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _lens(segs):
    return [a.shape[0] for a in segs]


def _make(seed, dim, src_lens, tgt_lens, planted):
    """Sources of the given lengths; the first `planted` targets are sources resampled to their length, the rest noise."""
    st, sig = synth.Stream(seed), synth.sigma(dim)
    src = [_values(st, f, dim, sig) for f in src_lens]
    tgt = []
    for t, f in enumerate(tgt_lens):
        if t < planted:
            tgt.append(_resample(st, src[int(st.integers(1, len(src))[0])], int(f), dim, sig))
        else:
            tgt.append(_values(st, f, dim, sig))
    return src, tgt


def case_a():
    st = synth.Stream(0x5EED6A00)
    ls = [65, 80, 100] + [int(x) for x in 112 + st.integers(29, 17)]
    lt = [57, 33, 60 - 4, 41, 2, 19, 50, 7] + [1] * 32
    ls = [ls[int(i)] for i in st.permutation(len(ls))]
    return 13, False, _make(0x5EED6A01, 13, ls, lt, 8)


def case_b():
    st = synth.Stream(0x5EED6B00)
    ls = [129, 140, 150, 160] + [int(x) for x in 176 + st.integers(60, 17)]
    lt = [int(x) for x in 1 + st.integers(300, 80)]
    ls = [ls[int(i)] for i in st.permutation(len(ls))]
    return 30, False, _make(0x5EED6B01, 30, ls, lt, 40)


def case_c(squared):
    g = synth.make_grid(128, 128, 128, 13, 0x5EED6C00)
    return 13, squared, (list(g.sources), list(g.targets))


CASES = {"a": case_a, "b": case_b, "c": lambda: case_c(False), "c_squared": lambda: case_c(True)}


def _search(e, dim, src, tgt, wg, **match_kw):
    """One filter matrix and one search with SSYM_FILTER_WG=wg; the sibling's launches of each, launches and cells."""
    os.environ["SSYM_FILTER_WG"] = "1" if wg else "0"
    try:
        sf, so = pack_segments(src, dim, np.float32)
        tf, to = pack_segments(tgt, dim, np.float32)
        d, q = e.dictionary(sf, so, dim), e.queries(tf, to, dim)
        c0 = wg_launches()
        filt = e.pair_matrix(d, q, exact=False)
        c1 = wg_launches()
        idx, cost = e.match(d, q, **match_kw)
        c2 = wg_launches()
        tm = e.timings()
        d.close()
        q.close()
    finally:
        del os.environ["SSYM_FILTER_WG"]
    return dict(filt=filt, idx=idx, cost=cost, wg_matrix=c1 - c0, wg_match=c2 - c1, cells=int(tm["n_filter_cells"]),
                launches=int(tm["main_launches"]), used_filter=int(tm["used_filter"])), (sf, so, tf, to)


def _oracle(oracle, dim, squared, packed, band=-1):
    sf, so, tf, to = packed
    return oracle.dtw_match_all(sf.astype(np.float64), so, tf.astype(np.float64), to, dim, band=band, squared=squared,
                                want_matrix=True, nthreads=16)


def _check_search(res, want_idx, want_cost):
    assert np.array_equal(res["idx"], want_idx)
    have = np.isfinite(want_cost)
    assert np.array_equal(np.isfinite(res["cost"]), have)
    assert np.allclose(res["cost"][have], want_cost[have], rtol=EXACT_RTOL, atol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_sibling_against_plain_kernel_and_oracle(oracle, name):
    dim, squared, (src, tgt) = CASES[name]()
    plan, _ = filter_plan(_lens(src), _lens(tgt), dim, num_cus())
    # one launch, of the class the sibling serves: four tiles, several passes, no skipped first tiles
    assert [(x.kernel, x.nt, x.skip, x.lo) for x in plan] == [("generic", 4, False, 0)], plan
    assert plan[0].passes == {"a": 2, "b": 3}.get(name, 2)
    e = Engine(metric="dtw", dtype="f32", squared=squared)
    try:
        _search(e, dim, *_other_values(src, tgt, dim, 0x5EED6F11), wg=True)      # the scratch holds another search
        on, packed = _search(e, dim, src, tgt, wg=True)
        off, _ = _search(e, dim, src, tgt, wg=False)
        assert (on["wg_matrix"], off["wg_matrix"]) == (1, 0), (on["wg_matrix"], off["wg_matrix"])
        plan_off, _ = filter_plan(_lens(src), _lens(tgt), dim, num_cus(), wg=False)      # the plan's gate says the same
        assert ([x.wg for x in plan], [x.wg for x in plan_off]) == ([True], [False])
        assert [x._replace(wg=False) for x in plan] == plan_off
        assert on["wg_match"] >= 1 and off["wg_match"] == 0
        assert on["used_filter"] == off["used_filter"] == 1
        assert on["launches"] == off["launches"] == len(plan)
        assert on["cells"] == off["cells"] == plan_cells(plan)
        assert np.array_equal(on["filt"], off["filt"])
        assert np.array_equal(on["idx"], off["idx"]) and np.array_equal(on["cost"], off["cost"])

        want_idx, want_cost, mat = _oracle(oracle, dim, squared, packed)
        assert np.isfinite(mat).all() and np.isfinite(on["filt"]).all()
        if not squared:                                   # (squared costs have no restated bound)
            pb = pair_bound_matrix(src, tgt, min(dim, 42))[0]
            err, tol = np.abs(on["filt"] - mat), pb + 1e-5 * mat
            print("filter err/tol %s: %.4f" % (name, float((err / tol).max())))
            assert (err <= tol).all(), (int((err > tol).sum()), float((err / tol).max()))
        _check_search(on, want_idx, want_cost)
    finally:
        e.close()


def _refusal_data(kind):
    st = synth.Stream(0x5EED6D00)
    long29 = [int(x) for x in 112 + st.integers(30, 17)]
    if kind == "first_pass":
        ls = [50, 60] + long29
    elif kind == "padding_pair":
        ls = long29
    else:
        ls = long29 + [112, 128]
    lt = [int(x) for x in 100 + st.integers(40, 29)] if kind == "band" else [int(x) for x in 1 + st.integers(40, 60)]
    return _make(0x5EED6D01 + len(kind), 13, ls, lt, 8)


@pytest.mark.parametrize("kind", ["first_pass", "padding_pair", "band", "prune"])
def test_refusals_keep_the_plain_kernels(oracle, kind):
    src, tgt = _refusal_data(kind)
    assert len(src) == (30 if kind == "padding_pair" else 32)
    band = 24 if kind == "band" else -1
    e = Engine(metric="dtw", dtype="f32", band=band)
    try:
        res, packed = _search(e, 13, src, tgt, wg=True, **(dict(prune=True) if kind == "prune" else {}))
        assert res["used_filter"] == 1
        if kind == "prune":                               # the unpruned filter matrix may take the sibling, the pruned search not
            assert res["wg_match"] == 0
        else:
            assert (res["wg_matrix"], res["wg_match"]) == (0, 0)
            if band < 0:                                  # the plan's gate says the same
                plan, _ = filter_plan(_lens(src), _lens(tgt), 13, num_cus())
                assert len(plan) == 1 and sum(x.wg for x in plan) == res["wg_matrix"], plan
        want_idx, want_cost, _ = _oracle(oracle, 13, False, packed, band=band)
        _check_search(res, want_idx, want_cost)
    finally:
        e.close()


def test_sibling_twice_on_one_context_same_bits():
    dim, _, (src, tgt) = case_a()
    dim_c, _, (src_c, tgt_c) = case_c(False)
    e = Engine(metric="dtw", dtype="f32")
    try:
        first, _ = _search(e, dim, src, tgt, wg=True)
        between, _ = _search(e, dim_c, src_c[:64], tgt_c[:40], wg=True)
        again, _ = _search(e, dim, src, tgt, wg=True)
        assert first["wg_matrix"] == between["wg_matrix"] == again["wg_matrix"] == 1
        for k in ("filt", "idx", "cost"):
            assert np.array_equal(first[k], again[k]), k
    finally:
        e.close()
