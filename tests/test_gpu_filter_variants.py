"""Every launch variant of the dtw MFMA filter (csrc/dtw_filter_plan.hpp plan_filter, csrc/dtw_filter.hip run_launch), pair by pair against the oracle.

The selection drops a pair whose filter cost, minus its bound (csrc/dtw_margin.hpp), cannot win, and the exact f64
re-score only sees the survivors: a filter value outside its bound, or a (target group, source pair) task the scheduler
never runs -- the cost matrix is reused scratch, such a pair keeps the previous call's value -- changes an answer with
no error reported.  Each case below is shaped so that its launches take one particular variant of the short-source
kernels (dtw_filter_sp_kernel.hpp: multi-pair tasks with KU = 2 or 3 operand planes, single-pair tasks of one to three
tiles, several pair blocks, few target groups) or the generic kernel beside them, and the launch plan is restated
(tests/filter_plan.py) from the segment lengths, the dim and the device's CU count: the timings' launch and cell counts
prove that the case ran the variant it names and that the A/B comparisons below compare two different kernels.

Per case: the whole filter matrix within the per-pair bound of tests/bounds.py after the scratch has been filled with
another search of the same shape, the exact matrix and the argmin of every target against the oracle, and the same bits
with the knobs that pick another variant (SSYM_SP_MULTIPAIR=0 in process; SSYM_FILTER_SP=0 and SSYM_SP_PAIRBLOCK=0 in a
child process each).
"""
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

from soundsym_amd import Engine, synth
from soundsym_amd.engine import pack_segments
from bounds import pair_bound_matrix
from filter_plan import Launch, _cells, filter_ku, filter_plan, plan_cells      # noqa: F401 (the launch plan, restated)

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the cases -------------------------------------------------------------------------------------------------------
# n x m segments, source lengths lo...hi, targets 1...60 frames (half of them planted near-copies of sources), and the
# plan each must run: the kernel per class, KU, pair blocks per class (None: not asserted), target groups.  (seed: a draw
# whose multi-pair tasks straddle a row-block edge, so that one pair per wave sweeps fewer cells -- the A/B's witness)
Case = namedtuple("Case", "name n m lo hi dim squared empty_tgt kernels ku blocks groups topk seed", defaults=(0,))
CASES = [
    # 512 pairs (= 2 mod 3: the last task holds two), n_pad 1024: set.len of 4 KB, the multi-pair prefetch's over-read
    Case("mp_ku2_two_blocks", 1024, 512, 1, 16, 13, False, 0, ("mp",), 2, (2,), 16, True),
    # empty sources and targets, 1024 pairs (= 1 mod 3), 12 target groups (not a multiple of 8)
    Case("mp_ku2_empty_segments", 2048, 360, 0, 16, 12, False, 9, ("mp",), 2, None, 12, False),
    Case("mp_ku3", 1500, 512, 1, 16, 27, False, 0, ("mp",), 3, (3,), 16, True, 1),
    Case("mp_ku3_8_groups", 4096, 256, 1, 16, 40, False, 0, ("mp",), 3, None, 8, False),
    # 2 target groups: six of the eight XCD ranges are empty
    Case("nt1_single_pair_two_blocks", 1024, 64, 1, 16, 13, False, 0, ("sp",), 2, (2,), 2, False),
    # squared costs, record layout 1 in two planes
    Case("mp_squared", 1024, 512, 1, 16, 20, True, 0, ("mp",), 2, None, 16, False),
    Case("nt1_nt2", 1024, 256, 1, 32, 13, False, 0, ("sp", "sp"), 2, (None, 2), 8, False),
    Case("nt1_nt2_ku3_7_groups", 700, 200, 1, 32, 30, False, 0, ("sp", "sp"), 3, None, 7, False),
    Case("nt1_nt2_nt3", 1024, 256, 1, 48, 13, False, 0, ("sp", "sp", "sp"), 2, None, 8, False),
    # three tiles with three planes: the generic dtw_filter_kernel beside the sp classes
    Case("nt3_ku3_generic", 1024, 256, 1, 48, 40, False, 0, ("sp", "sp", "generic"), 3, None, 8, False),
    # the reference's shape: a multi-pair one-tile class that ends inside the pair array, then two and three tiles
    Case("mixed_5_40", 4096, 1024, 5, 40, 30, False, 0, ("mp", "sp", "generic"), 3, None, 32, True, 1),
]
MP_CASES = [c.name for c in CASES if "mp" in c.kernels]


def case_data(case, values_seed=0):
    """(src, tgt) lists of [frames, dim] float32.  values_seed != 0: the same lengths, other values at the same amplitude
    (the scratch-filling search of the stale-task check)."""
    k = [c.name for c in CASES].index(case.name)
    st = synth.Stream(0x5EEDF100 + 16 * k + case.seed)
    sig = synth.sigma(case.dim)
    ls = case.lo + st.integers(case.n, case.hi - case.lo + 1)
    src = [(st.normal(int(f) * case.dim).reshape(int(f), case.dim) * sig).astype(np.float32) for f in ls]
    for _ in range(8):                                   # duplicates: the first index wins a tie
        i, j = (int(x) for x in st.integers(2, case.n))
        if i != j:
            src[max(i, j)] = src[min(i, j)].copy()
    n_pl = case.m // 2
    tgt = []
    for t, p in enumerate(st.integers(n_pl, case.n)):    # planted: a source resampled to within two frames, + noise
        p = int(p)
        while src[p].shape[0] == 0:
            p = (p + 1) % case.n
        a = src[p]
        f = int(np.clip(a.shape[0] + t % 5 - 2, 1, 60))
        rows = np.rint(np.linspace(0.0, a.shape[0] - 1.0, f)).astype(np.int64)
        tgt.append((a[rows].astype(np.float64) + st.normal(f * case.dim).reshape(f, case.dim) * (0.05 * sig)).astype(np.float32))
    lt = 1 + st.integers(case.m - n_pl, 60)
    lt[:min(33, lt.size // 2)] = 1                       # a group of 1-frame targets: the ring's minimum of 4 columns
    lt[lt.size - case.empty_tgt:] = 0
    tgt += [(st.normal(int(f) * case.dim).reshape(int(f), case.dim) * sig).astype(np.float32) for f in lt]
    tgt = [tgt[int(i)] for i in st.permutation(case.m)]
    if values_seed:
        st2 = synth.Stream(values_seed)
        src = [(st2.normal(a.size).reshape(a.shape) * sig).astype(np.float32) for a in src]
        tgt = [(st2.normal(a.size).reshape(a.shape) * sig).astype(np.float32) for a in tgt]
    return src, tgt


def run_case(e, case, src, tgt):
    """Filter matrix, argmin and the launch counters of one case on Engine e."""
    sf, so = pack_segments(src, case.dim, np.float32)
    tf, to = pack_segments(tgt, case.dim, np.float32)
    d, q = e.dictionary(sf, so, case.dim), e.queries(tf, to, case.dim)
    filt = e.pair_matrix(d, q, exact=False)
    idx, cost = e.match(d, q)
    tm = e.timings()
    out = dict(filt=filt, idx=idx, cost=cost, cells=int(tm["n_filter_cells"]), launches=int(tm["main_launches"]),
               used_filter=int(tm["used_filter"]))
    return out, (d, q, sf, so, tf, to)


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _lens(segs):
    return [a.shape[0] for a in segs]


def _check_plan(case, src, tgt, ncu):
    """The intended variant: kernels per class, KU, pair blocks and target groups as the case names them."""
    plan, groups = filter_plan(_lens(src), _lens(tgt), case.dim, ncu)
    assert tuple(x.kernel for x in plan) == case.kernels, plan
    assert filter_ku(case.dim) == case.ku and groups == case.groups, (case.dim, groups)
    if case.blocks is not None:
        for x, b in zip(plan, case.blocks):
            assert b is None or x.blocks == b, plan
    return plan


# ---- per case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_filter_variant_against_oracle(oracle, case):
    src, tgt = case_data(case)
    ncu = num_cus()
    plan = _check_plan(case, src, tgt, ncu)
    e = Engine(metric="dtw", dtype="f32", squared=case.squared)
    try:
        # stale-task check: the scratch cost matrix first holds another search of the same shape
        fill_src, fill_tgt = case_data(case, values_seed=0x5EEDF0FF)
        fill, hs = run_case(e, case, fill_src, fill_tgt)
        for h in hs[:2]:
            h.close()
        res, (d, q, sf, so, tf, to) = run_case(e, case, src, tgt)
        filt, idx, cost = res["filt"], res["idx"], res["cost"]
        # the launches ran the restated plan, whose cells differ from those of the variant each knob would pick instead
        assert res["used_filter"] == 1 and res["launches"] == len(plan), (res["launches"], plan)
        assert res["cells"] == plan_cells(plan), (res["cells"], plan_cells(plan), plan)
        alt, _ = filter_plan(_lens(src), _lens(tgt), case.dim, ncu, mp=False) if "mp" in case.kernels else \
            filter_plan(_lens(src), _lens(tgt), case.dim, ncu, sp=False)
        assert plan_cells(alt) != plan_cells(plan)
        assert fill["cells"] == res["cells"]

        want_idx, want_cost, mat = oracle.dtw_match_all(sf.astype(np.float64), so, tf.astype(np.float64), to, case.dim,
                                                        squared=case.squared, want_matrix=True, nthreads=16)
        fin = np.isfinite(mat)
        # pairs with an empty segment: the oracle's +inf, and the filter's (no frame: every DP cell stays +inf)
        assert np.array_equal(fin, np.array([[a.shape[0] > 0] for a in src]) & np.array([[b.shape[0] > 0 for b in tgt]]))
        assert np.isposinf(filt[~fin]).all()
        assert np.isfinite(filt[fin]).all()
        if not case.squared:                              # (squared costs have no restated bound)
            pb = pair_bound_matrix(src, tgt, min(case.dim, 42))[0]
            err, tol = np.abs(filt[fin] - mat[fin]), (pb + 1e-5 * mat)[fin]
            assert (err <= tol).all(), (int((err > tol).sum()), float((err / tol).max()))
        exact = e.pair_matrix(d, q, exact=True)
        assert np.array_equal(np.isfinite(exact), fin)
        assert np.allclose(exact[fin], mat[fin], rtol=EXACT_RTOL, atol=0)

        # the search: the oracle's argmin (first index on ties) for every target
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(np.isfinite(cost), np.isfinite(want_cost))
        have = np.isfinite(want_cost)
        assert np.allclose(cost[have], want_cost[have], rtol=EXACT_RTOL, atol=0)
        if case.topk:
            top, tcost = e.match_topk(d, q, 4)
            want_top, _ = oracle.topk(mat, 4, default_distance=0.0, fold_start=float("inf"))
            assert np.array_equal(top.astype(np.int64), want_top)
            assert np.allclose(tcost, mat[want_top, np.arange(len(tgt))[:, None]], rtol=EXACT_RTOL, atol=0)
            dist = np.median(np.where(fin, mat, np.nan), axis=0) * (0.5 + synth.Stream(7).uniform24(len(tgt)))
            di, dc = e.match(d, q, distance=dist)
            key = np.abs(mat - dist[None, :])
            wi = key.argmin(axis=0)
            assert np.array_equal(di, wi)
            assert np.allclose(dc, mat[wi, np.arange(len(tgt))], rtol=EXACT_RTOL, atol=0)

        # SSYM_SP_MULTIPAIR=0 (read per launch): one pair per wave, the same bits
        if case.name in MP_CASES:
            os.environ["SSYM_SP_MULTIPAIR"] = "0"
            try:
                single, _ = run_case(e, case, src, tgt)
            finally:
                del os.environ["SSYM_SP_MULTIPAIR"]
            assert single["cells"] == plan_cells(alt) != res["cells"]
            assert np.array_equal(single["filt"], filt)
            assert np.array_equal(single["idx"], idx) and np.array_equal(single["cost"], cost)
    finally:
        e.close()


# ---- the whole table under a knob: a child process each ---------------------------------------------------------------
_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_filter_variants as T
from soundsym_amd import Engine
out = {}
for c in T.CASES:
    e = Engine(metric="dtw", dtype="f32", squared=c.squared)
    src, tgt = T.case_data(c)
    r, _ = T.run_case(e, c, src, tgt)
    for k, v in r.items():
        out[c.name + "/" + k] = np.asarray(v)
    e.close()
np.savez(sys.argv[3], **out)
"""


def _run_table_in_process():
    out = {}
    for c in CASES:
        e = Engine(metric="dtw", dtype="f32", squared=c.squared)
        try:
            src, tgt = case_data(c)
            out[c.name], _ = run_case(e, c, src, tgt)
        finally:
            e.close()
    return out


def test_filter_sp_and_pair_block_knobs_same_bits(tmp_path):
    """SSYM_FILTER_SP=0 (every class on dtw_filter_kernel) and SSYM_SP_PAIRBLOCK=0 (one block: another task order) give
    the default's filter matrices and search results bit for bit, case by case."""
    ncu = num_cus()
    base = _run_table_in_process()
    for knob in ("SSYM_FILTER_SP", "SSYM_SP_PAIRBLOCK"):
        path = str(tmp_path / (knob + ".npz"))
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, HERE, path], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, **{knob: "0"}))
        assert r.returncode == 0, (knob, r.stderr[-3000:])
        got = np.load(path)
        blocks = 0
        for c in CASES:
            b = base[c.name]
            src, tgt = case_data(c)
            plan, _ = filter_plan(_lens(src), _lens(tgt), c.dim, ncu)
            other, _ = filter_plan(_lens(src), _lens(tgt), c.dim, ncu, sp=knob != "SSYM_FILTER_SP",
                                   pair_blocks=knob != "SSYM_SP_PAIRBLOCK")
            cells = int(got[c.name + "/cells"])
            assert b["cells"] == plan_cells(plan) and cells == plan_cells(other), (knob, c.name)
            if knob == "SSYM_FILTER_SP":                 # other kernels: their cells differ
                assert cells != b["cells"], c.name
            else:                                        # the same kernels in another order: the plan shows the blocks
                blocks += any(x.blocks >= 2 for x in plan)
            assert int(got[c.name + "/launches"]) == b["launches"], (knob, c.name)
            assert np.array_equal(got[c.name + "/filt"], b["filt"]), (knob, c.name)
            assert np.array_equal(got[c.name + "/idx"], b["idx"]), (knob, c.name)
            assert np.array_equal(got[c.name + "/cost"], b["cost"]), (knob, c.name)
        if knob == "SSYM_SP_PAIRBLOCK":
            assert blocks >= 5, blocks
