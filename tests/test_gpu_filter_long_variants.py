"""The multi-pass launches of the dtw MFMA filter (csrc/dtw_filter.hip launch_dtw_filter, the LongClass block), pair by
pair against the oracle: sources beyond 48 frames.

tests/test_gpu_filter_variants.py holds the single-pass variants; this file the rest of the unbanded filter.  A class of
source pairs runs passes of 48 or of 64 rows of dtw_filter_kernel, whichever pads its sources least, on the last rows of
their end-aligned slots, with the boundary row handed from pass to pass; small classes join their successor, the set's
own shape takes what the counter sets do not reach, and a class whose shorter sources leave first tiles empty runs the
SKIP0 instantiation.  Each case of tests/filter_long_cases.py names the classes it must launch; tests/filter_plan.py
restates the plan, and the timings' launch and cell counts prove that the case ran it and that the A/B comparisons
compare two different launches.

Per case: the whole filter matrix within the per-pair bound of tests/bounds.py after the scratch has been filled with
another search of the same lengths, the exact matrix and every target's argmin against the oracle, the same bits under
SSYM_FILTER_SKIP0=0 (in process), and under SSYM_FILTER_LONG_CLASSES=0 and SSYM_FILTER_ONE_LAUNCH (a child process
each).  One source of 4097 frames takes the search off the filter.

Worst measured |filter - oracle| / tolerance per case: LAB.md, "filter variants beyond 48 frames".
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from soundsym_amd import Engine
from soundsym_amd.engine import pack_segments
from bounds import pair_bound_matrix
from filter_plan import filter_plan, plan_cells, plan_classes
from filter_long_cases import LONG_CASES, beyond_reach_data, long_case_data, run_search

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _lens(segs):
    return [a.shape[0] for a in segs]


@pytest.mark.parametrize("case", LONG_CASES, ids=[c.name for c in LONG_CASES])
def test_long_filter_variant_against_oracle(oracle, case):
    src, tgt = long_case_data(case)
    ncu = num_cus()
    ls, lt = _lens(src), _lens(tgt)
    plan, _ = filter_plan(ls, lt, case.dim, ncu)
    assert plan_classes(plan) == case.classes, plan
    skips = any(x.skip for x in plan)
    e = Engine(metric="dtw", dtype="f32", squared=case.squared)
    try:
        # stale-task check: the scratch cost matrix first holds another search of the same lengths
        fill, hs = run_search(e, case.dim, *long_case_data(case, values_seed=0x5EEDF0FF))
        for h in hs[:2]:
            h.close()
        res, (d, q, sf, so, tf, to) = run_search(e, case.dim, src, tgt)
        filt, idx, cost = res["filt"], res["idx"], res["cost"]
        # the launches ran the restated plan, whose cells differ from those of the plan a knob would pick instead
        assert res["used_filter"] == 1 and res["launches"] == len(plan), (res["launches"], plan)
        assert res["cells"] == plan_cells(plan), (res["cells"], plan_cells(plan), plan)
        alt, _ = filter_plan(ls, lt, case.dim, ncu, skip0=False) if skips else \
            filter_plan(ls, lt, case.dim, ncu, long_classes=False)
        if case.name == "equal_128":                       # one class of the set's own shape: every knob launches the same
            assert alt == plan
        else:
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
            print("filter err/tol %s: %.4f" % (case.name, float((err / tol).max())))
            assert (err <= tol).all(), (int((err > tol).sum()), float((err / tol).max()))
        exact = e.pair_matrix(d, q, exact=True)
        assert np.array_equal(np.isfinite(exact), fin)
        assert np.allclose(exact[fin], mat[fin], rtol=EXACT_RTOL, atol=0)

        # the search: the oracle's argmin (first index on ties) for every target
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(np.isfinite(cost), np.isfinite(want_cost))
        have = np.isfinite(want_cost)
        assert np.allclose(cost[have], want_cost[have], rtol=EXACT_RTOL, atol=0)

        # SSYM_FILTER_SKIP0=0 (read per launch): the plain instantiation on every class, the same bits
        if skips:
            os.environ["SSYM_FILTER_SKIP0"] = "0"
            try:
                plain, _ = run_search(e, case.dim, src, tgt)
            finally:
                del os.environ["SSYM_FILTER_SKIP0"]
            assert plain["cells"] == plan_cells(alt) != res["cells"] and plain["launches"] == len(alt)
            assert np.array_equal(plain["filt"], filt)
            assert np.array_equal(plain["idx"], idx) and np.array_equal(plain["cost"], cost)
    finally:
        e.close()


def test_a_source_beyond_4096_frames_takes_the_exact_kernel(oracle):
    src, tgt, dim = beyond_reach_data()
    assert max(_lens(src)) == 4097
    sf, so = pack_segments(src, dim, np.float32)
    tf, to = pack_segments(tgt, dim, np.float32)
    e = Engine(metric="dtw", dtype="f32")
    try:
        idx, cost = e.match(e.dictionary(sf, so, dim), e.queries(tf, to, dim))
        assert e.timings()["used_filter"] == 0
        want_idx, want_cost = oracle.dtw_match_all(sf.astype(np.float64), so, tf.astype(np.float64), to, dim, nthreads=16)
        assert np.array_equal(idx, want_idx)
        have = np.isfinite(want_cost)
        assert np.array_equal(np.isfinite(cost), have) and have.sum() == len(tgt) - 1
        assert np.allclose(cost[have], want_cost[have], rtol=EXACT_RTOL, atol=0)
    finally:
        e.close()


# ---- the whole table under a knob: a child process each ---------------------------------------------------------------
_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import filter_long_cases as C
from soundsym_amd import Engine
out = {}
for c in C.LONG_CASES:
    e = Engine(metric="dtw", dtype="f32", squared=c.squared)
    src, tgt = C.long_case_data(c)
    r, _ = C.run_search(e, c.dim, src, tgt)
    for k, v in r.items():
        out[c.name + "/" + k] = np.asarray(v)
    e.close()
np.savez(sys.argv[3], **out)
"""


def _run_table_in_process():
    out = {}
    for c in LONG_CASES:
        e = Engine(metric="dtw", dtype="f32", squared=c.squared)
        try:
            out[c.name], _ = run_search(e, c.dim, *long_case_data(c))
        finally:
            e.close()
    return out


def test_long_classes_and_one_launch_knobs_same_bits(tmp_path):
    """SSYM_FILTER_LONG_CLASSES=0 (the set's own shape for every pair beyond 48 frames) and SSYM_FILTER_ONE_LAUNCH (for
    every pair) give the default's filter matrices and search results bit for bit, case by case, with the cells and
    launches of the corresponding restated plan."""
    ncu = num_cus()
    base = _run_table_in_process()
    for knob, value, kw in (("SSYM_FILTER_LONG_CLASSES", "0", dict(long_classes=False)),
                            ("SSYM_FILTER_ONE_LAUNCH", "1", dict(one_launch=True))):
        path = str(tmp_path / (knob + ".npz"))
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, HERE, path], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, **{knob: value}))
        assert r.returncode == 0, (knob, r.stderr[-3000:])
        got = np.load(path)
        differ = 0
        for c in LONG_CASES:
            b = base[c.name]
            src, tgt = long_case_data(c)
            plan, _ = filter_plan(_lens(src), _lens(tgt), c.dim, ncu)
            other, _ = filter_plan(_lens(src), _lens(tgt), c.dim, ncu, **kw)
            assert b["cells"] == plan_cells(plan) and b["launches"] == len(plan), (knob, c.name)
            assert int(got[c.name + "/used_filter"]) == 1
            assert int(got[c.name + "/cells"]) == plan_cells(other), (knob, c.name)
            assert int(got[c.name + "/launches"]) == len(other), (knob, c.name)
            differ += plan_cells(other) != plan_cells(plan)
            assert np.array_equal(got[c.name + "/filt"], b["filt"]), (knob, c.name)
            assert np.array_equal(got[c.name + "/idx"], b["idx"]), (knob, c.name)
            assert np.array_equal(got[c.name + "/cost"], b["cost"]), (knob, c.name)
        assert differ == len(LONG_CASES) - 1, (knob, differ)           # (equal_128: the same launch either way)
