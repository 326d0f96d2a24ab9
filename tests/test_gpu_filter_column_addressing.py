"""The column bookkeeping of dtw_filter_kernel (csrc/dtw_filter_kernel.hpp): staging DMAs from a scalar group base, the
hand-off row as a column-major buffer written one column per store, a top buffer of +inf in passes without a row
above, column 0 started by `prevTop`.  The smallest searches that reach every one of those addresses and values.

A case is 8 sources against three sets of 96 targets (three target groups each: a task's group base is not the set's,
and three XCD ranges are walked), 13 values per frame unless the case says otherwise.  Target record slots are ordered
by length, so a set's groups are its 32 shortest, next and longest targets:
    set "a": longest of 1 (with the empty target), of 2 and of 3 frames,
    set "b": longest of 5, of 127 and of 128 frames,
    set "c": one frame each, a ragged group of 1...128 frames, 128 frames each
-- every residue of the column count mod 4 and the clamped look-ahead at the end of a group's records.  The source lengths
choose the passes: 64 (one pass, no top row), 65 (two passes of 48 rows), 64 paired with 128 (two of 64; one lane starts
on the pass boundary), 129 (three passes), 70 with 80 (the SKIP0 instantiation); 20 values (three operand planes), squared
costs and the pruned search ride on the two-pass lengths.

Per case and set: the filter matrix equals the packed kernel's bit for bit, lies within tests/bounds.py of the oracle's,
the search returns the oracle's argmin, and a second run after other searches on the same context returns the same bits
(a stale hand-off row or top buffer would show).  The pruned search returns the unpruned indices and costs.

The packed kernel (csrc/dtw_filter_pk_kernel.hpp, SSYM_FILTER_PK=1) takes launches of four tiles only, and the planner
gives the 65-, 129- and 70/80-frame cases passes of 48 rows (three tiles, SKIP0 for two of them): under the knob alone
they would run the kernel under test again.  So the packed child also sets SSYM_FILTER_LONG_CLASSES=0, which launches
every pair beyond 48 frames on the set's own shape of four tiles -- results do not depend on the pass height -- and the
packed kernel then computes every case.  That it did is read from the launch's cell count: the plan counts no cells
for a launch of the packed kernel, so a packed search reports none.  One child process per setting runs the whole table;
the plain child (SSYM_FILTER_PK=0) is this process's twin.
"""
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

from soundsym_amd import Engine
from bounds import pair_bound_matrix
from filter_long_cases import run_search

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

Case = namedtuple("Case", "name src_lens dim squared prune", defaults=(13, False, False))
TWO_PASS = (64, 128, 128, 128, 128, 128, 128, 128)      # slots by length: pair 0 is (64, 128), r0 = 64 = the second pass's first row
CASES = [
    Case("one_pass_64", (49, 55, 60, 63, 64, 64, 64, 64)),
    Case("two_pass_65", (65, 65, 65, 65, 65, 65, 65, 65)),
    Case("two_pass_64_with_128", TWO_PASS),
    Case("three_pass_129", (100, 129, 129, 129, 129, 129, 129, 129)),
    Case("skip0_70_with_80", (70, 80, 70, 80, 70, 80, 70, 80)),
    Case("dim20", TWO_PASS, 20),
    Case("squared", TWO_PASS, 13, True),
    Case("pruned", TWO_PASS, 13, False, True),
]
SETS = ("a", "b", "c")


def target_lengths(which):
    if which == "a":
        return [0] + [1] * 31 + [2] * 32 + [3] * 32
    if which == "b":
        return [1 + i % 5 for i in range(32)] + [6 + (i * 121) // 31 for i in range(32)] + [128] * 32
    return [1] * 32 + [1 + (i * 127) // 31 for i in range(32)] + [128] * 32


def case_data(case):
    """(src, {set: tgt}): lists of [frames, dim] float32; a few targets are noisy copies of a source's first frames."""
    rng = np.random.default_rng(0xC01ADD + 16 * [c.name for c in CASES].index(case.name))
    src = [rng.standard_normal((f, case.dim)).astype(np.float32) for f in case.src_lens]
    sets = {}
    for which in SETS:
        lens = target_lengths(which)
        assert len(lens) == 96
        tgt = [rng.standard_normal((f, case.dim)).astype(np.float32) for f in lens]
        for t in range(5, 96, 7):
            a = src[t % 8]
            f = min(lens[t], a.shape[0])
            tgt[t][:f] = a[:f] + 0.05 * rng.standard_normal((f, case.dim)).astype(np.float32)
        order = rng.permutation(96)
        sets[which] = [tgt[int(i)] for i in order]
    return src, sets


def run_case(case):
    """Every set of the case searched twice on one context, the other sets' searches in between.  Returns
    {set: result of the FIRST run}, {set: result of the second}, {set: (sf, so, tf, to)}; a pruned case adds the pruned
    search's idx and cost as "pidx" / "pcost"."""
    src, sets = case_data(case)
    e = Engine(metric="dtw", dtype="f32", squared=case.squared)
    try:
        runs, packed = [{}, {}], {}
        for rep in range(2):
            for which in SETS:
                res, (d, q, sf, so, tf, to) = run_search(e, case.dim, src, sets[which])
                if case.prune:
                    res["pidx"], res["pcost"] = e.match(d, q, prune=True)
                    res["pruned"] = int(e.timings()["pruned"])
                runs[rep][which], packed[which] = res, (sf, so, tf, to)
                d.close()
                q.close()
        return runs[0], runs[1], packed
    finally:
        e.close()


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_filter_column_addressing as T
out = {}
for c in T.CASES:
    first, _, _ = T.run_case(c)
    for which, r in first.items():
        for k in ("filt", "idx", "cost", "cells", "launches"):
            out[c.name + "/" + which + "/" + k] = np.asarray(r[k])
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def knob_tables(tmp_path_factory):
    """The whole table on the plain kernel ("0") and on the packed one ("1": four-tile launches throughout), a fresh
    process each."""
    out = {}
    for value, env in (("0", dict(SSYM_FILTER_PK="0")), ("1", dict(SSYM_FILTER_PK="1", SSYM_FILTER_LONG_CLASSES="0"))):
        path = str(tmp_path_factory.mktemp("pk" + value) / "table.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, HERE, path], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, **env))
        assert r.returncode == 0, (value, r.stderr[-3000:])
        out[value] = np.load(path)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_column_addressing_case(oracle, knob_tables, case):
    src, sets = case_data(case)
    first, second, packed = run_case(case)
    for which in SETS:
        tgt, r = sets[which], first[which]
        sf, so, tf, to = packed[which]
        filt, idx, cost = r["filt"], r["idx"], r["cost"]
        assert r["used_filter"] == 1, (which, r)

        # the packed kernel's bits, and the plain child's.  The packed child launched the packed kernel alone (it
        # counts no cells); the plain child and this process ran the planner's launches on the kernel under test
        plain, pk = knob_tables["0"], knob_tables["1"]
        key = case.name + "/" + which + "/"
        assert int(pk[key + "launches"]) >= 1 and int(pk[key + "cells"]) == 0, (which, int(pk[key + "cells"]))
        assert int(plain[key + "cells"]) == r["cells"] > 0 and int(plain[key + "launches"]) == r["launches"], which
        assert np.array_equal(plain[key + "filt"], pk[key + "filt"]), which
        assert np.array_equal(filt, pk[key + "filt"]), which
        assert np.array_equal(idx, pk[key + "idx"]) and np.array_equal(cost, pk[key + "cost"]), which

        # the second run, after the other sets' searches on the same context
        assert np.array_equal(second[which]["filt"], filt), which
        assert np.array_equal(second[which]["idx"], idx) and np.array_equal(second[which]["cost"], cost), which

        want_idx, want_cost, mat = oracle.dtw_match_all(sf.astype(np.float64), so, tf.astype(np.float64), to, case.dim,
                                                        squared=case.squared, want_matrix=True)
        fin = np.isfinite(mat)
        assert np.array_equal(fin, np.array([[a.shape[0] > 0] for a in src]) & np.array([[b.shape[0] > 0 for b in tgt]]))
        assert np.isposinf(filt[~fin]).all() and np.isfinite(filt[fin]).all(), which
        if not case.squared:                              # (squared costs have no restated bound)
            pb = pair_bound_matrix(src, tgt, case.dim)[0]
            err, tol = np.abs(filt[fin] - mat[fin]), (pb + 1e-5 * mat)[fin]
            print("filter err/tol %s/%s: %.4f" % (case.name, which, float((err / tol).max())))
            assert (err <= tol).all(), (which, int((err > tol).sum()), float((err / tol).max()))

        assert np.array_equal(idx, want_idx), which
        have = np.isfinite(want_cost)
        assert np.array_equal(np.isfinite(cost), have), which
        assert np.allclose(cost[have], want_cost[have], rtol=EXACT_RTOL, atol=0), which

        if case.prune:
            for rr in (r, second[which]):
                assert rr["pruned"] == 1, which
                assert np.array_equal(rr["pidx"], idx) and np.array_equal(rr["pcost"], cost), which
