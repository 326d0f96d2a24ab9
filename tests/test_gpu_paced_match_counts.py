"""Paced matching with more targets than dtw_match_paced_kernel's grid has columns, and more sources than it has rows
(DESIGN.md section 5.21): 65 600 targets in one call, so that workgroups 0 ... 63 take a second target (t += gridDim.x) and
re-enter the target ring, bound1 / bound2 and the per-lane best triple under it -- the two targets run through every
ordered pair of 8 kinds (tests/count_cases.py, checked in tests/test_count_cases.py) --, and 1030 sources with one source
per block asked for, which the grid-y clamp turns into blocks of 2.  Bit for bit against tests/paced_match_ref.py, which
runs over the distinct targets once."""
import numpy as np
import pytest

import count_cases as cc
import paced_match_ref as ref
from paced_match_gpu import Sets, bits, check_match, check_matrix, match, matrix
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

BASE = 11


@pytest.fixture(scope="module")
def big():
    c = cc.paced_case()
    (c.want,) = cc.gather((c.want_u,), c.ids)
    c.distance = c.distance_u[c.ids]
    c.plain = cc.gather(ref.fold(c.want_u), c.ids)
    c.near = cc.gather(ref.fold(c.want_u, c.distance_u, BASE), c.ids)
    return c


@pytest.fixture(scope="module")
def sets(big):
    with Sets(big.src, big.tgt, big.dim) as s:
        yield s


def test_65600_targets_are_matched(big, sets):
    assert len(big.tgt) == cc.PACED_STRIDE + 64
    check_match(sets, big.want, folded=big.plain)
    idx, cost = check_match(sets, big.want, big.distance, BASE, folded=big.near)
    second = slice(cc.PACED_STRIDE, cc.PACED_STRIDE + 64)
    assert np.isfinite(cost[second]).any() and np.isposinf(cost[second]).any() and (idx[second] != idx[:64]).any()


def test_65600_targets_into_device_memory(big, sets):
    check_match(sets, big.want, big.distance, BASE, folded=big.near, device=True)
    check_match(sets, big.want, folded=big.plain, device=True, want_cost=False)


def test_the_matrix_of_65600_targets(big, sets):
    mat = check_matrix(sets, big.want)
    assert mat.shape == (9, 65600)


@pytest.mark.parametrize("knobs", [{"SSYM_PACED_MATCH_PACK": "0"}, {"SSYM_PACED_MATCH_BLOCK": "1"}])
def test_neither_packs_nor_blocks_matter_beyond_the_grid(big, sets, knobs, monkeypatch):
    base = match(sets, big.distance, BASE)
    base_mat = matrix(sets)[1]
    assert base[0] == nat.SSYM_OK
    with monkeypatch.context() as mp:
        for k, v in knobs.items():
            mp.setenv(k, v)
        mat = check_matrix(sets, big.want)
        assert (bits(mat) == bits(base_mat)).all()
        idx, cost = check_match(sets, big.want, big.distance, BASE, folded=big.near)
        assert np.array_equal(idx, base[1]) and (bits(cost) == bits(base[2])).all()
        check_match(sets, big.want, folded=big.plain)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_grid_y_clamp(dtype, monkeypatch):
    """1030 sources, one per block asked for: kMatchPacedGridY = 1023 makes blocks of 2, and the two sources that equal
    target 0 lie in blocks 510 and 512."""
    src, tgt = cc.clamp_case()
    want = ref.matrix(src, tgt)
    with Sets(src, tgt, 2, dtype) as s:
        plain = match(s)
        with monkeypatch.context() as mp:
            mp.setenv("SSYM_PACED_MATCH_BLOCK", "1")
            check_matrix(s, want)
            idx, cost = check_match(s, want)
            assert idx[0] == 1021 and bits(cost[0]) == bits(0.0)
            idx, _ = check_match(s, want, [0.0, 1.0, 0.5, 3.0, 2.0], base=5, device=True)
            assert idx[0] == 1026
            assert np.array_equal(match(s)[1], plain[1]) and (bits(match(s)[2]) == bits(plain[2])).all()
