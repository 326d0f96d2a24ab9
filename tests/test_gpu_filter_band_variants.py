"""Every instantiation of the banded dtw filter (csrc/dtw_band_kernel.hpp through dtw_filter.hip launch_band), pair by
pair against the banded oracle, with ragged lengths.

launch_band picks NTB = 1...6 tiles of diagonals from the radius, LASTN = 1 where the band ends one diagonal into its
last tile (radii that are multiples of 8) and 16 otherwise, workgroups of 8 waves up to NTB = 5 and of 4 at 6, two or
three operand planes from the dim, squared or plain costs.  tests/filter_long_cases.py has one radius per (NTB, LASTN)
(tests/test_filter_plan.py checks that on the CPU) and 257 targets: n_pad 512, two 8-wave target blocks or four 4-wave
ones, the last one almost empty.

Per radius, after the scratch has been filled with another search of the same lengths: the filter matrix finite exactly
where the end cell lies inside the band (|fa - fb| <= r, both segments non-empty), every finite pair within the per-pair
bound of tests/bounds.py, the exact matrix and every target's argmin against the oracle, and the same bits on a second
call.  A band the kernel cannot take (r = 48; a source pair beyond the LDS) is served by the UNBANDED filter
(filter_band_as_bound): finite wherever both segments have frames, within the bound of the unbanded oracle matrix.

Worst measured |filter - oracle| / tolerance per radius: LAB.md, "filter variants beyond 48 frames".
"""
import numpy as np
import pytest

from soundsym_amd import Engine
from bounds import pair_bound_matrix
from filter_long_cases import BAND_CASES, band_data, band_instance, run_search

pytestmark = pytest.mark.gpu
EXACT_RTOL = 1e-12


def _lens(segs):
    return np.array([a.shape[0] for a in segs])


def _oracle(oracle, sf, so, tf, to, dim, band, squared=False):
    return oracle.dtw_match_all(sf.astype(np.float64), so, tf.astype(np.float64), to, dim, band=band, squared=squared,
                                want_matrix=True, nthreads=16)


def _check_search(res, want_idx, want_cost):
    assert np.array_equal(res["idx"], want_idx)
    have = np.isfinite(want_cost)
    assert np.array_equal(np.isfinite(res["cost"]), have)
    assert np.allclose(res["cost"][have], want_cost[have], rtol=EXACT_RTOL, atol=0)


@pytest.mark.parametrize("case", BAND_CASES, ids=["r%d_dim%d%s" % (c.r, c.dim, "_squared" if c.squared else "") for c in BAND_CASES])
def test_band_variant_against_oracle(oracle, case):
    r, dim = case.r, case.dim
    src, tgt = band_data(r, dim)
    e = Engine(metric="dtw", dtype="f32", band=r, squared=case.squared)
    try:
        fill, hs = run_search(e, dim, *band_data(r, dim, values_seed=0x5EEDF0FE))
        for h in hs[:2]:
            h.close()
        res, (d, q, sf, so, tf, to) = run_search(e, dim, src, tgt)
        filt = res["filt"]
        assert res["used_filter"] == 1 and res["launches"] == 1, (res["launches"], band_instance(r))
        want_idx, want_cost, mat = _oracle(oracle, sf, so, tf, to, dim, r, case.squared)
        fa, fb = _lens(src)[:, None], _lens(tgt)[None, :]
        fin = np.isfinite(mat)
        assert np.array_equal(fin, (np.abs(fa - fb) <= r) & (fa > 0) & (fb > 0)) and fin.any() and not fin.all()
        assert np.isposinf(filt[~fin]).all()
        assert np.isfinite(filt[fin]).all()
        if not case.squared:                              # (squared costs have no restated bound)
            pb = pair_bound_matrix(src, tgt, min(dim, 42))[0]
            err, tol = np.abs(filt[fin] - mat[fin]), (pb + 1e-5 * mat)[fin]
            print("band filter err/tol r=%d dim=%d: %.4f" % (r, dim, float((err / tol).max())))
            assert (err <= tol).all(), (int((err > tol).sum()), float((err / tol).max()))
        exact = e.pair_matrix(d, q, exact=True)
        assert np.array_equal(np.isfinite(exact), fin)
        assert np.allclose(exact[fin], mat[fin], rtol=EXACT_RTOL, atol=0)
        _check_search(res, want_idx, want_cost)
        # a second call: identical bits
        again, _ = run_search(e, dim, src, tgt)
        assert np.array_equal(again["filt"], filt)
        assert np.array_equal(again["idx"], res["idx"]) and np.array_equal(again["cost"], res["cost"])
    finally:
        e.close()


@pytest.mark.parametrize("r,long_source", [(48, 0), (8, 900)], ids=["r48", "r8_pair_beyond_lds"])
def test_band_the_kernel_cannot_take_runs_the_unbanded_filter(oracle, r, long_source):
    dim = 13
    src, tgt = band_data(r, dim, long_source=long_source)
    e = Engine(metric="dtw", dtype="f32", band=r)
    try:
        fill, hs = run_search(e, dim, *band_data(r, dim, values_seed=0x5EEDF0FE, long_source=long_source))
        for h in hs[:2]:
            h.close()
        res, (d, q, sf, so, tf, to) = run_search(e, dim, src, tgt)
        filt = res["filt"]
        assert res["used_filter"] == 1
        fa, fb = _lens(src)[:, None], _lens(tgt)[None, :]
        full = (fa > 0) & (fb > 0)
        # finite even where the end cell lies outside the band: the unbanded kernel ran
        assert (full & (np.abs(fa - fb) > r)).any()
        assert np.isfinite(filt[full]).all() and np.isposinf(filt[~full]).all()
        _, _, umat = _oracle(oracle, sf, so, tf, to, dim, -1)
        want_idx, want_cost, bmat = _oracle(oracle, sf, so, tf, to, dim, r)
        assert np.array_equal(np.isfinite(umat), full)
        pb = pair_bound_matrix(src, tgt, dim)[0]
        err, tol = np.abs(filt[full] - umat[full]), (pb + 1e-5 * umat)[full]
        print("band-as-bound filter err/tol r=%d: %.4f" % (r, float((err / tol).max())))
        assert (err <= tol).all(), (int((err > tol).sum()), float((err / tol).max()))
        assert (filt[full] <= (bmat + pb + 1e-5 * umat)[full]).all()       # ... hence a lower bound of the banded cost
        _check_search(res, want_idx, want_cost)
    finally:
        e.close()
