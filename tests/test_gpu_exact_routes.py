"""launch_dtw_exact (csrc/dtw_exact.hip) on every route, against the oracle at 1e-12 relative with equal isinf patterns.

The launcher picks among five kernels by list length, frame width and LDS fit (tests/exact_plan.py restates it, and
tests/test_exact_plan.py pins that restatement to the source and checks on the CPU that every case below lands on the
route it is named for).  A candidate list's length lives on the device and each launched kernel decides from it whether
the list is its business: an off-by-one there leaves a list of exactly that length scored by nobody, and the search
returns what the candidate buffer held before.  So the handoff cases run lists of exactly T - 1, T and T + 1 pairs
(n_refined asserted), every listed pair's cost comes back (top-k with k = all sources) and is compared, every length has
data of its own and follows a call that left other costs in the buffer.

  a. the device-side handoffs cells -> reg, cells -> pipe, pipe -> reg through the filter route
     (guards: `if (total > totalHi)` of dtw_exact_cells_kernel, `if (total < totalLo || total > totalHi)` of
     dtw_exact_pipe_kernel, `if (!redo && (total < totalLo || ...` of dtw_exact_reg_kernel, and the launcher's
     `lowBound = cellsMax + 1` / `regLo = ... pipeMax + 1`)
  b. the host-side decision at the same thresholds: all-pairs calls and the dtw chain
  c. frame widths 1...128 around every rung of the dimr ladder, on the cells and on the register kernel
  d. the LDS limits: the last target length of the register kernel, the generic kernel behind it with its frames in LDS
     and in global memory, the 7680-frame limit
  e. bands the cells kernel does not take (r > 63): the register kernel's windowed staging
  f. the same bits from the cells, the pipelined and the register kernel
num_cus comes from the device; the cases are functions of it.
"""
import math

import numpy as np
import pytest

import exact_plan as xp
from exact_cases import (ALL_PAIRS, BAND_SRC, BAND_TGT, CHAINS, CHAIN_START, CHAIN_STEPS, DIM, DIMS,
                         GENERIC_LDS_DIMS, HANDOFFS, LDS_DIMS, LDS_SRC, LDS_SRC_LONG, LONGEST, SAME_M, SAME_N,
                         SAME_SRC, SAME_TGT, TGT_HI, TGT_LO, WIDE_BANDS, WIDTH_BAND, WIDTH_SRC, WIDTH_TGT, band_want,
                         handoff_lengths, lds_targets, reg_fit, same_bits_targets, split, width_long_sources,
                         width_want)
import tail_ref
from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _np(dtype):
    return np.float32 if dtype == "f32" else np.float64


def _segments(rng, lens, dim, dtype, shift=0.0):
    return [(rng.standard_normal((int(f), dim)) + shift).astype(_np(dtype)) for f in lens]


def _source_lens(rng, n, lo, hi):
    """n lengths in lo...hi, one of them hi (it sets pipeW)."""
    lens = rng.integers(lo, hi + 1, size=n)
    lens[int(rng.integers(0, n))] = hi
    return lens


def _matrix(oracle, src, tgt, dim, band=-1, squared=False):
    sf, so = pack_segments(src, dim, np.float64)
    tf, to = pack_segments(tgt, dim, np.float64)
    return oracle.dtw_match_all(sf, so, tf, to, dim, band=band, squared=squared, nthreads=oracle.max_threads(),
                                want_matrix=True)[2]


def _handles(e, src, tgt, dim):
    sf, so = pack_segments(src, dim, e.np_dtype)
    tf, to = pack_segments(tgt, dim, e.np_dtype)
    return e.dictionary(sf, so, dim), e.queries(tf, to, dim)


def _close(got, want, what=None):
    assert np.array_equal(np.isinf(got), np.isinf(want)), what
    fin = np.isfinite(want)
    assert np.allclose(got[fin], want[fin], rtol=RTOL, atol=0), what
    return bool(np.array_equal(got, want))


# ---- a. device-side handoffs through the filter route ------------------------------------------------------------------
def _with_warm_up(lengths):
    """The first length once more in front, with data of its own: the first checked list, too, follows a call that
    left other costs in the candidate buffer."""
    return lengths[:1] + lengths


def _listed_costs(e, d, q, n):
    """Every source's cost per target through the filter route: (idx [m][n], cost [m][n])."""
    if n == 1:
        idx, cost = e.match(d, q)
        return idx[:, None], cost[:, None]
    return e.match_topk(d, q, n)


def _check_list(e, length):
    tm = e.timings()
    assert tm["used_filter"] == 1 and tm["n_refined"] == length and tm["exact_redone"] == 0, (length, tm)


@pytest.mark.parametrize("case", HANDOFFS, ids=[c[0] for c in HANDOFFS])
def test_device_side_handoffs(oracle, case):
    """N <= 64 distinct sources x M targets = L pairs, top-k with k = N: every pair is a candidate and every cost comes
    back.  (The list's capacity is min(65536, N M) = L here, so the launcher itself stops after the kernel that takes
    max_pairs; the kernels' own comparisons still decide at L = T, and decide alone in the test below.)"""
    name, per_cu, src_hi, dtype, below, above = case
    ncu = num_cus()
    e = Engine(metric="dtw", dtype=dtype)
    try:
        for call, length in enumerate(_with_warm_up(handoff_lengths(per_cu, ncu))):
            n, m = split(length)
            rng = np.random.default_rng([0x5EED0E00, HANDOFFS.index(case), call])
            src = _segments(rng, _source_lens(rng, n, 20, src_hi), DIM, dtype)
            tgt = _segments(rng, rng.integers(TGT_LO, TGT_HI + 1, size=m), DIM, dtype)
            want_route = below if length <= per_cu * ncu else above
            assert xp.route(max(len(s) for s in src), max(len(t) for t in tgt), DIM, dtype, -1, ncu, True, length,
                            length) == want_route
            d, q = _handles(e, src, tgt, DIM)
            idx, cost = _listed_costs(e, d, q, n)
            _check_list(e, length)
            mat = _matrix(oracle, src, tgt, DIM)
            assert np.array_equal(np.sort(idx.astype(np.int64), axis=1), np.tile(np.arange(n), (m, 1))), (name, length)
            bits = _close(cost, mat[idx.astype(np.int64), np.arange(m)[:, None]], (name, length))
            assert (np.diff(cost, axis=1) >= 0).all()
            print("EXACT_BITS a %s L=%d n=%d m=%d route=%s equal=%s" % (name, length, n, m, want_route, bits))
            d.close()
            q.close()
    finally:
        e.close()


@pytest.mark.parametrize("case", HANDOFFS, ids=[c[0] for c in HANDOFFS])
def test_device_side_handoffs_with_room_in_the_list(oracle, case):
    """The same lengths in a list with room for twice as many pairs, so that only the kernels' comparisons with the
    length on the device decide: a plain search over N identical sources (every pair ties, all N M are candidates: the
    construction of test_dtw_candidate_overflow_is_redone_with_the_reported_size) behind N far sources no target lists.
    (Not top-k: its threshold is the k-th smallest distinct bound, which N tied sources do not reach.)"""
    name, per_cu, src_hi, dtype, below, above = case
    ncu = num_cus()
    e = Engine(metric="dtw", dtype=dtype)
    try:
        for call, length in enumerate(_with_warm_up(handoff_lengths(per_cu, ncu))):
            n, m = split(length)
            rng = np.random.default_rng([0x5EED0E40, HANDOFFS.index(case), call])
            one = _segments(rng, [src_hi], DIM, dtype)[0]
            far = _segments(rng, _source_lens(rng, n, max(20, src_hi - 40), src_hi), DIM, dtype, shift=25.0)
            src = far + [one.copy() for _ in range(n)]
            tgt = _segments(rng, rng.integers(TGT_LO, TGT_HI + 1, size=m), DIM, dtype)       # pairwise different
            want_route = below if length <= per_cu * ncu else above
            assert xp.route(src_hi, max(len(t) for t in tgt), DIM, dtype, -1, ncu, True, 2 * length, length) == want_route
            d, q = _handles(e, src, tgt, DIM)
            idx, cost = e.match(d, q)
            _check_list(e, length)
            mat = _matrix(oracle, src[n:n + 1], tgt, DIM)                                    # [1][m]: the tied cost
            assert (idx == n).all(), (name, length)                                          # the first of the tied sources
            _close(cost, mat[0], (name, length))
            d.close()
            q.close()
    finally:
        e.close()


# ---- b. the host-side decision at the same thresholds ------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_PAIRS, ids=["%dcu%+d_src%d_%s" % c for c in ALL_PAIRS])
def test_host_side_decision_all_pairs(oracle, case):
    per_cu, off, src_hi, want_route = case
    ncu = num_cus()
    length = per_cu * ncu + off
    n, m = split(length)
    rng = np.random.default_rng([0x5EED0E80, ALL_PAIRS.index(case)])
    src = _segments(rng, _source_lens(rng, n, 20, src_hi), DIM, "f32")
    tgt = _segments(rng, rng.integers(TGT_LO, TGT_HI + 1, size=m), DIM, "f32")
    assert xp.route(src_hi, max(len(t) for t in tgt), DIM, "f32", -1, ncu, False, length) == want_route
    mat = _matrix(oracle, src, tgt, DIM)
    e = Engine(metric="dtw", dtype="f32")
    try:
        d, q = _handles(e, src, tgt, DIM)
        got = e.pair_matrix(d, q, exact=True)
        _close(got, mat)
        idx, cost = e.match(d, q, force_exact=True)
        tm = e.timings()
        assert tm["used_filter"] == 0 and tm["n_refined"] == length and tm["exact_redone"] == 0, tm
        _close(cost, mat.min(axis=0))
        _close(mat[idx.astype(np.int64), np.arange(m)], mat.min(axis=0))
        assert np.array_equal(got[idx.astype(np.int64), np.arange(m)], cost)
    finally:
        e.close()


@pytest.mark.parametrize("case", CHAINS, ids=["%dcu%+d_%d_%d_%s" % c for c in CHAINS])
def test_host_side_decision_chain(oracle, case):
    per_cu, off, lo, hi, want_route = case
    ncu = num_cus()
    n = per_cu * ncu + off
    rng = np.random.default_rng([0x5EED0EC0, CHAINS.index(case)])
    segs = _segments(rng, _source_lens(rng, n, lo, hi), DIM, "f32")
    start = _segments(rng, [CHAIN_START], DIM, "f32")[0]
    assert xp.route(hi, CHAIN_START, DIM, "f32", -1, ncu, False, n) == want_route
    assert xp.route(hi, hi, DIM, "f32", -1, ncu, True, n, n) == want_route
    cols = {}

    def entry(i):
        if i not in cols:
            cols[i] = _matrix(oracle, segs, [segs[i]], DIM)[:, 0]
        return cols[i]

    start_col = _matrix(oracle, segs, [start], DIM)[:, 0]
    dist = rng.choice(start_col, size=CHAIN_STEPS) * rng.uniform(0.97, 1.03, size=CHAIN_STEPS)
    want_idx, want_val = tail_ref.chain(entry, start_col, dist, math.inf, "value")
    col = start_col                         # the precondition of comparing indices under a cost tolerance
    for step, dd in enumerate(dist):
        k1, k2 = tail_ref.best_two_keys(col, dd)
        assert k1 == k2 or k2 == math.inf or k2 - k1 > 1e-9 * k2, (step, k1, k2)
        col = entry(int(want_idx[step]))
    assert np.unique(want_idx).size >= 2
    e = Engine(metric="dtw", dtype="f32")
    try:
        sf, so = pack_segments(segs, DIM, np.float32)
        idx, val = e.chain(e.dictionary(sf, so, DIM), start, dist)
        assert np.array_equal(idx.astype(np.int64), want_idx), (idx, want_idx)
        _close(val, want_val)
    finally:
        e.close()


# ---- c. frame widths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("dim", DIMS)
def test_frame_widths(oracle, dim, dtype):
    """Every rung of the dimr ladder from both sides, PARTS = 2 (49...64) and 3 (65...96), the generic kernel above:
    once on 9 x 7 pairs (the cells kernel up to 48 values) and once on more than 4 pairs per CU with sources of at
    most 64 frames (the register kernel), unbanded and with a band of 7; squared costs on f64."""
    ncu = num_cus()
    squared = dtype == "f64"
    rng = np.random.default_rng([0x5EED0F00, dim, dtype == "f64"])
    tgt = _segments(rng, WIDTH_TGT, dim, dtype)
    sets = [(True, _segments(rng, WIDTH_SRC, dim, dtype)), (False, _segments(rng, width_long_sources(ncu), dim, dtype))]
    assert all((s[:, -1] != 0).all() for _, ss in sets for s in ss) and all((t[:, -1] != 0).all() for t in tgt)
    for band in (-1, WIDTH_BAND):
        e = Engine(metric="dtw", dtype=dtype, band=band, squared=squared)
        try:
            for short, src in sets:
                want_route = width_want(dim, band, short)
                assert len(src) * len(tgt) > xp.CELLS_PER_CU * ncu or short
                assert xp.route(max(len(s) for s in src), max(WIDTH_TGT), dim, dtype, band, ncu, False,
                                len(src) * len(tgt)) == want_route
                mat = _matrix(oracle, src, tgt, dim, band=band, squared=squared)
                assert np.isfinite(mat).sum() >= 4 and np.isinf(mat).any()
                d, q = _handles(e, src, tgt, dim)
                bits = _close(e.pair_matrix(d, q, exact=True), mat, (dim, dtype, band, short))
                print("EXACT_BITS c dim=%d %s band=%d route=%s equal=%s" % (dim, dtype, band, want_route, bits))
                d.close()
                q.close()
        finally:
            e.close()


# ---- d. LDS fallbacks ----------------------------------------------------------------------------------------------------
def _lds_case(oracle, e, ncu, dim, dtype, src_lens, fb, want_route, seed):
    rng = np.random.default_rng(seed)
    src, tgt = _segments(rng, src_lens, dim, dtype), _segments(rng, lds_targets(fb), dim, dtype)
    assert xp.route(max(src_lens), fb, dim, dtype, -1, ncu, False, len(src) * len(tgt)) == want_route, (dim, dtype, fb)
    mat = _matrix(oracle, src, tgt, dim)
    d, q = _handles(e, src, tgt, dim)
    bits = _close(e.pair_matrix(d, q, exact=True), mat, (dim, dtype, fb, want_route))
    print("EXACT_BITS d dim=%d %s fb=%d route=%s equal=%s" % (dim, dtype, fb, want_route, bits))
    d.close()
    q.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("dim", LDS_DIMS)
def test_register_kernel_lds_limit_and_the_generic_kernel_behind_it(oracle, dim, dtype):
    """`regLds <= 64 KiB`: the longest target that fits (fbEven: an even length), the next length and the one after.
    This departs from the issue, which expected generic_lds at that length + 2: at 13 and 40 values the generic kernel's
    own frames never fit its 64 KiB where the register kernel's do not (its rows are wider), so what lies behind the
    limit is dtw_exact_kernel<false> (generic_global), asserted here from the plan; the <true> | <false> edge the issue
    asked for is run where it exists, at 97 and 124 values, in the test below."""
    ncu = num_cus()
    fit = reg_fit(dim, dtype, ncu)
    assert fit % 2 == 0 and xp.reg_lds_bytes(fit, dim, dtype, -1) <= 64 * 1024 < xp.reg_lds_bytes(fit + 1, dim, dtype, -1)
    assert xp.longest_target("generic_lds", max(LDS_SRC), dim, dtype, -1, ncu, 12, limit=2048) is None
    dimr = xp.exact_dimr(dim)
    e = Engine(metric="dtw", dtype=dtype)
    try:
        for k, (fb, a, b) in enumerate(((fit, "pipe", "reg%d" % dimr), (fit + 1, "generic_global", "generic_global"),
                                        (fit + 2, "generic_global", "generic_global"))):
            _lds_case(oracle, e, ncu, dim, dtype, LDS_SRC, fb, a, [0x5EED0F40, dim, k])
            _lds_case(oracle, e, ncu, dim, dtype, LDS_SRC_LONG, fb, b, [0x5EED0F41, dim, k])
    finally:
        e.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("dim", GENERIC_LDS_DIMS)
def test_generic_kernel_frames_in_lds_and_in_global_memory(oracle, dim, dtype):
    """`boundBytes + frameBytes <= 64 KiB`: the last target length of dtw_exact_kernel<true> and the first of <false>."""
    ncu = num_cus()
    last = xp.longest_target("generic_lds", max(LDS_SRC), dim, dtype, -1, ncu, 12, limit=2048)
    assert last is not None and last >= 1
    e = Engine(metric="dtw", dtype=dtype)
    try:
        _lds_case(oracle, e, ncu, dim, dtype, LDS_SRC, last, "generic_lds", [0x5EED0F50, dim, 0])
        _lds_case(oracle, e, ncu, dim, dtype, LDS_SRC, last + 1, "generic_global", [0x5EED0F50, dim, 1])
    finally:
        e.close()


def test_longest_target_and_the_refusal_past_it(oracle):
    """`boundBytes > 120 * 1024`: 7680 frames are scored, 7681 are SSYM_E_UNSUPPORTED with a message, and the engine
    answers the next call correctly."""
    ncu = num_cus()
    rng = np.random.default_rng(0x5EED0F60)
    src = _segments(rng, [3, 70], DIM, "f32")
    tgt, over = _segments(rng, [LONGEST], DIM, "f32"), _segments(rng, [LONGEST + 1], DIM, "f32")
    assert xp.route(70, LONGEST, DIM, "f32", -1, ncu, False, 2) == "generic_global"
    assert xp.route(70, LONGEST + 1, DIM, "f32", -1, ncu, False, 2) == "unsupported"
    mat = _matrix(oracle, src, tgt, DIM)
    e = Engine(metric="dtw", dtype="f32")
    try:
        d, q = _handles(e, src, tgt, DIM)
        _close(e.pair_matrix(d, q, exact=True), mat)
        _, qo = _handles(e, src[:1], over, DIM)
        for call in (lambda: e.pair_matrix(d, qo, exact=True), lambda: e.match(d, qo, force_exact=True)):
            with pytest.raises(nat.SsymError) as err:
                call()
            assert err.value.code == nat.SSYM_E_UNSUPPORTED and "too long" in str(err.value)
        _close(e.pair_matrix(d, q, exact=True), mat)
        idx, cost = e.match(d, q, force_exact=True)
        assert idx[0] == int(np.argmin(mat[:, 0]))
        _close(cost, mat.min(axis=0))
    finally:
        e.close()


# ---- e. bands the cells kernel does not take ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("dim", LDS_DIMS)
@pytest.mark.parametrize("band", WIDE_BANDS)
def test_bands_past_the_cells_kernel(oracle, band, dim, dtype):
    """`panelX <= 128`: r = 64 is the first band of the register kernel, which stages 64 + 2 r + 1 target rows per
    chunk of 64 source rows; pairs more than r frames apart in length end outside the band (+inf)."""
    ncu = num_cus()
    assert xp.route(max(BAND_SRC), max(BAND_TGT), dim, dtype, 63, ncu, False, 36) == "cells"
    assert xp.route(max(BAND_SRC), max(BAND_TGT), dim, dtype, band, ncu, False, 36) == band_want(dim, dtype)
    rng = np.random.default_rng([0x5EED0F80, band, dim])
    src, tgt = _segments(rng, BAND_SRC, dim, dtype), _segments(rng, BAND_TGT, dim, dtype)
    mat = _matrix(oracle, src, tgt, dim, band=band)
    apart = np.abs(np.array(BAND_SRC)[:, None] - np.array(BAND_TGT)[None, :]) > band
    assert np.array_equal(np.isinf(mat), apart) and apart.sum() >= 6 and (~apart).sum() >= 6
    e = Engine(metric="dtw", dtype=dtype, band=band)
    try:
        d, q = _handles(e, src, tgt, dim)
        _close(e.pair_matrix(d, q, exact=True), mat)
        idx, cost = e.match(d, q, force_exact=True)
        _close(cost, mat.min(axis=0))
    finally:
        e.close()


# ---- f. the same bits on whichever kernel ------------------------------------------------------------------------------
def test_same_bits_from_cells_pipe_and_reg(oracle):
    ncu = num_cus()
    rng = np.random.default_rng(0x5EED0FA0)
    src = _segments(rng, [SAME_SRC] * SAME_N, DIM, "f32")
    m_all = same_bits_targets(ncu)[-1][0]
    tgt = _segments(rng, [SAME_TGT] * m_all, DIM, "f32")
    mat = _matrix(oracle, src, tgt[:SAME_M], DIM)
    e = Engine(metric="dtw", dtype="f32")
    try:
        all_pairs, listed = [], []
        for m, want_route in same_bits_targets(ncu):
            for is_list in (False, True):
                assert xp.route(SAME_SRC, SAME_TGT, DIM, "f32", -1, ncu, is_list, SAME_N * m) == want_route
            d, q = _handles(e, src, tgt[:m], DIM)
            all_pairs.append(e.pair_matrix(d, q, exact=True)[:, :SAME_M])
            idx, cost = e.match_topk(d, q, SAME_N)                   # the same pairs as a candidate list
            _check_list(e, SAME_N * m)
            by_source = np.zeros((SAME_N, SAME_M))
            by_source[idx[:SAME_M].astype(np.int64), np.arange(SAME_M)[:, None]] = cost[:SAME_M]
            listed.append(by_source)
            d.close()
            q.close()
        _close(all_pairs[0], mat)
        for got in all_pairs[1:] + listed:
            assert np.array_equal(got, all_pairs[0])
        print("EXACT_BITS f equal=%s" % np.array_equal(all_pairs[0], mat))
    finally:
        e.close()
