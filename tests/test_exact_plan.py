"""tests/exact_plan.py against soundsym_amd/csrc/dtw_exact.hip, and the cases of tests/exact_cases.py (what
tests/test_gpu_exact_routes.py runs) against the plan (CPU only).

The plan restates the launcher's routing; the GPU cases stand on its thresholds.  This file reads every factor and limit
out of the source and asserts that each is found exactly once where the plan expects it, so that a changed threshold
fails here and does not silently move the GPU cases off their edges.  Then, for the MI355X's 256 CUs and two other
counts, every GPU case must land on the kernel it is named for, and every list length must be scored by exactly one of
the kernels the plan launches.
"""
import os
import re

import numpy as np
import pytest

import exact_plan as xp
import exact_cases as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "soundsym_amd", "csrc")
CU_COUNTS = [256, 64, 304]
KIB = r"(\d+) \* 1024"


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


SRC = _read("dtw_exact.hip")
LAUNCHER = SRC[SRC.index("int32_t launch_dtw_exact("):].replace("\\\n", "\n")      # (macros: no line continuations)


def _once(pattern, text=LAUNCHER):
    """The groups of the one match of `pattern` (a regular expression) in text, as integers."""
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    groups = found[0] if isinstance(found[0], tuple) else (found[0],)
    return tuple(int(g) for g in groups)


def _count(expr, text=SRC):
    """Occurrences of a C++ expression in text, whatever the white space between its tokens (comments are no part of it)."""
    return len(re.findall(r"\s*".join(re.escape(tok) for tok in expr.split()), text))


# ---- the factors and limits, each exactly once where the plan expects it ------------------------------------------------
def test_list_length_factors():
    assert _once(r"cellsMax = banded \? ~0ull : \(maxEnv > 0 \? \(uint64_t\)maxEnv : \(uint64_t\)ctx->num_cus \* (\d+)\);") \
        == (xp.CELLS_PER_CU,)
    assert _once(r"pipeMax = \(uint64_t\)ctx->num_cus \* (\d+) / std::max<uint32_t>\(pipeW, 1\);") == (xp.PIPE_PER_CU,)
    assert _once(r"pipeW = \(src\.max_frames \+ (\d+)\) / (\d+);") == (63, 64)
    assert _once(r"pipeW >= (\d+) && pipeW <= (\d+)") == (xp.PIPE_W_MIN, xp.PIPE_W_MAX)
    assert _once(r"src\.max_frames <= (\d+)") == (xp.CELLS_SRC_FRAMES,)
    # the launcher's four num_cus products: the two grids beside the two maxima
    assert sorted(int(v) for v in re.findall(r"num_cus \* (\d+)", LAUNCHER)) == sorted([64, xp.CELLS_PER_CU, 8, xp.PIPE_PER_CU])


def test_handoff_comparisons():
    """The device-side comparisons and the thresholds the launcher hands them."""
    assert _count("if (total > totalHi)") == 1                      # cells
    assert _count("if (total < totalLo || total > totalHi)") == 1    # pipe
    assert _count("if (!redo && (total < totalLo || total > totalHi))") == 1                  # reg
    assert _count("total > totalHi") == 3 and _count("total < totalLo") == 2 and _count("total >= totalHi") == 0
    assert _count("total = c < maxPairs ? c : maxPairs;") == 4                  # the three and the generic kernel
    assert _count("lowBound = cellsMax + 1;", LAUNCHER) == 1
    assert _count("regLo = (!pairs || max_pairs <= pipeMax) ? ~0ull : pipeMax + 1;", LAUNCHER) == 1
    assert _count("regLo = lowBound;", LAUNCHER) == 1
    assert _count("(pairs != nullptr || total <= cellsMax);", LAUNCHER) == 1
    assert _count("if (total <= cellsMax)", LAUNCHER) == 1
    assert _count("if (pipeOk && lowBound <= pipeMax && !(pairs == nullptr && total > pipeMax)) {", LAUNCHER) == 1
    assert _count("max_pairs, fbEven, panelX, out, cellsMax);", LAUNCHER) == 1
    assert _count("max_pairs, fbEven, out, lowBound, pipeMax, failCount, forceGiveUp);", LAUNCHER) == 1
    assert _count("max_pairs, fbEven, out, regLo, ~0ull,", LAUNCHER) == 1


def test_frame_width_ladder():
    m = re.findall(r"const int dimr = (.*?);", LAUNCHER, flags=re.S)
    assert len(m) == 1
    rungs = re.findall(r"dim <= (\d+) \? (\d+)", m[0])
    assert [(int(a), int(b)) for a, b in rungs] == [(r, r) for r in xp.DIMR_LADDER]
    assert re.sub(r"\s+", " ", m[0]).endswith("dim <= 96 ? 96 : 0")
    assert re.findall(r"dimr <= (\d+)", LAUNCHER) == [str(xp.NARROW_DIMR)] * 2              # cellsOk, pipeOk
    cases = re.findall(r"case (\d+): SSYM_EXACT_REG\((\d+), (\d)\);", LAUNCHER) + \
        re.findall(r"default: SSYM_EXACT_(REG)\((\d+), (\d)\);", LAUNCHER)
    assert [(c[1], c[2]) for c in cases] == [("12", "1"), ("14", "1"), ("16", "1"), ("40", "1"), ("48", "1"), ("64", "2"),
                                             ("96", "3")]
    for kernel in ("CELLS", "PIPE"):
        assert re.findall(r"case (\d+): SSYM_EXACT_%s\(\1\);" % kernel, LAUNCHER) == ["12", "14", "16", "40"]
        assert _count("default: SSYM_EXACT_%s(48); break;" % kernel, LAUNCHER) == 1


def test_lds_limits():
    assert _once(r"boundBytes > " + KIB) == (xp.BOUND_KIB,)
    assert _once(r"regLds <= \(size_t\)\(dimr >= (\d+) \? (\d+) : (\d+)\) \* 1024") == (64, xp.REG_LDS_WIDE_KIB, xp.REG_LDS_KIB)
    assert re.findall(r"regLds <= " + KIB, LAUNCHER) == [str(xp.REG_LDS_KIB)] * 2            # cellsOk, pipeOk
    assert _once(r"cellsLds <= " + KIB) == (xp.CELLS_LDS_KIB,)
    assert _once(r"pipeLds <= " + KIB) == (xp.PIPE_LDS_KIB,)
    assert _once(r"ldsFrames = boundBytes \+ frameBytes <= " + KIB) == (xp.GENERIC_LDS_KIB,)
    assert _once(r"panelX <= (\d+)") == (xp.PANEL_MAX,)
    assert _once(r"std::min<uint32_t>\(fbEven, panelEnv > 0 \? panelEnv : (\d+)\)") == (xp.PANEL_MAX,)
    # the sizes themselves
    assert _count("boundBytes = 2 * (size_t)fbCap * sizeof(double);", LAUNCHER) == 1
    assert _count("frameBytes = (64 * (size_t)(dim | 1u) + (size_t)fbCap * (dim | 1u)) * sizeof(double);", LAUNCHER) == 1
    assert _count("fbEven = (fbCap + 1) & ~1u;", LAUNCHER) == 1
    assert _count("std::min<uint32_t>(fbEven, (64 + 2 * (uint32_t)ctx->band + 1) & ~1u) : fbEven;", LAUNCHER) == 1
    assert _count("regLds = 2 * (size_t)fbEven * sizeof(double) + (size_t)winRows * ldr * (bf32 ? sizeof(float) : "
                  "sizeof(double));", LAUNCHER) == 1
    assert _count("cellsLds = 2 * (size_t)fbEven * sizeof(double) + (size_t)panelX * 64 * sizeof(double) +", LAUNCHER) == 1
    assert _count("pipeLds = (size_t)pipeW * fbEven * sizeof(double) + (size_t)fbEven * ldp * (bf32 ? sizeof(float) : "
                  "sizeof(double)) +", LAUNCHER) == 1
    assert _count("panelX = banded ? 2 * (uint32_t)ctx->band + 1 :", LAUNCHER) == 1


def test_row_strides():
    assert _count("constexpr int wave_ld(int dimr) { return dimr % 4 == 2 ? dimr : dimr + 2; }", _read("dtw_wave.hpp")) == 1
    assert _count("const int up4 = (dimr + 3) / 4 * 4;", LAUNCHER) == 1
    assert _count("const int ldr = bf32 ? up4 + (up4 % 8 == 4 ? 0 : 4) : wave_ld(dimr);", LAUNCHER) == 1
    assert [xp.wave_ld(r) for r in xp.DIMR_LADDER] == [14, 14, 18, 42, 50, 66, 98]
    assert [xp.exact_ld(r, True) for r in xp.DIMR_LADDER] == [12, 20, 20, 44, 52, 68, 100]      # = 4 (mod 8) floats
    assert all(xp.exact_ld(r, True) % 8 == 4 and xp.wave_ld(r) % 4 == 2 for r in xp.DIMR_LADDER)


# ---- the plan itself ----------------------------------------------------------------------------------------------------
def test_thresholds_as_functions_of_num_cus():
    for ncu in CU_COUNTS:
        p = xp.exact_plan(230, 30, 13, "f32", -1, ncu, True, 65536)
        assert p == xp.Plan(("cells", "pipe", "reg14"), 4 * ncu, 4 * ncu + 1, 16 * ncu, 16 * ncu + 1)
        p = xp.exact_plan(500, 30, 13, "f32", -1, ncu, True, 65536)
        assert p == xp.Plan(("pipe", "reg14"), None, 0, 8 * ncu, 8 * ncu + 1)
        p = xp.exact_plan(64, 30, 13, "f32", -1, ncu, True, 65536)
        assert p == xp.Plan(("cells", "reg14"), 4 * ncu, None, None, 4 * ncu + 1)
        # a list whose capacity the pipelined kernel covers: the register kernel only redoes a give-up
        p = xp.exact_plan(230, 30, 13, "f32", -1, ncu, True, 16 * ncu)
        assert p == xp.Plan(("cells", "pipe", "reg14"), 4 * ncu, 4 * ncu + 1, 16 * ncu, xp.U64_MAX)
        assert xp.exact_plan(230, 30, 13, "f32", -1, ncu, True, 4 * ncu).launched == ("cells",)
        # banded: the cells kernel at every length up to r = 63, the register kernel past it
        assert xp.exact_plan(230, 300, 40, "f32", 63, ncu, True, 65536) == xp.Plan(("cells",), xp.U64_MAX, None, None, None)
        assert xp.exact_plan(230, 300, 40, "f32", 64, ncu, True, 65536) == xp.Plan(("reg40",), None, None, None, 0)
    assert xp.exact_plan(70, 7681, 13, "f32", -1, 256, False, 2).launched == ("unsupported",)
    assert xp.exact_plan(70, 7680, 13, "f32", -1, 256, False, 2).launched == ("generic_global",)


@pytest.mark.parametrize("ncu", CU_COUNTS)
def test_plan_scores_every_length_exactly_once(ncu):
    """The plan against itself: whatever the capacity of a list and its length, exactly one of the kernels the plan
    launches takes it by the plan's thresholds.  This says something about the launcher only as far as the pins above
    tie the plan to it; that the kernels obey the thresholds is what tests/test_gpu_exact_routes.py runs."""
    edges = sorted({1, 2, 4 * ncu, 8 * ncu, 64 * ncu // 3, 64 * ncu // 5, 64 * ncu // 6, 64 * ncu // 7, 16 * ncu, 32 * ncu,
                    65536})
    lengths = sorted({max(v + o, 1) for v in edges for o in (-1, 0, 1)})
    for src in (1, 64, 65, 128, 129, 192, 230, 256, 257, 320, 384, 448, 512, 513, 4096):
        for tgt, dim, dtype, band in ((30, 13, "f32", -1), (30, 13, "f64", -1), (140, 48, "f64", -1), (140, 49, "f32", -1),
                                      (140, 96, "f64", -1), (140, 97, "f32", -1), (683, 13, "f32", -1), (300, 40, "f32", 32),
                                      (300, 40, "f64", 64), (400, 13, "f32", 100), (7680, 13, "f32", -1)):
            for cap in lengths:
                listed = xp.exact_plan(src, tgt, dim, dtype, band, ncu, True, cap)
                for length in [v for v in lengths if v <= cap]:
                    assert len(xp.workers(listed, length)) == 1, (src, tgt, dim, dtype, band, cap, length, listed)
                host = xp.exact_plan(src, tgt, dim, dtype, band, ncu, False, cap)
                assert len(xp.workers(host, cap)) == 1, (src, tgt, dim, dtype, band, cap, host)
                # the host's decision and the device's agree
                assert xp.workers(host, cap) == xp.workers(xp.exact_plan(src, tgt, dim, dtype, band, ncu, True, 65537), cap)


# ---- the GPU cases land where they are named ----------------------------------------------------------------------------
@pytest.mark.parametrize("ncu", CU_COUNTS)
def test_gpu_cases_land_on_their_routes(ncu):
    seen = set()
    for label, args, want in R.planned_routes(ncu):
        assert xp.route(*args) == want, (label, args, want)
        seen.add(want)
    assert seen == {"cells", "pipe", "generic_lds", "generic_global"} | {"reg%d" % r for r in xp.DIMR_LADDER}


@pytest.mark.parametrize("ncu", CU_COUNTS)
def test_handoff_lists_stand_on_the_thresholds(ncu):
    for name, per_cu, src_hi, dtype, below, above in R.HANDOFFS:
        t = per_cu * ncu
        for room in (1, 2):
            p = xp.exact_plan(src_hi, R.TGT_HI, R.DIM, dtype, -1, ncu, True, room * (t + 1))
            hi = p.cells_hi if below == "cells" else p.pipe_hi
            lo = p.pipe_lo if above == "pipe" else p.reg_lo
            assert (hi, lo) == (t, t + 1), (name, p)
        assert R.handoff_lengths(per_cu, ncu) == [t + 1, t, t - 1]
        for length in R.handoff_lengths(per_cu, ncu):
            n, m = R.split(length)
            assert n * m == length and 1 <= n <= 64
    with open(os.path.join(os.path.dirname(HERE), "include", "soundsym_amd.h")) as f:
        assert re.findall(r"#define SSYM_TOPK_MAX (\d+)", f.read()) == [str(R.TOPK_MAX)]
    # the thresholds: 4 and 16 pairs per CU at pipeW = 4, 8 per CU at pipeW = 8
    assert {(c[1], (c[2] + 63) // 64) for c in R.HANDOFFS} == {(4, 1), (4, 4), (16, 4), (8, 8)}
    assert [(c[0], c[1]) for c in R.ALL_PAIRS] == [(4, 0), (4, 1), (4, 0), (4, 1), (16, 0), (16, 1)]
    assert [(c[0], c[1]) for c in R.CHAINS] == [(4, -1), (4, 0), (4, 1), (16, 0), (16, 1)]


def test_width_and_lds_cases_stand_on_their_edges():
    ladder = xp.DIMR_LADDER
    assert {1, 128} <= set(R.DIMS) and all({r, r + 1} <= set(R.DIMS) for r in ladder)
    assert {11, 13, 15, 39, 63, 95} <= set(R.DIMS)
    assert len(R.WIDTH_SRC) == 9 and len(R.WIDTH_TGT) == 7 and R.WIDTH_SRC.count(0) == 1 and R.WIDTH_TGT.count(0) == 1
    assert max(R.WIDTH_SRC) == max(R.WIDTH_TGT) == 140 and min(R.WIDTH_SRC) == 0
    for ncu in CU_COUNTS:
        lens = R.width_long_sources(ncu)
        assert max(lens) == 64 and 0 in lens and len(lens) * len(R.WIDTH_TGT) > 4 * ncu
        for dim in R.LDS_DIMS:
            for dtype in ("f32", "f64"):
                fit = R.reg_fit(dim, dtype, ncu)
                kib = 64 * 1024
                assert xp.reg_lds_bytes(fit, dim, dtype, -1) <= kib < xp.reg_lds_bytes(fit + 1, dim, dtype, -1)
        for dim in R.GENERIC_LDS_DIMS:
            last = xp.longest_target("generic_lds", max(R.LDS_SRC), dim, "f32", -1, ncu, 12, limit=2048)
            assert sum(xp.generic_lds_bytes(last, dim)) <= 64 * 1024 < sum(xp.generic_lds_bytes(last + 1, dim))
    assert R.LONGEST * 16 == xp.BOUND_KIB * 1024
    # bands: the first the cells kernel does not take, pairs on both sides of every band
    assert min(R.WIDE_BANDS) == (xp.PANEL_MAX - 1) // 2 + 1 and 2 * 63 + 1 <= xp.PANEL_MAX < 2 * 64 + 1
    for band in R.WIDE_BANDS:
        apart = np.abs(np.array(R.BAND_SRC)[:, None] - np.array(R.BAND_TGT)[None, :]) > band
        assert apart.sum() >= 6 and (~apart).sum() >= 6
        assert max(R.BAND_TGT) > 64 + 2 * band + 1                  # the window is narrower than the target
    assert 150 <= min(R.BAND_SRC + R.BAND_TGT) and max(R.BAND_SRC + R.BAND_TGT) <= 400
    assert (R.SAME_N * R.SAME_M, R.SAME_SRC, R.SAME_TGT) == (40, 200, 25)
