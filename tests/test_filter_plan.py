"""tests/filter_plan.py against soundsym_amd/csrc/dtw_filter.hip, and the cases of tests/filter_long_cases.py (what
tests/test_gpu_filter_long_variants.py and tests/test_gpu_filter_band_variants.py run) against the plan (CPU only).

The plan restates the launcher's classes; the GPU cases stand on them.  This file reads the planner's thresholds out of
the source, checks the plan's arithmetic on sets small enough to work out by hand, and asserts for three CU counts that
every case launches the classes it is named for: a case that stops exercising its variant fails here first.
"""
import os
import re

import numpy as np
import pytest

import filter_plan as P
import filter_long_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "soundsym_amd", "csrc")
CU_COUNTS = [256, 64, 304]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


SRC = _read("dtw_filter.hip")
LAUNCHER = SRC[SRC.index("int32_t launch_dtw_filter("):]


def _once(pattern, text=LAUNCHER):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def _lens(segs):
    return [a.shape[0] for a in segs]


@pytest.fixture(scope="module")
def lengths():
    return {c.name: tuple(_lens(x) for x in C.long_case_data(c)) for c in C.LONG_CASES}


# ---- the thresholds the plan restates --------------------------------------------------------------------------------
def test_the_planner_has_the_thresholds_the_plan_restates():
    assert int(_once(r"constexpr int kMaxClasses = (\d+);")) == P.MAX_CLASSES
    _once(r"if \(nCls == kMaxClasses - 3 && sp < nPairs\)")
    _once(r"cls\[nCls - 1\] = LongClass\{4, shape\.rb, cls\[nCls - 1\]\.lo, nPairs\};")
    assert int(_once(r"if \(cls\[c\]\.hi - cls\[c\]\.lo < (\d+)\)")) == P.SMALL_CLASS
    _once(r"if \(48 \* p3 < 64 \* p4\) \{ nt = 3; passes = p3; \} else \{ nt = 4; passes = p4; \}")
    _once(r"skipping \+= \(rowsCls - \(int\)pairLen\(sp\)\) % \(16 \* cls\[c\]\.nt\) >= 17;")
    _once(r"skipTile = skipOn && 8 \* skipping >= cls\[c\]\.hi - cls\[c\]\.lo && skipping > 0;")
    _once(r"end == nRealPairs \? nPairs : end")
    _once(r"\} else if \(abandon \|\| oneLong \|\| oneLaunch\) \{")
    _once(r"if \(skipTile && r0min - \(rowOrigin \+ firstPass \* passRows\) >= 17\)", SRC)
    _once(r"const int firstPass = std::min\(std::max\(r0min - rowOrigin, 0\) / passRows, nPasses - 1\);", SRC)
    internal = _read("ssym_internal.hpp")
    assert int(_once(r"if \(max_frames <= (\d+)\) return FilterShape\{4, \(max_frames \+ 63\) / 64\};", internal)) == P.MAX_FRAMES
    _once(r"return 2 \* ctx->band \+ 1 > 6 \* 16 \|\| band_lds_bytes\(ctx->band, src, tgt\) > 160 \* 1024 - 64;", SRC)
    band = _read("dtw_band_kernel.hpp")
    assert int(_once(r"constexpr int kBandImagePad = (\d+);", band)) == 8
    assert int(_once(r"constexpr int kBandTgtQuantum = (\d+);", band)) == 256


def test_best_shape_pads_least():
    want = {1: (3, 1), 48: (3, 1), 49: (4, 1), 64: (4, 1), 65: (3, 2), 96: (3, 2), 97: (4, 2), 128: (4, 2), 129: (3, 3),
            144: (3, 3), 145: (4, 3), 192: (4, 3), 193: (3, 5), 240: (3, 5), 241: (4, 4), 256: (4, 4), 257: (3, 6),
            288: (3, 6), 289: (4, 5), 4096: (4, 64)}
    for f, shape in want.items():
        assert P.best_shape(f) == shape, f
        nt, passes = shape
        assert 16 * nt * passes >= f and 16 * nt * passes == min(48 * -(-f // 48), 64 * -(-f // 64)), f


# ---- the plan's arithmetic by hand -----------------------------------------------------------------------------------
def test_plan_by_hand_one_class_of_two_48_row_passes():
    # 256 sources of 70 frames: 128 pairs in (3, 2), the last 96 of a 128-row slot; a source starts at row 58, 26 rows
    # into its first pass: the first tile is empty, 80 rows of 96; ten columns
    plan, groups = P.filter_plan([70] * 256, [10], 13, 256)
    assert groups == 1 and plan == [P.Launch(3, "generic", 0, 128, 0, 128 * 80 * 10, 2, 32, True)]
    plan, _ = P.filter_plan([70] * 256, [10], 13, 256, skip0=False)
    assert plan == [P.Launch(3, "generic", 0, 128, 0, 128 * 96 * 10, 2, 32, False)]
    for kw in (dict(long_classes=False), dict(one_launch=True)):
        plan, _ = P.filter_plan([70] * 256, [10], 13, 256, **kw)
        assert plan == [P.Launch(4, "generic", 0, 128, 0, 128 * 128 * 10, 2, 0, False)]


def test_plan_by_hand_leading_passes_and_padding_pairs():
    # 40 sources: 38 of 50 frames, two of 250 (a 256-row slot): runs (4, 1) and (4, 4); 19 pairs join the last class, the
    # 12 padding pairs ride with it.  Rows: a 50-frame pair starts at row 206 = pass 3, 14 rows in (no skip): 64; the
    # 250-frame pair at row 6: 256; a padding pair at row 256: its last pass, 64 rows in: 64 - 16
    plan, _ = P.filter_plan([50] * 38 + [250] * 2, [7, 0, 3], 13, 256)
    assert P.plan_classes(plan) == (("generic", 4, 4, False),)          # 8 x 0 skipping real pairs
    assert plan[0].cells == (19 * 64 + 256 + 12 * 64) * 7 and (plan[0].lo, plan[0].hi, plan[0].origin) == (0, 32, 0)
    # the same with 100-frame sources in place of 50: rows 156 = pass 2, 28 rows in: they skip, and so do the padding pairs
    plan, _ = P.filter_plan([100] * 38 + [250] * 2, [7, 0, 3], 13, 256)
    assert P.plan_classes(plan) == (("generic", 4, 4, True),)
    assert plan[0].cells == (19 * (128 - 16) + 256 + 12 * (64 - 16)) * 7
    # short sources beside them: their own single-pass classes on the last rows of the slot
    plan, _ = P.filter_plan([10] * 4 + [30] * 2 + [100] * 32 + [250] * 2, [7, 0, 3], 13, 256)
    assert [(x.kernel, x.nt, x.lo, x.hi, x.origin) for x in plan] == \
        [("sp", 1, 0, 2, 240), ("sp", 2, 2, 3, 224), ("generic", 4, 3, 32, 0)]
    plan, _ = P.filter_plan([10] * 4 + [30] * 2 + [100] * 32 + [250] * 2, [7, 0, 3], 13, 256, one_launch=True)
    assert [(x.kernel, x.nt, x.passes, x.lo, x.hi, x.origin) for x in plan] == [("generic", 4, 4, 0, 32, 0)]


def test_plan_up_to_48_frames_is_the_single_pass_plan():
    plan, _ = P.filter_plan([5] * 100 + [40] * 100, [20] * 40, 40, 256)
    assert [(x.kernel, x.nt, x.passes, x.origin) for x in plan] == [("sp", 1, 1, 32), ("generic", 3, 1, 0)]
    with pytest.raises(AssertionError):
        P.filter_plan([4097], [20], 13, 256)


# ---- the GPU cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncu", CU_COUNTS)
@pytest.mark.parametrize("case", C.LONG_CASES, ids=[c.name for c in C.LONG_CASES])
def test_case_launches_the_classes_it_names(lengths, case, ncu):
    ls, lt = lengths[case.name]
    assert len(lt) == case.m and len(lt) % 32 != 0
    plan, groups = P.filter_plan(ls, lt, case.dim, ncu)
    assert P.plan_classes(plan) == case.classes, plan
    assert groups == -(-case.m // 32)
    assert plan[-1].hi == -(-len(ls) // 32) * 16 and all(a.hi == b.lo for a, b in zip(plan, plan[1:]))
    # an alternative plan with other cells (what the GPU test's A/B stands on): SKIP0 off where a class skips, the set's own
    # shape for every long pair otherwise -- except where the default is already that one launch
    alt, _ = P.filter_plan(ls, lt, case.dim, ncu, skip0=False) if any(x.skip for x in plan) else \
        P.filter_plan(ls, lt, case.dim, ncu, long_classes=False)
    if case.name == "equal_128":
        assert alt == plan == P.filter_plan(ls, lt, case.dim, ncu, one_launch=True)[0]
    else:
        assert P.plan_cells(alt) > P.plan_cells(plan)


def test_cases_stand_on_the_edges_they_name(lengths):
    plans = {c.name: P.filter_plan(*lengths[c.name], c.dim, 256)[0] for c in C.LONG_CASES}
    assert [(x.origin, x.hi - x.lo) for x in plans["nt3x2_nt4x2"]] == [(32, 128), (0, 128)]
    # (3, 2) at row origin 96 of a 192-row slot: not a multiple of 64; classes of exactly 128 pairs do not join
    assert [(x.origin, x.hi - x.lo) for x in plans["nt4x1_nt3x2_nt3x3"]] == [(128, 128), (96, 128), (48, 128)]
    # 50 real pairs of (3, 2) joined the class behind them; 8 padding pairs ride along
    assert (plans["small_class_joins"][0].lo, plans["small_class_joins"][0].hi) == (0, 208)
    assert sum(f <= 96 for f in lengths["small_class_joins"][0]) == 100
    # the last class is smaller than 128 pairs and keeps its shape
    last = plans["short_and_long"][-1]
    assert 0 < last.hi - last.lo < P.SMALL_CLASS and (last.nt, last.passes) == (3, 5)
    assert len(plans["short_and_long"]) == 6
    for name in C.SAME_LENGTHS:
        assert sorted(lengths[name][0]) == sorted(lengths[C.SAME_LENGTHS[0]][0])
    assert [P.filter_ku(c.dim) for c in C.LONG_CASES if c.name in C.SAME_LENGTHS] == [2, 3, 2]
    assert sorted(set(lengths["many_passes"][0])) == [49, 64, 100, 700, 1000, 2049, 3000, 4096]
    assert set(lengths["equal_128"][0]) == {128} and set(lengths["equal_128"][1]) == {128}


def test_counter_cap_cases_run_out_of_counter_sets(lengths, monkeypatch):
    for name, runs in (("counter_cap", 9), ("counter_cap_288", 8)):
        ls, lt = lengths[name]
        pair_len = sorted(ls)[1::2]
        shapes = [P.best_shape(f) for f in pair_len]
        assert len(set(shapes)) == runs and shapes == sorted(shapes, key=lambda s: 16 * s[0] * s[1]), name
        assert len(set(shapes[:-1])) >= P.MAX_CLASSES - 3                  # the seventh run is not the last pair's
    # with counter sets to spare the 288-frame set would end in its last run's own shape: six passes of 48 rows
    ls, lt = lengths["counter_cap_288"]
    capped, _ = P.filter_plan(ls, lt, 13, 256)
    monkeypatch.setattr(P, "MAX_CLASSES", 100)
    free, _ = P.filter_plan(ls, lt, 13, 256)
    assert P.plan_classes(free) == (("generic", 3, 6, True),) and P.plan_classes(capped) == (("generic", 4, 5, True),)
    assert P.plan_cells(free) != P.plan_cells(capped)


def test_targets_cover_the_hand_off_row_edges(lengths):
    residues = set()
    for c in C.LONG_CASES:
        lt = sorted(lengths[c.name][1])
        assert lt[-1] <= C.TGT_MAX
        longest = [max(lt[g:g + 32]) for g in range(0, len(lt), 32)]
        residues |= {f % 4 for f in longest}
        if c.m == 70:
            assert longest[0] == 1 and lt[:3] == [0, 0, 0]              # a group of 1-frame targets, a few empty ones
        elif not c.grid:
            assert lt[:2] == [0, 0]
    assert residues == {0, 1, 2, 3}


def test_planted_targets_are_about_half_and_of_another_length():
    case = C.LONG_CASES[0]
    src, tgt = C.long_case_data(case)
    fill_src, fill_tgt = C.long_case_data(case, values_seed=0x5EEDF0FF)
    assert _lens(fill_src) == _lens(src) and _lens(fill_tgt) == _lens(tgt)
    assert not any(np.array_equal(a, b) for a, b in zip(src, fill_src) if a.size)
    near = 0
    for b in tgt:
        if b.shape[0] >= 60:
            near += any(abs(a.shape[0] - b.shape[0]) <= 2 and
                        np.abs(a[0] - b[0]).max() < 0.5 and np.abs(a[-1] - b[-1]).max() < 0.5 for a in src)
    assert 28 <= near <= 36, near


# ---- the banded cases ------------------------------------------------------------------------------------------------
def test_band_radii_reach_every_instantiation():
    got = {C.band_instance(r) for r in C.BAND_RADII}
    assert got == {(ntb, lastn, 8 if ntb <= 5 else 4) for ntb in range(1, 7) for lastn in (1, 16)}
    assert {r for r in C.BAND_RADII if C.band_instance(r)[1] == 1} == {0, 8, 16, 24, 32, 40}
    assert C.band_instance(47) == (6, 16, 4) and C.band_instance(40) == (6, 1, 4) and C.band_instance(48)[0] == 7
    combos = {(C.band_instance(c.r)[:2], P.filter_ku(c.dim), c.squared) for c in C.BAND_CASES}
    assert {k for _, k, _ in combos} == {2, 3} and {s for _, _, s in combos} == {False, True}


def test_band_data_shapes():
    for r in (0, 8, 47):
        src, tgt = C.band_data(r, 13)
        ls, lt = _lens(src), _lens(tgt)
        assert len(ls) == C.BAND_N and len(lt) == C.BAND_M and -(-len(lt) // 256) * 256 == 512
        assert min(ls) == 0 and max(ls) == C.BAND_MAX and sorted(lt)[:3] == [0, 0, 0] and max(lt) == C.BAND_MAX
        assert np.array_equal(src[20], src[21])
        assert C.band_lds_bytes(r, max(ls), max(lt)) <= C.BAND_LDS_LIMIT
        reach = (np.abs(np.array(ls)[:, None] - np.array(lt)[None, :]) <= r) & (np.array(ls)[:, None] > 0) & (np.array(lt)[None, :] > 0)
        assert reach.any(axis=0).sum() >= C.BAND_M // 3                   # the planted third, at least, has a finite pair
        assert (~reach).any()
    src, tgt = C.band_data(8, 13, long_source=900)
    assert max(_lens(src)) == 900 and C.band_lds_bytes(8, 900, max(_lens(tgt))) > C.BAND_LDS_LIMIT
    assert C.band_lds_bytes(8, 820, 120) <= C.BAND_LDS_LIMIT               # (the limit lies between)
