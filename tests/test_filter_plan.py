"""tests/filter_plan.py against soundsym_amd/csrc/dtw_filter_plan.hpp, and the cases of tests/filter_long_cases.py (what
tests/test_gpu_filter_long_variants.py and tests/test_gpu_filter_band_variants.py run) against the plan (CPU only).

The plan restates the launcher's planner; the GPU cases stand on it.  This file builds tests/cpp/filter_plan_dump.cpp -- a
host program over the planner's header alone -- and holds every launch it prints against the restatement, field by field:
the GPU tests' cases, sets worked out by hand and seeded random sets, at three CU counts, three dims, the default knobs and
each knob alone.  It checks the plan's arithmetic on sets small enough to work out by hand, and asserts for three CU counts
that every case launches the classes it is named for: a case that stops exercising its variant fails here first.
"""
import json
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import filter_plan as P
import filter_long_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "soundsym_amd", "csrc")
CU_COUNTS = [256, 64, 304]
DIMS = [13, 20, 30]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _once(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def _lens(segs):
    return [a.shape[0] for a in segs]


@pytest.fixture(scope="module")
def lengths():
    return {c.name: tuple(_lens(x) for x in C.long_case_data(c)) for c in C.LONG_CASES}


# ---- the planner itself, run --------------------------------------------------------------------------------------------
# One knob at a time: (name, the dump's FilterKnobs fields that differ from the product's, the restatement's arguments).
# "abandon" / "swept": an early-abandoning call and what the context's previous one swept.
KNOB_ORDER = ("pk", "sp", "multipair", "pairblock", "wg", "skip0", "nt8", "one_launch", "long_classes", "prune_nt")
KNOB_DEFAULTS = dict(pk=0, sp=1, multipair=1, pairblock=-1, wg=1, skip0=1, nt8=0, one_launch=0, long_classes=1, prune_nt=0)
KNOBS = [
    ("default", {}, {}),
    ("SSYM_FILTER_PK=1", dict(pk=1), dict(pk=True)),
    ("SSYM_FILTER_SP=0", dict(sp=0), dict(sp=False)),
    ("SSYM_SP_MULTIPAIR=0", dict(multipair=0), dict(mp=False)),
    ("SSYM_SP_MULTIPAIR=2", dict(multipair=2), dict(mp_always=True)),
    ("SSYM_SP_PAIRBLOCK=0", dict(pairblock=0), dict(pair_blocks=False)),
    ("SSYM_SP_PAIRBLOCK=40", dict(pairblock=40), dict(pair_block=40)),
    ("SSYM_FILTER_WG=0", dict(wg=0), dict(wg=False)),
    ("SSYM_FILTER_SKIP0=0", dict(skip0=0), dict(skip0=False)),
    ("SSYM_FILTER_NT8", dict(nt8=1), dict(nt8=True)),
    ("SSYM_FILTER_ONE_LAUNCH", dict(one_launch=1), dict(one_launch=True)),
    ("SSYM_FILTER_LONG_CLASSES=0", dict(long_classes=0), dict(long_classes=False)),
    ("abandon", dict(abandon=1), dict(pruned=True)),
    ("abandon_swept_0.1", dict(abandon=1, swept=0.1), dict(pruned=True, prune_swept=0.1)),
    ("abandon_SSYM_PRUNE_NT=2", dict(abandon=1, prune_nt=2), dict(pruned=True, prune_nt=2)),
    ("abandon_swept_0.1_SSYM_PRUNE_NT=4", dict(abandon=1, swept=0.1, prune_nt=4), dict(pruned=True, prune_swept=0.1, prune_nt=4)),
]
# the sets of the by-hand tests below
HAND_SETS = {
    "hand_70": ([70] * 256, [10]),
    "hand_50_250": ([50] * 38 + [250] * 2, [7, 0, 3]),
    "hand_100_250": ([100] * 38 + [250] * 2, [7, 0, 3]),
    "hand_short_beside": ([10] * 4 + [30] * 2 + [100] * 32 + [250] * 2, [7, 0, 3]),
    "hand_5_40": ([5] * 100 + [40] * 100, [20] * 40),
    "hand_10_x2048": ([10] * 2048, [20] * 256),
    "hand_128": ([128] * 256, [128] * 64),
}


def _cu_counts(name):
    return CU_COUNTS + [8] if name in HAND_SETS else CU_COUNTS      # (8: the by-hand tests' chip)


def _random_sets():
    """200 seeded sets of 1...600 sources of 0...4096 frames and 1...300 targets: ragged, of equal lengths, all empty, one or
    two sources (the rest of the slots padding pairs), and lengths on the tile and pass edges 16 / 32 / 48 / 64 k +- 1."""
    rng = np.random.default_rng(0x5EEDF700)
    sets = {}
    for k in range(200):
        n, m = int(rng.integers(1, 601)), int(rng.integers(1, 301))
        top = int(rng.choice([16, 32, 48, 64, 100, 128, 200, 300, 1000, 4096]))
        kind = k % 8
        if kind == 0:                                   # an odd source count
            n |= 1
        if kind == 1:                                   # equal lengths
            ls = [int(rng.integers(0, top + 1))] * n
        elif kind == 2:                                 # on the edges of tiles and passes
            edges = [q * j + d for q in (16, 32, 48, 64) for j in range(1, 70) for d in (-1, 0, 1) if q * j + d <= top]
            ls = [int(x) for x in rng.choice(edges, n)]
        elif kind == 3 and k % 16 == 3:                 # nothing but empty sources
            ls = [0] * n
        elif kind == 3:                                 # one or two sources: every other pair is padding
            ls = [int(x) for x in rng.integers(0, top + 1, 1 + k // 16 % 2)]
        elif kind == 4:                                 # a few lengths, many sources of each: classes of every size
            ls = [int(x) for x in rng.choice(rng.integers(0, top + 1, 5), n)]
        else:
            ls = [int(x) for x in rng.integers(0, top + 1, n)]
        lt = [int(x) for x in rng.integers(0, int(rng.choice([2, 60, 150, 1000])) + 1, m)]
        sets["random_%03d" % k] = (ls, lt)
    return sets


def _all_sets(lengths):
    import test_gpu_filter_variants as V                # (their case tables; neither module touches the GPU on import)
    import test_gpu_filter_wg as W
    sets = dict(HAND_SETS)
    sets.update({"long_" + name: ls_lt for name, ls_lt in lengths.items()})
    sets.update({"variant_" + c.name: tuple(_lens(x) for x in V.case_data(c)) for c in V.CASES})
    sets.update({"wg_" + name: tuple(_lens(x) for x in make()[2]) for name, make in W.CASES.items()})
    sets.update({"wg_refusal_" + kind: tuple(_lens(x) for x in W._refusal_data(kind))
                 for kind in ("first_pass", "padding_pair", "prune")})
    sets.update(_random_sets())
    return sets


@pytest.fixture(scope="module")
def planner(lengths, tmp_path_factory):
    """The dump program, built and run once over every set x CU count x dim x knob setting: its constants, its launches per
    run id, the sets; the program, its output, the case file and the make command for the tests that run it again."""
    tmp = tmp_path_factory.mktemp("filter_plan")
    make = ["make", "-s", "-C", os.path.join(HERE, "cpp"), "-f", "filter_plan.mk"]
    exe = str(tmp / "filter_plan_dump")
    subprocess.run(make + ["OUT=" + exe], check=True, timeout=300)
    sets = _all_sets(lengths)
    cases = str(tmp / "cases.txt")
    with open(cases, "w") as f:
        for name, (ls, lt) in sets.items():
            f.write("set %d %s %d %s\n" % (len(ls), " ".join(map(str, ls)), len(lt), " ".join(map(str, lt))))
            for dim in DIMS:
                for ncu in _cu_counts(name):
                    for knob, fields, _ in KNOBS:
                        k = dict(KNOB_DEFAULTS, **fields)
                        f.write("run %s|%d|%d|%s %d %d %d %r %s\n" % (name, dim, ncu, knob, dim, ncu, k.get("abandon", 0),
                                                                     k.get("swept", 1.0), " ".join(str(k[x]) for x in KNOB_ORDER)))
    stdout = subprocess.run([exe, cases], check=True, capture_output=True, text=True, timeout=300).stdout
    out = stdout.splitlines()
    runs = {}
    for line in out[1:]:
        r = json.loads(line)
        runs[r["id"]] = r["launches"]
    return SimpleNamespace(consts=json.loads(out[0]), runs=runs, sets=sets, exe=exe, stdout=stdout, cases=cases, make=make)


def _restated(launch):
    """A launch the planner printed as the Launch record of tests/filter_plan.py, and its kernel kind."""
    kind = launch["kind"]
    kernel = {"Mp": "mp", "Sp": "sp", "Pk": "pk"}.get(kind, "generic")
    blocks = {"mp": launch["taskPairs"], "sp": launch["hi"] - launch["lo"]}.get(kernel, 0)
    if blocks:
        assert 1 <= launch["pairBlock"] <= blocks
        blocks = -(-blocks // launch["pairBlock"])
    return P.Launch(launch["nt"], kernel, launch["lo"], launch["hi"], blocks, launch["cells"], launch["passes"], launch["origin"],
                    kind == "GenericSkip0", launch["grid"], launch["taskChunk"], kind == "Wg"), kind


def _kind(x, pruned):
    return {"mp": "Mp", "sp": "Sp", "pk": "Pk"}.get(x.kernel) or \
        ("GenericPrune" if pruned else "Wg" if x.wg else "GenericSkip0" if x.skip else "Generic")


def test_the_planner_has_the_thresholds_the_plan_restates(planner):
    # the unbanded planner's, as the dump program prints them (the rules that use them: the test below, by running them)
    assert planner.consts == dict(kMaxClasses=P.MAX_CLASSES, kSmallClass=P.SMALL_CLASS, kSpRowBlock=P.ROW_BLOCK, kSpRing=P.RING,
                                  kFilterRecHalfs=P.REC_HALFS, kFilterWavesPerBlock=P.WAVES_PER_BLOCK,
                                  kFilterMaxFrames=P.MAX_FRAMES, SSYM_SP_OCC_NT2=P.SP_OCC_NT2)
    # the banded launcher's, read out of the source
    _once(r"return 2 \* ctx->band \+ 1 > 6 \* 16 \|\| band_lds_bytes\(ctx->band, src, tgt\) > 160 \* 1024 - 64;",
          _read("dtw_filter.hip"))
    band = _read("dtw_band_kernel.hpp")
    assert int(_once(r"constexpr int kBandImagePad = (\d+);", band)) == 8
    assert int(_once(r"constexpr int kBandTgtQuantum = (\d+);", band)) == 256


def test_the_planner_plans_what_the_plan_restates(planner):
    """Every field both sides know -- kernel kind, tiles, pair range, passes, row origin, SKIP0, pair blocks, cells, grid,
    task chunk, the wg kernel's gate -- of every launch of every run; and the counter sets: one per launch, in order."""
    runs, sets = planner.runs, planner.sets
    assert len(runs) == sum(len(_cu_counts(name)) for name in sets) * len(DIMS) * len(KNOBS)
    kinds = set()
    for name, (ls, lt) in sets.items():
        ls, lt = sorted(ls), sorted(lt)                  # (the restatement sorts them anyway: sorted once, that is quick)
        for dim in DIMS:
            for ncu in _cu_counts(name):
                for knob, _, kw in KNOBS:
                    rid = "%s|%d|%d|%s" % (name, dim, ncu, knob)
                    got = [_restated(x) for x in runs[rid]]
                    want, _ = P.filter_plan(ls, lt, dim, ncu, **kw)
                    assert [g for g, _ in got] == want, rid
                    assert [k for _, k in got] == [_kind(x, kw.get("pruned", False)) for x in want], rid
                    sets_used = [x["ctrSet"] for x in runs[rid]]
                    assert sets_used == sorted(set(sets_used)) and all(0 <= s < P.MAX_CLASSES for s in sets_used), rid
                    base = max(8, ncu * 2 // 8 * 8)             # two workgroups per CU, occ / 2 times as many at most
                    assert all(x["occ"] in (1, 2, 3) and x["grid"] % 8 == 0 and 0 < x["grid"] <= base // 2 * x["occ"]
                               for x in runs[rid]), rid
                    kinds |= {(k, g.nt) for g, k in got}
    # every kernel kind at every tile count the launcher has it for
    assert kinds == {("Mp", 1), ("Sp", 1), ("Sp", 2), ("Sp", 3), ("Generic", 1), ("Generic", 2), ("Generic", 3), ("Generic", 4),
                     ("Generic", 8), ("GenericSkip0", 3), ("GenericSkip0", 4), ("GenericPrune", 1), ("GenericPrune", 2),
                     ("GenericPrune", 3), ("GenericPrune", 4), ("Wg", 4), ("Pk", 4)}, sorted(kinds)


def test_the_planner_stops_where_the_filter_does(planner, tmp_path):
    cases = tmp_path / "beyond.txt"
    cases.write_text("".join("set 2 5 %d 1 9\nrun %d 13 256 0 1.0 0 1 1 -1 1 1 0 0 1 0\n" % (f, f)
                             for f in (P.MAX_FRAMES, P.MAX_FRAMES + 1)))
    out = subprocess.run([planner.exe, str(cases)], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    within, beyond = (json.loads(x) for x in out[1:])
    assert [(x["nt"], x["passes"]) for x in within["launches"]] == [(4, 64)] and beyond["launches"] is None
    assert P.filter_shape(P.MAX_FRAMES) == (4, 64) and P.filter_shape(P.MAX_FRAMES + 1) == (0, 0)


def test_the_planner_is_clean_under_the_sanitizers(planner, tmp_path):
    """The dump program once more with -fsanitize=address,undefined, as the stand-alone program it is, over the same cases:
    the same output, nothing reported."""
    exe = str(tmp_path / "filter_plan_dump_san")
    subprocess.run(planner.make + ["OUT=" + exe, "EXTRA=-fsanitize=address,undefined -fno-sanitize-recover=all"], check=True,
                   timeout=300)
    r = subprocess.run([exe, planner.cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout == planner.stdout


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
    # into its first pass: the first tile is empty, 80 rows of 96; ten columns.
    # Grid: 128 tasks (one target group) are 32 workgroups of four waves, fewer than the 512 of 256 CUs.  Chunk: a task of
    # 96 rows x 10 mean columns would be grabbed 8192 // 960 = 8 at a time, but 128 tasks // (32 x 4 waves x 16 grabs) = 0: 1
    plan, groups = P.filter_plan(*HAND_SETS["hand_70"], 13, 256)
    assert groups == 1 and plan == [P.Launch(3, "generic", 0, 128, 0, 128 * 80 * 10, 2, 32, True, 32, 1, False)]
    plan, _ = P.filter_plan(*HAND_SETS["hand_70"], 13, 256, skip0=False)
    assert plan == [P.Launch(3, "generic", 0, 128, 0, 128 * 96 * 10, 2, 32, False, 32, 1, False)]   # (three tiles: no wg kernel)
    # the set's own shape: four tiles from row 0, 128 whole pairs, pass 0 (rows 0...63) holds rows 58... of every source: wg
    for kw in (dict(long_classes=False), dict(one_launch=True)):
        plan, _ = P.filter_plan(*HAND_SETS["hand_70"], 13, 256, **kw)
        assert plan == [P.Launch(4, "generic", 0, 128, 0, 128 * 128 * 10, 2, 0, False, 32, 1, True)]
        plan, _ = P.filter_plan(*HAND_SETS["hand_70"], 13, 256, wg=False, **kw)
        assert plan == [P.Launch(4, "generic", 0, 128, 0, 128 * 128 * 10, 2, 0, False, 32, 1, False)]
    # on a chip of 8 CUs (16 workgroups) the grid is the chip's
    plan, _ = P.filter_plan(*HAND_SETS["hand_70"], 13, 8)
    assert plan == [P.Launch(3, "generic", 0, 128, 0, 128 * 80 * 10, 2, 32, True, 16, 1, False)]


def test_plan_by_hand_grid_chunk_and_pair_blocks_of_the_short_kernels():
    # 2048 sources of 10 frames (1024 pairs, one 16-row tile from row 0) x 256 targets of 20 (8 groups) on 8 CUs: 16
    # workgroups at two per CU.  A 10-frame source starts at row 6: one row block of 4 skipped, 12 rows; 8 x 20 columns.
    src, tgt = HAND_SETS["hand_10_x2048"]
    cells = 1024 * 12 * 160
    # multi-pair tasks, three pairs each with two operand planes: 342 per group, 2736 tasks >= 16 x 4 waves; two workgroups
    # per CU: 16.  Chunk: 48 rows x 20 columns, 8192 // 960 = 8 at a time, but 2736 // (16 x 4 x 16) = 2 keeps 16 grabs per
    # wave.  Pair block: 1 MiB // (3 x 2 sources x 16 rows x 96 bytes) = 113 tasks' pairs: 342 in 4 blocks
    plan, _ = P.filter_plan(src, tgt, 13, 8)
    assert plan == [P.Launch(1, "mp", 0, 1024, 4, cells, 1, 0, False, 16, 2, False)]
    # with three planes two pairs each: 512 per group, 4096 tasks // 1024 = 4 of 8192 // (32 x 20) = 12 -> 8; blocks of
    # 1 MiB // (2 x 2 x 16 x 96) = 170: 512 in 4; every pair's 12 rows
    plan, _ = P.filter_plan(src, tgt, 30, 8)
    assert plan == [P.Launch(1, "mp", 0, 1024, 4, cells, 1, 0, False, 16, 4, False)]
    # one pair per wave (SSYM_SP_MULTIPAIR=0): 8192 tasks, three workgroups per CU: 24; 8192 // (16 x 20) = 25 -> 8 at a
    # time, 8192 // (24 x 64) = 5; blocks of 1 MiB // (2 x 16 x 96) = 341 pairs: 1024 in 4
    plan, _ = P.filter_plan(src, tgt, 13, 8, mp=False)
    assert plan == [P.Launch(1, "sp", 0, 1024, 4, cells, 1, 0, False, 24, 5, False)]
    # ... with three planes the sp kernel runs two workgroups per CU: 16 -- the chunk stays the one worked out for 24
    plan, _ = P.filter_plan(src, tgt, 30, 8, mp=False)
    assert plan == [P.Launch(1, "sp", 0, 1024, 4, cells, 1, 0, False, 16, 5, False)]
    plan, _ = P.filter_plan(src, tgt, 13, 8, mp=False, pair_blocks=False)
    assert plan == [P.Launch(1, "sp", 0, 1024, 1, cells, 1, 0, False, 24, 5, False)]
    plan, _ = P.filter_plan(src, tgt, 13, 8, mp=False, pair_block=40)
    assert plan == [P.Launch(1, "sp", 0, 1024, 26, cells, 1, 0, False, 24, 5, False)]
    # dtw_filter_kernel (SSYM_FILTER_SP=0): all 16 rows of every pair, no minimum of columns; grid and chunk as above
    plan, _ = P.filter_plan(src, tgt, 13, 8, sp=False)
    assert plan == [P.Launch(1, "generic", 0, 1024, 0, 1024 * 16 * 160, 1, 0, False, 24, 5, False)]
    # few tasks: 100 pairs x 2 groups; 34 x 2 = 68 multi-pair tasks would not fill 256 CUs (2048 waves): sp, 200 tasks in
    # 50 -> 56 workgroups
    plan, _ = P.filter_plan([10] * 200, [20] * 40, 13, 256)
    assert [(x.kernel, x.grid, x.chunk, x.blocks) for x in plan] == [("sp", 56, 1, 1)]
    plan, _ = P.filter_plan([10] * 200, [20] * 40, 13, 256, mp_always=True)      # SSYM_SP_MULTIPAIR=2: 68 tasks, 17 -> 24 workgroups
    assert [(x.kernel, x.grid, x.chunk, x.blocks) for x in plan] == [("mp", 24, 1, 1)]


def test_plan_by_hand_the_wg_kernel_and_an_abandoning_call():
    # 256 sources x 64 targets of 128 frames on 8 CUs: 128 pairs x 2 groups = 256 tasks on 16 workgroups; a task of 128 rows
    # x 128 columns is grabbed alone.  Whole blocks of four pairs, none padding, every source from row 0: the wg kernel
    src, tgt = HAND_SETS["hand_128"]
    plan, _ = P.filter_plan(src, tgt, 13, 8)
    assert plan == [P.Launch(4, "generic", 0, 128, 0, 128 * 128 * 256, 2, 0, False, 16, 1, True)]
    # the gate: 254 and 248 sources (a padding pair and four of them ride with the class) and 255 (an odd count: the last
    # real pair holds one source) keep dtw_filter_kernel
    for n, pairs in ((254, 128), (255, 128), (248, 128)):
        plan, _ = P.filter_plan(src[:n], tgt, 13, 8)
        assert [(x.lo, x.hi, x.wg) for x in plan] == [(0, pairs, False)], n
    # SSYM_FILTER_NT8: the 128 rows in one pass of eight tiles, one workgroup per CU: 8
    plan, _ = P.filter_plan(src, tgt, 13, 8, nt8=True)
    assert plan == [P.Launch(8, "generic", 0, 128, 0, 128 * 128 * 256, 1, 0, False, 8, 1, False)]
    plan, _ = P.filter_plan(src, tgt, 13, 8, pk=True)
    assert plan == [P.Launch(4, "pk", 0, 128, 0, 0, 2, 0, False, 16, 1, False)]
    # early abandoning: dtw_filter_kernel's PRUNE instantiation, its cells counted on the device (0 here); passes of 64 rows
    # after a call that swept a quarter of its cells or more (and on the first), of 32 below; SSYM_PRUNE_NT pins either
    for kw in (dict(), dict(prune_swept=0.25), dict(prune_swept=0.1, prune_nt=4)):
        plan, _ = P.filter_plan(src, tgt, 13, 8, pruned=True, **kw)
        assert plan == [P.Launch(4, "generic", 0, 128, 0, 0, 2, 0, False, 16, 1, False)], kw
    for kw in (dict(prune_swept=0.1), dict(prune_nt=2), dict(prune_swept=0.24, prune_nt=3)):
        plan, _ = P.filter_plan(src, tgt, 13, 8, pruned=True, **kw)
        assert plan == [P.Launch(2, "generic", 0, 128, 0, 0, 4, 0, False, 16, 1, False)], kw
    # short sources of an abandoning call: their classes on dtw_filter_kernel too, whatever the pass height
    plan, _ = P.filter_plan(*HAND_SETS["hand_5_40"], 13, 256, pruned=True, prune_swept=0.1)
    assert [(x.kernel, x.nt, x.passes, x.origin, x.cells, x.lo, x.hi) for x in plan] == \
        [("generic", 1, 1, 32, 0, 0, 50), ("generic", 3, 1, 0, 0, 50, 112)]


def test_plan_by_hand_leading_passes_and_padding_pairs():
    # 40 sources: 38 of 50 frames, two of 250 (a 256-row slot): runs (4, 1) and (4, 4); 19 pairs join the last class, the
    # 12 padding pairs ride with it.  Rows: a 50-frame pair starts at row 206 = pass 3, 14 rows in (no skip): 64; the
    # 250-frame pair at row 6: 256; a padding pair at row 256: its last pass, 64 rows in: 64 - 16
    plan, _ = P.filter_plan(*HAND_SETS["hand_50_250"], 13, 256)
    assert P.plan_classes(plan) == (("generic", 4, 4, False),)          # 8 x 0 skipping real pairs
    assert plan[0].cells == (19 * 64 + 256 + 12 * 64) * 7 and (plan[0].lo, plan[0].hi, plan[0].origin) == (0, 32, 0)
    # 32 tasks: 8 workgroups, one task at a time; padding pairs in the class: no wg kernel
    assert (plan[0].grid, plan[0].chunk, plan[0].wg) == (8, 1, False)
    # the same with 100-frame sources in place of 50: rows 156 = pass 2, 28 rows in: they skip, and so do the padding pairs
    plan, _ = P.filter_plan(*HAND_SETS["hand_100_250"], 13, 256)
    assert P.plan_classes(plan) == (("generic", 4, 4, True),)
    assert plan[0].cells == (19 * (128 - 16) + 256 + 12 * (64 - 16)) * 7
    # short sources beside them: their own single-pass classes on the last rows of the slot
    plan, _ = P.filter_plan(*HAND_SETS["hand_short_beside"], 13, 256)
    assert [(x.kernel, x.nt, x.lo, x.hi, x.origin) for x in plan] == \
        [("sp", 1, 0, 2, 240), ("sp", 2, 2, 3, 224), ("generic", 4, 3, 32, 0)]
    plan, _ = P.filter_plan(*HAND_SETS["hand_short_beside"], 13, 256, one_launch=True)
    assert [(x.kernel, x.nt, x.passes, x.lo, x.hi, x.origin) for x in plan] == [("generic", 4, 4, 0, 32, 0)]


def test_plan_up_to_48_frames_is_the_single_pass_plan():
    plan, _ = P.filter_plan(*HAND_SETS["hand_5_40"], 40, 256)
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
