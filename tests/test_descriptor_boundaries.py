"""The front-end kernels' internal boundaries, read from csrc/mfcc.hip, csrc/pitch.hip and csrc/sequence.hip (CPU only).

tests/test_gpu_mfcc_shapes.py, test_gpu_sequence_shapes.py and test_gpu_pitch_shapes.py pick their cases to fall on both
sides of every branch of the kernels: grid-stride loops that take a second item, filter and coefficient counts against
the 256 threads and the kMaxFilters LDS array, the pitch kernel's lag loops against 256 threads and the parity of its lag
count.  This file reads the constants that place those branches from the sources, takes the MI355X's 256 CUs, and checks
that the case lists still straddle each of them, so that a moved constant moves the case lists with it.
"""
import os
import re

import pitch_ref as ref
from soundsym_amd.engine import pitch_lags
import test_gpu_mfcc_shapes as M
import test_gpu_pitch_shapes as P
import test_gpu_sequence_shapes as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "soundsym_amd", "csrc")
NUM_CUS = 256                       # MI355X
THREADS = 256                       # every kernel here runs 256-thread workgroups


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _defines():
    with open(os.path.join(ROOT, "include", "soundsym_amd.h")) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (SSYM_\w+) (\d+)\b", f.read())}


def _constants(text, names):
    """constexpr int NAME = <integer expression of integers, header macros and earlier names>."""
    env = dict(_defines())
    out = {}
    for name in names:
        m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, text)
        assert m, name
        expr = m.group(1).strip()
        for k, v in sorted(list(env.items()) + list(out.items()), key=lambda kv: -len(kv[0])):
            expr = re.sub(r"\b%s\b" % k, str(v), expr)
        assert re.fullmatch(r"[0-9\s()*/+-]+", expr), (name, expr)
        out[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}))
    return out


def _grid_factors(text):
    return [int(v) for v in re.findall(r"num_cus \* (\d+)", text)]


MF = _constants(_read("mfcc.hip"), ("kBin", "kHop", "kMaxFilters"))
PI = _constants(_read("pitch.hip"), ("kW", "kH", "kPW", "kPH", "kThreads", "kChunk", "kMaxTau"))
SQ = _constants(_read("sequence.hip"), ("kThreads",))
MFCC_GRID = _grid_factors(_read("mfcc.hip"))
PITCH_GRID = _grid_factors(_read("pitch.hip"))
SEQ_GRID = _grid_factors(_read("sequence.hip"))


def test_constants_are_read():
    assert MF == {"kBin": 1024, "kHop": 256, "kMaxFilters": 130}
    assert (PI["kW"], PI["kH"], PI["kChunk"], PI["kMaxTau"]) == (2048, 1024, 8192, 682)
    assert PI["kThreads"] == SQ["kThreads"] == THREADS
    # one factor per launch: mfcc_kernel and mfcc_batch_kernel; the one cap of the peak and pitch kernels; the means
    assert MFCC_GRID == [M.GRID_FACTOR] * 2 and PITCH_GRID == [P.CAP_FACTOR] and len(SEQ_GRID) == 1
    assert (M.BIN, M.HOP) == (MF["kBin"], MF["kHop"]) and (P.W, P.H, P.CHUNK) == (PI["kW"], PI["kH"], PI["kChunk"])


# ---- MFCC -------------------------------------------------------------------------------------------------------------
def test_mfcc_coefficient_counts_straddle_the_limits():
    nfs = {2 * nc + 2 for nc in M.NCS}
    assert min(M.NCS) == 1 and max(M.NCS) == 64 and max(nfs) == MF["kMaxFilters"]
    # filters: up to 128 and past it (the edge of a min(nf, 128)); coefficients: around a 32-lane half wave
    assert 128 in nfs and MF["kMaxFilters"] > 128 and {31, 32, 33} <= set(M.NCS) and {7, 8} <= set(M.NCS)
    assert all(nf <= THREADS for nf in nfs)          # one filter per thread: a single pass in mfcc_frame
    bands_nc = {b[2] for b in M.BANDS} | {64}
    assert 64 in bands_nc


def test_mfcc_bands_reach_every_edge():
    labels = {b[5] for b in M.BANDS}
    assert labels == {"none", "some", "all"}
    for label, rate, nc, f_lo, f_hi, empty in M.BANDS:
        _, lo, hi = M.filterbank(rate, nc, f_lo, f_hi)
        none = hi == 0
        assert {"none": not none.any(), "some": none.any() and not none.all(), "all": none.all()}[empty], label
        assert f_lo < min(f_hi, rate / 2)             # every band is one the library accepts
    assert any(b[3] == 0.0 for b in M.BANDS)
    assert any(b[4] == b[1] / 2 for b in M.BANDS) and any(b[4] > b[1] / 2 for b in M.BANDS)
    assert any(b[2] == 64 and b[5] == "some" for b in M.BANDS)
    assert set(M.RATES) >= {8000.0, 16000.0, 22050.0, 44100.0, 48000.0, 96000.0}


def test_mfcc_grid_is_straddled():
    cap = NUM_CUS * MFCC_GRID[0]
    frames = M.grid_frames(NUM_CUS)
    assert {cap - 1, cap, cap + 1} <= set(frames) and max(frames) > 2 * cap
    counts = [M.Engine.mfcc_num_frames(n, True) for n in M.batch_lengths()]
    assert sum(counts) > 2 * cap
    # the batch's binary search meets runs of equal frame offsets (empty sounds, many in a row)
    assert counts.count(0) > 1000 and any(counts[i] == counts[i + 1] == 0 for i in range(len(counts) - 1))
    assert {1023, 1024, 1025, 1279, 1280} <= set(M.BATCH_LENGTHS)
    # ... and its out_mean runs the means kernel past its cap
    assert M.BATCH_SOUNDS * M.BATCH_NC > NUM_CUS * SEQ_GRID[0] * SQ["kThreads"]


# ---- sequence ---------------------------------------------------------------------------------------------------------
def test_sequence_sizes_straddle_the_grids():
    assert S.DIMS == list(range(1, 65))
    means_cap = NUM_CUS * SEQ_GRID[0] * SQ["kThreads"]
    assert S.MANY_SOUNDS * S.MANY_DIM > means_cap
    pairs = S.MANY_SOUNDS - 1
    assert pairs > SQ["kThreads"] and pairs % SQ["kThreads"] != 0
    assert S.LONG_FRAMES >= 100000


# ---- pitch ------------------------------------------------------------------------------------------------------------
def _lag_passes(lo, hi):
    """(nR, passes of the voiced loop k <= hi - lo, passes of the two-lag loop q <= (nR + 1) / 2) over 256 threads."""
    nR = hi - lo + 3
    return nR, (hi - lo) // THREADS + 1, ((nR + 1) // 2) // THREADS + 1


def test_lag_cases_give_their_range():
    for rate, lo, hi in P.LAG_CASES + [P.NARROW]:
        f_min, f_max = P.limits(rate, lo, hi)
        assert ref.lag_range(rate, f_min, f_max) == (lo, hi)
        assert pitch_lags(rate, f_min, f_max) == (lo, hi)


def test_lag_cases_straddle_the_loops():
    cases = [(lo, hi) for _, lo, hi in P.LAG_CASES]
    diffs = {hi - lo for lo, hi in cases}
    info = {(lo, hi): _lag_passes(lo, hi) for lo, hi in cases}
    assert {0, 1} <= diffs
    # the voiced loop's second pass: hi - lo = 255 is one pass, 256 two
    assert any(v[1] == 1 and hi - lo == THREADS - 1 for (lo, hi), v in info.items())
    assert any(v[1] == 2 and hi - lo == THREADS for (lo, hi), v in info.items())
    # the two-lag loop's second pass: the last hi - lo with one pass and the first with two, both in the list
    one = max(d for d in range(PI["kMaxTau"]) if _lag_passes(2, 2 + d)[2] == 1)
    assert one in diffs and one + 1 in diffs and one - 1 in diffs and one + 2 in diffs
    assert max(d for d in diffs) >= one + 2
    # both parities of nR at every edge
    for group in ({0, 1}, {254, 255, 256, 257}, {506, 507, 508, 509, 510}):
        assert group <= diffs
        assert {(d + 3) % 2 for d in group} == {0, 1}
    assert {(hi - lo + 3) % 2 for lo, hi in cases if lo == 2} == {0, 1}
    assert {(hi - lo + 3) % 2 for lo, hi in cases if hi == PI["kMaxTau"]} == {0, 1}
    assert min(lo for lo, _ in cases) == 2 and max(hi for _, hi in cases) == PI["kMaxTau"]
    # every lag index stays inside a[kMaxTau + 3] and r[kMaxTau + 2]
    for lo, hi in cases:
        nR = hi - lo + 3
        assert 2 * ((nR + 1) // 2) <= PI["kMaxTau"] + 2 and nR <= PI["kMaxTau"] + 2
    # rates other than 44 100 Hz at the extremes
    assert {rate for rate, lo, hi in P.LAG_CASES if lo == 2 or hi == PI["kMaxTau"]} - {44100.0}


def test_window_and_chunk_counts_straddle_the_grid():
    cap = NUM_CUS * PITCH_GRID[0]
    lengths, poison, bad = P.window_case(NUM_CUS)
    wins = [ref.num_windows(n) for n in lengths]
    total = sum(wins)
    assert total > 2 * cap
    isbad = [g in set(bad) for g in range(total)]
    assert any(isbad[g] and not isbad[g + cap] for g in range(total - cap))
    assert any(not isbad[g] and isbad[g + cap] for g in range(total - cap))
    assert isbad[total - 1] and isbad[sum(wins[:2]) - 1]                      # a sound's last window is bad
    assert P.NARROW[2] - P.NARROW[1] + 1 == 16
    lengths = P.chunk_case(NUM_CUS)
    assert P.n_chunks(lengths) > 2 * cap
    assert {PI["kPW"] - 1, PI["kPW"], PI["kPW"] + 1, 191, 192} <= set(lengths)
    for k in (1, 2):
        assert {PI["kChunk"] * k - 1, PI["kChunk"] * k, PI["kChunk"] * k + 1} <= set(lengths)
    # a power window straddles a chunk end inside a sound: start < kChunk < start + kPW <= length
    assert any(n >= PI["kChunk"] - PI["kPH"] + PI["kPW"] for n in lengths)
    assert all(n < PI["kW"] for n in lengths[:2 * cap + 50])                 # no pitch window in the short sounds


def test_voicings_cover_the_division():
    assert {-2.0, -1.0, -0.5} <= set(P.VOICINGS) and max(P.VOICINGS) >= 1e3

