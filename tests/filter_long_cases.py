"""The cases of tests/test_gpu_filter_long_variants.py and tests/test_gpu_filter_band_variants.py as data: segment
lengths, values and the classes each unbanded case must launch -- TEST INFRASTRUCTURE, no GPU needed.
tests/test_filter_plan.py checks on the CPU that the restated plan (tests/filter_plan.py) gives every case the classes
it is named for.

Unbanded cases: sources beyond 48 frames, in groups of (count, shortest, longest) with lengths drawn uniformly; targets
of 0...150 frames, m = 70 (three target groups, the last one of six): 32 planted near-copies of sources resampled to
another length, three empty ones and 29 of one frame (the first group: a longest member of one frame), six of any
length.  Banded cases: about 60 sources of 1...120 frames against 257 targets of 0...120.
"""
from collections import namedtuple

import numpy as np

from soundsym_amd import synth

TGT_MAX = 150
LongCase = namedtuple("LongCase", "name groups dim squared m classes grid", defaults=(None,))
_A = ((256, 65, 96), (256, 97, 128))
G, SKIP = "generic", True
LONG_CASES = [
    # passes of 48 and of 64 rows side by side, both classes with short members whose first tile is empty
    LongCase("nt3x2_nt4x2", _A, 13, False, 70, ((G, 3, 2, SKIP), (G, 4, 2, SKIP))),
    # every source fills its class's rows: the plain instantiation
    LongCase("nt3x2_nt4x2_full_rows", ((256, 96, 96), (256, 128, 128)), 13, False, 70, ((G, 3, 2, False), (G, 4, 2, False))),
    # 50 pairs of two 48-row passes ride with the 150 of two 64-row passes
    LongCase("small_class_joins", ((100, 65, 96), (300, 97, 128)), 13, False, 70, ((G, 4, 2, SKIP),)),
    # 128 pairs each: one 64-row pass on the generic kernel, (3, 2) at row origin 96 of a 192-row slot, (3, 3) at 48
    LongCase("nt4x1_nt3x2_nt3x3", ((256, 49, 64), (256, 65, 96), (256, 129, 144)), 13, False, 70,
             ((G, 4, 1, False), (G, 3, 2, SKIP), (G, 3, 3, False))),
    # the three single-pass classes beside the long ones; the last class (193...200 frames) keeps its shape, however small
    LongCase("short_and_long", ((1024, 1, 200),), 13, False, 70,
             (("sp", 1, 1, False), ("sp", 2, 1, False), ("sp", 3, 1, False), (G, 4, 2, SKIP), (G, 4, 3, SKIP), (G, 3, 5, SKIP))),
    # nine runs of shapes for seven counter sets: the set's own shape takes the rest, and every small class joins it
    LongCase("counter_cap", ((96, 49, 300),), 13, False, 70, ((G, 4, 5, SKIP),)),
    # ... and where only the cap can give that shape: eight runs, the last one's own shape six passes of 48 rows
    LongCase("counter_cap_288", ((96, 49, 288),), 13, False, 70, ((G, 4, 5, SKIP),)),
    LongCase("ku3", _A, 40, False, 70, ((G, 3, 2, SKIP), (G, 4, 2, SKIP))),
    LongCase("squared", _A, 20, True, 70, ((G, 3, 2, SKIP), (G, 4, 2, SKIP))),
    # the headline's segment shape
    LongCase("equal_128", ((64, 128, 128),), 13, False, 40, ((G, 4, 2, False),), (64, 40, 128, 13)),
    # hand-off rows through 64 passes; sources that end 1, 15 and 16 rows into a pass
    LongCase("many_passes", tuple((2, f, f) for f in (49, 64, 100, 700, 1000, 2049, 3000, 4096)), 13, False, 40,
             ((G, 4, 64, SKIP),)),
]
SAME_LENGTHS = ("nt3x2_nt4x2", "ku3", "squared")        # one draw of lengths at three record layouts


def _values(st, f, dim, sig):
    return (st.normal(int(f) * dim).reshape(int(f), dim) * sig).astype(np.float32)


def _resample(st, a, f, dim, sig):
    """Source a resampled to f frames along a straight warping line, + noise."""
    rows = np.rint(np.linspace(0.0, a.shape[0] - 1.0, f)).astype(np.int64)
    return (a[rows].astype(np.float64) + st.normal(f * dim).reshape(f, dim) * (0.05 * sig)).astype(np.float32)


def _other_values(src, tgt, dim, seed):
    st, sig = synth.Stream(seed), synth.sigma(dim)
    return ([(st.normal(a.size).reshape(a.shape) * sig).astype(np.float32) for a in src],
            [(st.normal(a.size).reshape(a.shape) * sig).astype(np.float32) for a in tgt])


def source_lengths(case):
    name = SAME_LENGTHS[0] if case.name in SAME_LENGTHS else case.name
    st = synth.Stream(0x5EEDF300 + 16 * [c.name for c in LONG_CASES].index(name))
    return np.concatenate([lo + st.integers(cnt, hi - lo + 1) for cnt, lo, hi in case.groups])


def long_case_data(case, values_seed=0):
    """(src, tgt) lists of [frames, dim] float32.  values_seed != 0: the same lengths, other values at the same amplitude
    (the scratch-filling search of the stale-task check)."""
    k = [c.name for c in LONG_CASES].index(case.name)
    dim, sig = case.dim, synth.sigma(case.dim)
    if case.grid:
        g = synth.make_grid(*case.grid, 0x5EEDF380 + k)
        src, tgt = list(g.sources), list(g.targets)
    else:
        ls = source_lengths(case)
        st = synth.Stream(0x5EEDF400 + 16 * k)
        ls = ls[st.permutation(ls.size)]
        src = [_values(st, f, dim, sig) for f in ls]
        for i in (int(x) for x in st.integers(4, ls.size)):        # duplicates of the same length: the first index wins a tie
            same = [j for j in range(i + 1, ls.size) if ls[j] == ls[i]]
            if same:
                src[same[0]] = src[i].copy()
        n_pl = 32 if case.m == 70 else case.m // 2
        tgt = []
        for t, p in enumerate(st.integers(n_pl, ls.size)):          # planted: a source at another length, + noise
            a = src[int(p)]
            tgt.append(_resample(st, a, int(np.clip(a.shape[0] + t % 5 - 2, 1, TGT_MAX)), dim, sig))
        if case.m == 70:                                            # a whole group whose longest target has one frame
            lt = [0] * 3 + [1] * 29 + [TGT_MAX - k % 4] + [int(x) for x in 2 + st.integers(5, TGT_MAX - 1)]
        else:
            lt = [0] * 2 + [int(x) for x in 1 + st.integers(case.m - n_pl - 2, TGT_MAX)]
        tgt += [_values(st, f, dim, sig) for f in lt]
        tgt = [tgt[int(i)] for i in st.permutation(case.m)]
    if values_seed:
        src, tgt = _other_values(src, tgt, dim, values_seed)
    return src, tgt


def beyond_reach_data():
    """One source of 4097 frames among shorter ones: the filter stops at 4096."""
    dim, sig, st = 13, synth.sigma(13), synth.Stream(0x5EEDF4F0)
    src = [_values(st, f, dim, sig) for f in (60, 4097, 130, 17, 64, 200, 1, 90)]
    tgt = [_resample(st, src[i], f, dim, sig) for i, f in ((0, 58), (2, 133), (5, 150), (1, 150))]
    tgt += [_values(st, f, dim, sig) for f in (0, 1, 33, 77, 150, 96, 5, 120)]
    return src, tgt, dim


# ---- the banded kernel -----------------------------------------------------------------------------------------------
# every instantiation launch_band can pick: NTB = ceil((2 r + 1) / 16) tiles of diagonals, LASTN = 1 where the radius is a
# multiple of 8 (the band ends one diagonal into its last tile), 8-wave workgroups up to NTB = 5 and 4-wave ones at 6
BAND_RADII = (3, 7, 0, 15, 8, 23, 16, 31, 24, 39, 32, 47, 40)
BandCase = namedtuple("BandCase", "r dim squared")
BAND_CASES = [BandCase(r, 13, False) for r in BAND_RADII] + [BandCase(r, 40, False) for r in (8, 32, 47)] + \
    [BandCase(r, 13, True) for r in (8, 32)]
BAND_N, BAND_M, BAND_MAX = 60, 257, 120
BAND_LDS_LIMIT = 160 * 1024 - 64


def band_instance(r):
    """(NTB, LASTN, waves per workgroup) of launch_band for radius r."""
    ntb = (2 * r + 1 + 15) // 16
    return ntb, 1 if 2 * r + 1 == 16 * (ntb - 1) + 1 else 16, 8 if ntb <= 5 else 4


def band_lds_bytes(r, src_max, tgt_max):
    """dtw_filter.hip band_slots / band_lds_bytes: both sources of a pair, slot s of a source holding frame s - r."""
    kb = (2 * r + 1 + 15) // 16 * 16
    slots = max(r + src_max, max(tgt_max, 1) + kb) + 1
    return (2 * slots * 48 + 8) * 2


def band_data(r, dim, values_seed=0, long_source=0):
    """(src, tgt): 60 sources of 1...120 frames (one empty, one pair of duplicates) and 257 targets of 0...120, a third of
    them planted near-copies within +-r frames of their source's length.  long_source: frames of one more source, in place of
    source 3 (a pair that does not fit the LDS)."""
    sig = synth.sigma(dim)
    st = synth.Stream(0x5EEDF500 + 64 * r + dim)
    ls = 1 + st.integers(BAND_N, BAND_MAX)
    ls[7] = 0
    ls[11], ls[40] = BAND_MAX, 1
    if long_source:
        ls[3] = long_source
    src = [_values(st, f, dim, sig) for f in ls]
    src[21] = src[20].copy()
    n_pl = BAND_M // 3
    tgt = []
    for t, p in enumerate(st.integers(n_pl, BAND_N)):
        p = int(p)
        while src[p].shape[0] == 0:
            p = (p + 1) % BAND_N
        a = src[p]
        tgt.append(_resample(st, a, int(np.clip(a.shape[0] + t % (2 * r + 1) - r, 1, BAND_MAX)), dim, sig))
    lt = [0] * 3 + [1, BAND_MAX] + [int(x) for x in 1 + st.integers(BAND_M - n_pl - 5, BAND_MAX)]
    tgt += [_values(st, f, dim, sig) for f in lt]
    tgt = [tgt[int(i)] for i in st.permutation(BAND_M)]
    if values_seed:
        src, tgt = _other_values(src, tgt, dim, values_seed)
    return src, tgt


# ---- one search ------------------------------------------------------------------------------------------------------
def run_search(e, dim, src, tgt):
    """Filter matrix, argmin and the launch counters of one search on Engine e; the handles and packed arrays behind."""
    from soundsym_amd.engine import pack_segments
    sf, so = pack_segments(src, dim, np.float32)
    tf, to = pack_segments(tgt, dim, np.float32)
    d, q = e.dictionary(sf, so, dim), e.queries(tf, to, dim)
    filt = e.pair_matrix(d, q, exact=False)
    idx, cost = e.match(d, q)
    tm = e.timings()
    out = dict(filt=filt, idx=idx, cost=cost, cells=int(tm["n_filter_cells"]), launches=int(tm["main_launches"]),
               used_filter=int(tm["used_filter"]))
    return out, (d, q, sf, so, tf, to)
