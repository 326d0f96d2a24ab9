"""The cases of tests/test_gpu_exact_routes.py as data: which lists, shapes and lengths, and the kernel
each must land on -- TEST INFRASTRUCTURE, no GPU needed.  Every table is a function of num_cus; tests/test_exact_plan.py
checks on the CPU that each case lands on the route it is named for (tests/exact_plan.py).

  a. HANDOFFS    candidate lists of exactly T + 1, T, T - 1 pairs at the device-side handoffs cells -> reg,
                 cells -> pipe and pipe -> reg (N <= 64 distinct sources x M targets = L, top-k with k = N: every pair
                 is listed and every cost comes back), and the same lengths in a list with room for 2 L pairs
  b. ALL_PAIRS   all-pairs calls on either side of the same thresholds; CHAINS: the dtw chain's list steps
  c. DIMS        frame widths around every rung of the dimr ladder, on a short and on a long list
  d. LDS_*       the last target length of the register kernel's LDS and the generic kernel behind it; LONGEST
  e. WIDE_BANDS  bands the cells kernel does not take
  f. SAME_*      one set of 40 pairs scored by the cells, the pipelined and the register kernel
"""
import exact_plan as xp

TOPK_MAX = 64               # SSYM_TOPK_MAX: the most sources a top-k row returns
DIM = 13


def split(length):
    """N x M = length with the most sources top-k can return (N <= 64); a prime length gives N = 1."""
    n = max(d for d in range(1, TOPK_MAX + 1) if length % d == 0)
    return n, length // n


# (name, pairs per CU at the threshold, longest source, dtype, the kernel up to the threshold, the kernel past it)
HANDOFFS = [
    ("cells_reg", 4, 64, "f32", "cells", "reg14"),              # pipeW = 1: no pipelined kernel
    ("cells_pipe_w4", 4, 230, "f32", "cells", "pipe"),
    ("pipe_reg_w4", 16, 230, "f32", "pipe", "reg14"),
    ("cells_pipe_w4_f64", 4, 230, "f64", "cells", "pipe"),
    ("pipe_reg_w4_f64", 16, 230, "f64", "pipe", "reg14"),
    ("pipe_reg_w8", 8, 500, "f32", "pipe", "reg14"),            # sources past 256 frames: no cells kernel
]
TGT_LO, TGT_HI = 8, 30


def handoff_lengths(per_cu, ncu):
    """In the order they run on one engine: every list follows one that left other costs in the candidate buffer."""
    t = per_cu * ncu
    return [t + 1, t, t - 1]


def handoff_routes(ncu, room=False):
    """(label, exact_plan.route arguments, the kernel that must work) of every list of a.  room: the same lengths in
    lists whose capacity is twice their length, so that only the comparisons on the device decide."""
    for name, per_cu, src_hi, dtype, below, above in HANDOFFS:
        for length in handoff_lengths(per_cu, ncu):
            cap = 2 * length if room else length
            yield ("%s/%d" % (name, length), (src_hi, TGT_HI, DIM, dtype, -1, ncu, True, cap, length),
                   below if length <= per_cu * ncu else above)


# (pairs per CU, offset from the threshold, longest source, the kernel)
ALL_PAIRS = [(4, 0, 64, "cells"), (4, 1, 64, "reg14"), (4, 0, 230, "cells"), (4, 1, 230, "pipe"),
             (16, 0, 230, "pipe"), (16, 1, 230, "reg14")]


def all_pairs_routes(ncu):
    for per_cu, off, src_hi, want in ALL_PAIRS:
        length = per_cu * ncu + off
        yield ("all_pairs/%d/%d" % (src_hi, length), (src_hi, TGT_HI, DIM, "f32", -1, ncu, False, length), want)


# (pairs per CU, offset, entry frames lo...hi, the kernel of the chain's list steps)
CHAINS = [(4, -1, 8, 64, "cells"), (4, 0, 8, 64, "cells"), (4, 1, 8, 64, "reg14"),
          (16, 0, 100, 256, "pipe"), (16, 1, 100, 256, "reg14")]


CHAIN_START = 40            # frames of the start sound
CHAIN_STEPS = 4


def chain_routes(ncu):
    for per_cu, off, lo, hi, want in CHAINS:
        n = per_cu * ncu + off
        yield ("chain/step0/%d" % n, (hi, CHAIN_START, DIM, "f32", -1, ncu, False, n), want)
        yield ("chain/list/%d" % n, (hi, hi, DIM, "f32", -1, ncu, True, n, n), want)     # count == max_pairs == N


DIMS = [1, 11, 12, 13, 14, 15, 16, 17, 39, 40, 41, 48, 49, 63, 64, 65, 95, 96, 97, 128]
WIDTH_SRC = [1, 140, 0, 64, 65, 37, 128, 129, 90]        # 9 ragged sources, one empty
WIDTH_TGT = [140, 1, 0, 63, 65, 128, 17]                 # 7 ragged targets, one empty
WIDTH_BAND = 7


def width_long_sources(ncu):
    """Lengths 0...64 of enough sources for a list of more than 4 pairs per CU against the 7 targets."""
    n = -(-(xp.CELLS_PER_CU * ncu + 1) // len(WIDTH_TGT))
    return [(7 * i + 64) % 65 for i in range(n)]


def width_want(dim, band, short):
    dimr = xp.exact_dimr(dim)
    if dimr and dimr <= 48:
        return "cells" if (band >= 0 or short) else "reg%d" % dimr
    return "reg%d" % dimr if dimr else "generic_global"


def width_routes(ncu):
    for dim in DIMS:
        for dtype in ("f32", "f64"):
            for band in (-1, WIDTH_BAND):
                for short, lens in ((True, WIDTH_SRC), (False, width_long_sources(ncu))):
                    yield ("width/%d/%s/%d/%s" % (dim, dtype, band, short),
                           (max(lens), max(WIDTH_TGT), dim, dtype, band, ncu, False, len(lens) * len(WIDTH_TGT)),
                           width_want(dim, band, short))


LDS_SRC = [30, 300, 77, 150]             # pipeW = 5: the pipelined kernel takes the short list while regLds fits
LDS_SRC_LONG = [30, 520, 77, 150]        # pipeW = 9: the register kernel
LDS_DIMS = [13, 40]
GENERIC_LDS_DIMS = [97, 124]             # the generic kernel keeps its frames in LDS only behind no register kernel


def lds_targets(fb):
    return [9, fb, max(fb // 2, 1)]


def reg_fit(dim, dtype, ncu):
    """The longest target whose rows the register kernel's 64 KiB take."""
    return xp.longest_target("reg", max(LDS_SRC_LONG), dim, dtype, -1, ncu, 12, limit=2048)


def lds_routes(ncu):
    for dim in LDS_DIMS:
        for dtype in ("f32", "f64"):
            fit = reg_fit(dim, dtype, ncu)
            dimr = xp.exact_dimr(dim)
            for fb, a, b in ((fit, "pipe", "reg%d" % dimr), (fit + 1, "generic_global", "generic_global"),
                             (fit + 2, "generic_global", "generic_global")):
                yield ("lds/%d/%s/%d" % (dim, dtype, fb), (max(LDS_SRC), fb, dim, dtype, -1, ncu, False, 12), a)
                yield ("lds_long/%d/%s/%d" % (dim, dtype, fb), (max(LDS_SRC_LONG), fb, dim, dtype, -1, ncu, False, 12), b)
    for dim in GENERIC_LDS_DIMS:
        for dtype in ("f32", "f64"):
            last = xp.longest_target("generic_lds", max(LDS_SRC), dim, dtype, -1, ncu, 12, limit=2048)
            yield ("generic/%d/%s/%d" % (dim, dtype, last), (max(LDS_SRC), last, dim, dtype, -1, ncu, False, 12), "generic_lds")
            yield ("generic/%d/%s/%d" % (dim, dtype, last + 1), (max(LDS_SRC), last + 1, dim, dtype, -1, ncu, False, 12),
                   "generic_global")


LONGEST = 7680               # 2 x 7680 doubles: the 120 KiB of boundary rows
WIDE_BANDS = [64, 100]
BAND_SRC = [150, 400, 233, 310, 191, 377]
BAND_TGT = [400, 150, 256, 193, 320, 215]


def band_want(dim, dtype):
    """192 or 264 staged rows of 40 doubles pass the register kernel's 64 KiB: the generic kernel has those pairs."""
    return "generic_global" if (dim, dtype) == (40, "f64") else "reg%d" % xp.exact_dimr(dim)


def band_routes(ncu):
    for band in WIDE_BANDS:
        for dim in LDS_DIMS:
            for dtype in ("f32", "f64"):
                yield ("band/%d/%d/%s" % (band, dim, dtype), (max(BAND_SRC), max(BAND_TGT), dim, dtype, band, ncu, False, 36),
                       band_want(dim, dtype))


SAME_N, SAME_M, SAME_SRC, SAME_TGT = 8, 5, 200, 25       # 40 pairs of 200-frame sources and 25-frame targets


def same_bits_targets(ncu):
    """Targets in all: the 40 pairs alone, in a list just past 4 pairs per CU, in one just past 16 per CU."""
    return [(SAME_M, "cells"), (xp.CELLS_PER_CU * ncu // SAME_N + 1, "pipe"), (16 * ncu // SAME_N + 1, "reg14")]


def same_bits_routes(ncu):
    for m, want in same_bits_targets(ncu):
        for listed in (False, True):
            yield ("same_bits/%d/%s" % (m, listed), (SAME_SRC, SAME_TGT, DIM, "f32", -1, ncu, listed, SAME_N * m), want)


def planned_routes(ncu):
    """Every case above as (label, exact_plan.route arguments, kernel) for a device of ncu CUs."""
    for gen in (handoff_routes(ncu), handoff_routes(ncu, room=True), all_pairs_routes(ncu), chain_routes(ncu),
                width_routes(ncu), lds_routes(ncu), band_routes(ncu), same_bits_routes(ncu)):
        for item in gen:
            yield item
