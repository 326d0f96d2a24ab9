"""Which kernel scores a list of dtw pairs: launch_dtw_exact (soundsym_amd/csrc/dtw_exact.hip) restated -- TEST
INFRASTRUCTURE.  tests/test_exact_plan.py pins every factor and limit below to the source; tests/exact_cases.py holds the
cases that stand on the plan's thresholds.

The launcher picks among five kernels.  By list length: dtw_exact_cells_kernel takes unbanded lists of up to
CELLS_PER_CU pairs per CU (and every banded list), dtw_exact_pipe_kernel lists of up to PIPE_PER_CU / pipeW per CU where
pipeW = ceil(longest source / 64) lies in PIPE_W_MIN...PIPE_W_MAX, dtw_exact_reg_kernel the rest.  A candidate list
(listed = True) has its length on the device: every candidate kernel is launched with the thresholds below and decides
for itself; an all-pairs call or a chain step is decided on the host from the same numbers.  By frame width: the
register widths of DIMR_LADDER (49...64 values in two fetches, 65...96 in three), above them the generic
dtw_exact_kernel.  By LDS: the register kernel's rows must fit REG_LDS_KIB (REG_LDS_WIDE_KIB at the widths 64 and 96), else
the generic kernel with its frames in LDS (GENERIC_LDS_KIB) or in global memory; a boundary row above BOUND_KIB is
unsupported.
"""
from collections import namedtuple

CELLS_PER_CU = 4            # cellsMax = num_cus * 4
PIPE_PER_CU = 64            # pipeMax = num_cus * 64 / pipeW
PIPE_W_MIN, PIPE_W_MAX = 2, 8
CELLS_SRC_FRAMES = 256      # the cells kernel's unbanded lists: src.max_frames <= 256
PANEL_MAX = 128             # panelX <= 128: targets in panels of 128 columns, bands up to r = 63
DIMR_LADDER = (12, 14, 16, 40, 48, 64, 96)
NARROW_DIMR = 48            # widest frames of the cells and pipe kernels
BOUND_KIB = 120             # boundary rows: 2 * fbCap doubles
REG_LDS_KIB, REG_LDS_WIDE_KIB = 64, 150
CELLS_LDS_KIB = PIPE_LDS_KIB = 150
GENERIC_LDS_KIB = 64
U64_MAX = 2 ** 64 - 1

Plan = namedtuple("Plan", "launched cells_hi pipe_lo pipe_hi reg_lo")
Plan.__doc__ = """launched: the kernels in launch order ("cells", "pipe", "reg<dimr>", "generic_lds", "generic_global"),
or ("unsupported",).  cells_hi / pipe_lo, pipe_hi / reg_lo: totalHi of the cells kernel, totalLo and totalHi of the
pipelined one, totalLo of the register kernel -- None where that kernel is not launched."""


def wave_ld(dimr):
    """dtw_wave.hpp: row stride of f64 frames, 2 (mod 4) doubles."""
    return dimr if dimr % 4 == 2 else dimr + 2


def exact_dimr(dim):
    return next((r for r in DIMR_LADDER if dim <= r), 0)


def exact_ld(dimr, f32):
    up4 = (dimr + 3) // 4 * 4
    return up4 + (0 if up4 % 8 == 4 else 4) if f32 else wave_ld(dimr)


def reg_lds_bytes(tgt_max_frames, dim, dtype, band):
    """regLds: two boundary rows and the staged target rows (all of them, or a banded chunk's window)."""
    dimr = exact_dimr(dim)
    fb_even = (max(tgt_max_frames, 1) + 1) & ~1
    win = min(fb_even, (64 + 2 * band + 1) & ~1) if band >= 0 else fb_even
    return 2 * fb_even * 8 + win * exact_ld(dimr, dtype == "f32") * (4 if dtype == "f32" else 8)


def generic_lds_bytes(tgt_max_frames, dim):
    """(boundBytes, frameBytes) of dtw_exact_kernel."""
    fb = max(tgt_max_frames, 1)
    return 2 * fb * 8, (64 * (dim | 1) + fb * (dim | 1)) * 8


def exact_plan(src_max_frames, tgt_max_frames, dim, dtype, band, num_cus, listed, max_pairs):
    """The launches of one launch_dtw_exact call.  listed: a candidate list of at most max_pairs pairs whose length is on
    the device; otherwise max_pairs is the call's N x M (or a chain step's N) and the host decides."""
    f32 = dtype == "f32"
    elt = 4 if f32 else 8
    fb_cap = max(tgt_max_frames, 1)
    bound_bytes, frame_bytes = generic_lds_bytes(tgt_max_frames, dim)
    if bound_bytes > BOUND_KIB * 1024:
        return Plan(("unsupported",), None, None, None, None)
    total = max_pairs
    if total == 0:
        return Plan((), None, None, None, None)
    fb_even = (fb_cap + 1) & ~1
    dimr = exact_dimr(dim)
    ldr = exact_ld(dimr, f32)
    banded = band >= 0
    win = min(fb_even, (64 + 2 * band + 1) & ~1) if banded else fb_even
    reg_lds = 2 * fb_even * 8 + win * ldr * elt
    launched = []
    cells_hi = pipe_lo = pipe_hi = reg_lo = None

    low_bound = 0
    panel = 2 * band + 1 if banded else min(fb_even, PANEL_MAX)
    cells_lds = 2 * fb_even * 8 + panel * 64 * 8 + win * ldr * elt
    cells_max = U64_MAX if banded else num_cus * CELLS_PER_CU
    cells_ok = (dimr and dimr <= NARROW_DIMR and panel <= PANEL_MAX and cells_lds <= CELLS_LDS_KIB * 1024 and
                (banded or (src_max_frames <= CELLS_SRC_FRAMES and reg_lds <= REG_LDS_KIB * 1024)) and
                (listed or total <= cells_max))
    if cells_ok:
        launched.append("cells")
        cells_hi = cells_max
        if total <= cells_max:
            return Plan(tuple(launched), cells_hi, None, None, None)
        low_bound = cells_max + 1

    pipe_w = (src_max_frames + 63) // 64
    pipe_lds = pipe_w * fb_even * 8 + fb_even * ldr * elt + (pipe_w + 1) * 4
    pipe_max = num_cus * PIPE_PER_CU // max(pipe_w, 1)
    pipe_ok = (not banded and dimr and dimr <= NARROW_DIMR and PIPE_W_MIN <= pipe_w <= PIPE_W_MAX and
               pipe_lds <= PIPE_LDS_KIB * 1024 and reg_lds <= REG_LDS_KIB * 1024)
    if pipe_ok and low_bound <= pipe_max and not (not listed and total > pipe_max):
        launched.append("pipe")
        pipe_lo, pipe_hi = low_bound, pipe_max
        # a list the pipelined kernel certainly took: the register kernel behind it only redoes a give-up
        reg_lo = U64_MAX if (not listed or max_pairs <= pipe_max) else pipe_max + 1
    else:
        reg_lo = low_bound

    if dimr and reg_lds <= (REG_LDS_WIDE_KIB if dimr >= 64 else REG_LDS_KIB) * 1024:
        launched.append("reg%d" % dimr)
        return Plan(tuple(launched), cells_hi, pipe_lo, pipe_hi, reg_lo)
    launched.append("generic_lds" if bound_bytes + frame_bytes <= GENERIC_LDS_KIB * 1024 else "generic_global")
    return Plan(tuple(launched), cells_hi, pipe_lo, pipe_hi, None)


def workers(plan, length):
    """The launched kernels that score a list of `length` pairs (the kernels' own comparisons with their thresholds; a
    give-up of the pipelined kernel aside).  Every pair is scored exactly once iff this has one entry."""
    out = []
    for k in plan.launched:
        if k == "cells":
            works = length <= plan.cells_hi
        elif k == "pipe":
            works = plan.pipe_lo <= length <= plan.pipe_hi
        elif k.startswith("reg"):
            works = plan.reg_lo <= length
        else:
            works = k != "unsupported"
        if works:
            out.append(k)
    return out


def worker(plan, length):
    w = workers(plan, length)
    assert len(w) == 1, (plan, length, w)
    return w[0]


def route(src_max_frames, tgt_max_frames, dim, dtype, band, num_cus, listed, max_pairs, length=None):
    """The one kernel that scores the list (length: the listed pairs, max_pairs when not given)."""
    p = exact_plan(src_max_frames, tgt_max_frames, dim, dtype, band, num_cus, listed, max_pairs)
    if p.launched == ("unsupported",):
        return "unsupported"
    return worker(p, max_pairs if length is None else length)


def longest_target(name, src_max_frames, dim, dtype, band, num_cus, max_pairs, limit=7680):
    """The largest longest-target length at which an all-pairs call of max_pairs pairs is scored by a kernel whose name
    starts with `name`, or None."""
    best = None
    for fb in range(1, limit + 1):
        if route(src_max_frames, fb, dim, dtype, band, num_cus, False, max_pairs).startswith(name):
            best = fb
    return best
