"""The launch plan of the unbanded dtw filter, restated from the segment lengths, the dim and the device's CU count
(soundsym_amd/csrc/dtw_filter_plan.hpp plan_filter) -- TEST INFRASTRUCTURE, no GPU needed and no call into the library.

The GPU tests (tests/test_gpu_filter_variants.py: sources of at most 48 frames; tests/test_gpu_filter_long_variants.py:
beyond) compare the timings' launch and cell counts with this plan: that proves that a case ran the variant it names and
that an A/B comparison compared two different launches.  tests/test_filter_plan.py holds the plan against the cases' class
tables on the CPU, and against plan_filter itself, field by field (tests/cpp/filter_plan_dump.cpp prints its launches).
"""
from collections import namedtuple

REC_HALFS = 48          # kFilterRecHalfs
WAVES_PER_BLOCK = 4     # kFilterWavesPerBlock
ROW_BLOCK = 4           # kSpRowBlock
RING = 4                # kSpRing
SP_OCC_NT2 = 3          # SSYM_SP_OCC_NT2: workgroups per CU of the two-tile sp kernel with two operand planes
MAX_CLASSES = 10        # kMaxClasses: counter sets, three single-pass classes + up to seven multi-pass ones
SMALL_CLASS = 128       # a long class of fewer pairs joins its successor
MAX_FRAMES = 4096       # filter_shape: beyond, the exact kernel only

# kernel: "mp", "sp", "generic" or "pk"; passes of 16 * nt rows on the last rows_pad - origin rows of the end-aligned slots;
# skip: the SKIP0 instantiation (a first pass's empty first tile is not evaluated)
# grid, chunk: workgroups and tasks per grab of the launch; wg: dtw_filter_wg_kernel serves it
Launch = namedtuple("Launch", "nt kernel lo hi blocks cells passes origin skip grid chunk wg", defaults=(1, 0, False, 0, 0, False))


def _ceil(a, b):
    return -(-a // b)


def filter_ku(dim):
    """Operand planes the unbanded filter multiplies (ssym_internal.hpp filter_pieces / filter_mfmas): up to 13 values
    record layout 3 (two planes), 14...26 layout 1 in two planes, 27...42 layout 1 in three."""
    du = min(dim, 42)
    return 2 if du <= 26 else 3


def filter_shape(max_frames):
    """(tiles per pass, passes) of the set's own shape (ssym_internal.hpp filter_shape); (0, 0) beyond the filter's reach."""
    if max_frames <= 48:
        return _ceil(max(max_frames, 1), 16), 1
    if max_frames <= MAX_FRAMES:
        return 4, _ceil(max_frames, 64)
    return 0, 0


def _cells(pair_len, col_len, lo, hi, origin, rows_pad, pass_rows, row_block, min_cols, per_task=1):
    """plan_filter's cells of single-pass launches: rows of the pairs [lo, hi) times the columns of every target group."""
    cols = sum(max(c, min_cols) if row_block else c for c in col_len)
    rows = 0
    for sp in range(lo, hi):
        longer = pair_len[sp]
        if per_task > 1:                 # every pair of a task starts at the task's first row block
            first = lo + (sp - lo) // per_task * per_task
            longer = max(pair_len[first:min(first + per_task, hi)])
        r0min = rows_pad - longer
        if row_block:
            rows += pass_rows - min(max(r0min - origin, 0), 15) // row_block * row_block
        else:
            rows += pass_rows            # one pass: its first pass is the only one
    return rows * cols


def _cells_passes(pair_len, col_len, lo, hi, origin, rows_pad, pass_rows, passes, skip):
    """plan_filter's cells with rowBlock = 0 (dtw_filter_kernel): a task skips its leading passes of padding, and under SKIP0 the
    16 rows of its first pass's first tile when that holds padding only."""
    cols = sum(col_len)
    rows = 0
    for sp in range(lo, hi):
        r0min = rows_pad - pair_len[sp]
        first = min(max(r0min - origin, 0) // pass_rows, passes - 1)
        rows += (passes - first) * pass_rows
        if skip and r0min - (origin + first * pass_rows) >= 17:
            rows -= 16
    return rows * cols


def best_shape(length):
    """LongClass best(): passes of 48 or of 64 rows, whichever pads `length` frames least (ties: 64)."""
    p4, p3 = _ceil(max(length, 1), 64), _ceil(max(length, 1), 48)
    return (3, p3) if 48 * p3 < 64 * p4 else (4, p4)


def filter_plan(src_lens, tgt_lens, dim, num_cus, sp=True, mp=True, pair_blocks=True, skip0=True, long_classes=True,
                one_launch=False, wg=True, pk=False, nt8=False, mp_always=False, pair_block=None, pruned=False, prune_nt=0,
                prune_swept=1.0):
    """The launches of one unbanded filter call: per class of source pairs its tile count, kernel, pair range, pair blocks
    of the sp kernels' task order, DP cells per lane (n_filter_cells is 64 times their sum), row passes, row origin,
    whether it skips first tiles, its grid and task chunk, and whether dtw_filter_wg_kernel serves it.  Sources of at most
    48 frames: classes cut where the longer member of a pair needs more than 16, 32 frames.  Beyond: the same three
    single-pass classes, then the long classes (passes of 48 or 64 rows, whichever pads least; small classes join their
    successor; the set's own shape takes what the counter sets do not reach).  sp / mp / pair_blocks / skip0 / long_classes /
    wg False: the plan under SSYM_FILTER_SP=0, SSYM_SP_MULTIPAIR=0, SSYM_SP_PAIRBLOCK=0, SSYM_FILTER_SKIP0=0,
    SSYM_FILTER_LONG_CLASSES=0, SSYM_FILTER_WG=0; one_launch, nt8, pk: under SSYM_FILTER_ONE_LAUNCH, SSYM_FILTER_NT8,
    SSYM_FILTER_PK=1; mp_always: SSYM_SP_MULTIPAIR=2; pair_block: SSYM_SP_PAIRBLOCK=<pairs>.  pruned: an early-abandoning
    call (every class on the generic kernel, cells 0, the long pairs in one class of 2 or 4 tiles by prune_nt, the pinned
    SSYM_PRUNE_NT, or the previous call's prune_swept).
    Returns (plan, target groups)."""
    ls = sorted(int(x) for x in src_lens)           # record slots are ordered by length
    lt = sorted(int(x) for x in tgt_lens)
    n, m = len(ls), len(lt)
    n_pad, m_pad = _ceil(n, 32) * 32, _ceil(m, 32) * 32
    mean_tgt = max(_ceil(sum(lt), m), 1) if m else 1
    ls += [0] * (n_pad - n)
    lt += [0] * (m_pad - m)
    top = max(max(ls), 1)
    top_tiles, rb = filter_shape(top)
    assert top_tiles, "beyond 4096 source frames the filter does not run"
    rows_pad = 16 * top_tiles * rb
    n_pairs, n_real = n_pad // 2, (n + 1) // 2
    pair_len = [max(ls[2 * p], ls[2 * p + 1]) for p in range(n_pairs)]
    col_len = [max(lt[32 * g:32 * g + 32]) for g in range(m_pad // 32)]
    n_groups = len(col_len)

    def first_above(frames):                        # first real pair whose longer member exceeds `frames`
        return next((p for p in range(n_real) if pair_len[p] > frames), n_real)

    bound = [0] + [0 if one_launch else first_above(16 * c) for c in range(1, top_tiles)]
    ku = filter_ku(dim)
    grid_blocks = max(8, num_cus * 2 // 8 * 8)      # two workgroups per CU, a multiple of 8
    plan = []

    def wave_blocks(tasks):                         # workgroups of four waves, one task each, rounded up to eight
        return _ceil(_ceil(tasks, WAVES_PER_BLOCK), 8) * 8

    def chunk(rows_per_task, tasks, grid):          # tasks per grab: short tasks several at a time, 16 grabs per wave at least
        c = max(1, min(8, 8192 // max(1, rows_per_task * mean_tgt)))
        return max(1, min(c, tasks // max(1, grid * WAVES_PER_BLOCK * 16)))

    def generic_launch(nt, passes, lo, hi, origin, skip):
        """dtw_filter_kernel and its siblings on four tiles: grid by the kernel's workgroups per CU (three on one tile, one
        on eight), and which of them runs."""
        occ = 3 if nt == 1 else 1 if nt == 8 else 2
        tasks = (hi - lo) * n_groups
        grid = min(grid_blocks // 2 * occ, wave_blocks(tasks))
        ch = chunk(16 * nt * passes, tasks, grid)
        if nt == 4 and pk and not pruned:
            return Launch(nt, "pk", lo, hi, 0, 0, passes, origin, False, grid, ch, False)
        skip = skip and nt in (3, 4) and not pruned
        # the wg kernel's gate: four tiles, no skip, whole blocks of four pairs, no padding pair, an even source count,
        # and pass 0 holding a row of the first (the shortest) pair
        gate = wg and not pruned and nt == 4 and not skip and (hi - lo) % 4 == 0 and hi <= n_real and n % 2 == 0 and \
            origin + 64 > rows_pad - pair_len[lo]
        cells = 0 if pruned else _cells_passes(pair_len, col_len, lo, hi, origin, rows_pad, 16 * nt, passes, skip)
        return Launch(nt, "generic", lo, hi, 0, cells, passes, origin, skip, grid, ch, gate)

    def single_pass(nt, lo, hi, origin):            # a class of one pass: the sp kernels where they serve it
        np_ = hi - lo
        mpn = 3 if ku == 2 else 2
        if pruned or not sp:
            return generic_launch(nt, 1, lo, hi, origin, False)
        if nt == 1 and (mp or mp_always) and (mp_always or _ceil(np_, mpn) * n_groups >= grid_blocks // 2 * 2 * WAVES_PER_BLOCK):
            task_pairs = _ceil(np_, mpn)
            tasks = task_pairs * n_groups
            pb = max(16, (1 << 20) // (mpn * 2 * 16 * REC_HALFS * 2)) if pair_blocks else task_pairs
            pb = pair_block or pb
            grid = min(grid_blocks, wave_blocks(tasks))                 # two workgroups per CU
            return Launch(nt, "mp", lo, hi, _ceil(task_pairs, min(pb, task_pairs)),
                          _cells(pair_len, col_len, lo, hi, origin, rows_pad, 16, ROW_BLOCK, RING, mpn), 1, origin, False,
                          grid, chunk(16 * mpn, tasks, grid), False)
        if nt <= 3 and (ku == 2 or nt <= 2):
            pb = max(16, (1 << 20) // (2 * 16 * nt * REC_HALFS * 2)) if pair_blocks else np_
            pb = pair_block or pb
            occ = 3 if nt == 1 and ku == 2 else SP_OCC_NT2 if nt == 2 and ku == 2 else 2
            tasks = np_ * n_groups
            grid = min(grid_blocks // 2 * occ, wave_blocks(tasks))
            # (the chunk is worked out for the grid dtw_filter_kernel would get: three workgroups per CU on one tile, else two)
            generic_grid = min(grid_blocks // 2 * (3 if nt == 1 else 2), wave_blocks(tasks))
            return Launch(nt, "sp", lo, hi, _ceil(np_, min(pb, np_)),
                          _cells(pair_len, col_len, lo, hi, origin, rows_pad, 16 * nt, ROW_BLOCK, RING), 1, origin, False,
                          grid, chunk(16 * nt, tasks, generic_grid), False)
        return generic_launch(nt, 1, lo, hi, origin, False)

    def multi_pass(nt, passes, lo, hi, origin, skip):
        if passes == 1 and nt <= 3:                  # (the single-pass kernels take it whatever skip says)
            return single_pass(nt, lo, hi, origin)
        return generic_launch(nt, passes, lo, hi, origin, skip)

    for c in range(min(top_tiles, 3)):
        nt, lo = c + 1, bound[c]
        hi = bound[c + 1] if c + 1 < top_tiles else n_pairs
        if hi > lo:
            plan.append(single_pass(nt, lo, hi, rows_pad - 16 * nt))
    if top_tiles < 4:
        return plan, n_groups

    lo3 = bound[3]
    if pruned:                                       # passes of 32 rows when the last pruned call swept under a quarter
        height = prune_nt if prune_nt in (2, 4) else (2 if prune_swept < 0.25 else 4)
        if n_pairs > lo3:
            plan.append(generic_launch(height, rb * 4 // height, lo3, n_pairs, 0, False))
        return plan, n_groups
    if nt8 and rb == 2:                              # the whole 128-row column in one wave
        if n_pairs > lo3:
            plan.append(generic_launch(8, 1, lo3, n_pairs, 0, False))
        return plan, n_groups
    if not long_classes or one_launch:              # the set's own shape for every long pair
        if n_pairs > lo3:
            plan.append(multi_pass(4, rb, lo3, n_pairs, 0, False))
        return plan, n_groups
    cls = []                                         # [nt, passes, lo, hi]
    sp_ = lo3
    while sp_ < n_pairs:
        nt, passes = best_shape(pair_len[sp_] if sp_ < n_real else 0)
        # the run of pairs this shape is the best for: up to the first pair longer than its rows
        end = max(sp_ + 1, min(n_pairs, first_above(16 * nt * passes) if sp_ < n_real else n_pairs))
        cls.append([nt, passes, sp_, n_pairs if end == n_real else end])       # padding pairs ride with the last real one
        sp_ = cls[-1][3]
        if len(cls) == MAX_CLASSES - 3 and sp_ < n_pairs:                        # no counter set left
            cls[-1] = [4, rb, cls[-1][2], n_pairs]
            break
    c = 0
    while c + 1 < len(cls):                          # small classes join their successor; the last one keeps its own
        if cls[c][3] - cls[c][2] < SMALL_CLASS:
            cls[c + 1][2] = cls[c][2]
            del cls[c]
        else:
            c += 1
    for nt, passes, lo, hi in cls:
        rows_cls = 16 * nt * passes
        assert all(pair_len[p] <= rows_cls for p in range(lo, hi)), "a class holds a pair longer than its rows"
        skipping = sum((rows_cls - pair_len[p]) % (16 * nt) >= 17 for p in range(lo, min(hi, n_real)))
        skip = skip0 and 8 * skipping >= hi - lo and skipping > 0
        if hi > lo:
            plan.append(multi_pass(nt, passes, lo, hi, rows_pad - rows_cls, skip))
    return plan, n_groups


def plan_cells(plan):
    return 64 * sum(x.cells for x in plan)


def plan_classes(plan):
    """(kernel, tiles, passes, skip) per launch: what a case table names."""
    return tuple((x.kernel, x.nt, x.passes, x.skip) for x in plan)
