// dtw_filter_plan.hpp -- the launch plan of the unbanded dtw filter: geometry, knobs and plan_filter().
//
// Host only, standard library only: dtw_filter.hip runs the plan (run_launch), tests/cpp/filter_plan_dump.cpp prints it for
// the CPU tests, which hold it against its restatement in tests/filter_plan.py.  plan_filter() decides, from the segment
// lengths alone, which kernel runs on which range of source pairs, with which grid, task chunk and pair block, and how many
// DP cells the launch evaluates; nothing else in the library makes any of these decisions.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ssym {

constexpr int kFilterRecHalfs = 48;      // f16 values per frame record (96 bytes)
constexpr int kFilterWavesPerBlock = 4;
constexpr int kTaskCtrStride = 64;       // the 8 task counters sit in separate 256-byte lines (separate L2 channels)
#ifndef SSYM_SP_ROWBLOCK
#define SSYM_SP_ROWBLOCK 4
#endif
constexpr int kSpRowBlock = SSYM_SP_ROWBLOCK;                    // G: DP rows of the first tile are skipped in blocks of G
constexpr int kSpRing = 4;                                     // staged columns per wave
#ifndef SSYM_SP_OCC_NT2
#define SSYM_SP_OCC_NT2 3        // two-tile tasks at three waves per SIMD (162 registers since the loop copies own their operand registers); 2: tools
#endif
constexpr int kMaxClasses = 10;          // counter sets: three single-pass classes + up to seven multi-pass ones
constexpr int kSmallClass = 128;         // a long class of fewer pairs joins its successor
constexpr int kFilterMaxFrames = 4096;   // source frames the filter takes: beyond, the exact kernel only

// dtw filter geometry (see dtw_filter_kernel.hpp): a source slot holds 16*nt*rb rows, processed by
// one wave in rb passes of nt 32x32 tiles each.
struct FilterShape {
    int nt = 0, rb = 0;
    int rows() const { return 16 * nt * rb; }
};
inline FilterShape filter_shape(int max_frames)
{
    if (max_frames <= 16) return FilterShape{1, 1};
    if (max_frames <= 32) return FilterShape{2, 1};
    if (max_frames <= 48) return FilterShape{3, 1};
    if (max_frames <= kFilterMaxFrames) return FilterShape{4, (max_frames + 63) / 64};
    return FilterShape{};   // beyond the filter's reach: exact kernel only
}
// MFMAs the unbanded filter issues per 32 x 32 tile for a record layout (filter_pieces, ssym_internal.hpp)
// (layout 1 needs dim + 6 slots: frames of 14...26 values fit two planes as well)
inline int filter_mfmas(int pieces, int dim) { return (pieces == 3 || (pieces == 1 && dim + 6 <= 32)) ? 2 : 3; }
// values per frame the filter sees: frames wider than 42 values enter with their first 42 only, which
// makes the filter's cost a LOWER bound of the pair's cost ("wide frames")
inline int filter_dim_used(int dim) { return dim <= 42 ? dim : 42; }

// The knobs of the unbanded launcher (measurements and tests; none changes a result).  The defaults are the product's;
// read_filter_knobs() in dtw_filter.hip fills the others in from the environment, once per filter call.
struct FilterKnobs {
    bool pk = false;            // SSYM_FILTER_PK=1: four-tile launches on the packed-addition kernel (dtw_filter_pk_kernel.hpp)
    bool sp = true;             // SSYM_FILTER_SP=0: single-pass launches stay on dtw_filter_kernel
    int spMultipair = 1;        // SSYM_SP_MULTIPAIR: 0 never, 1 where the multi-pair tasks still fill the chip, 2 whatever the size
    int spPairBlock = -1;       // SSYM_SP_PAIRBLOCK: source pairs per block of the sp task order; 0 one block; -1 about 1 MB of records
    bool wg = true;             // SSYM_FILTER_WG=0: no dtw_filter_wg_kernel
    bool skip0 = true;          // SSYM_FILTER_SKIP0=0: no SKIP0 instantiation
    bool nt8 = false;           // SSYM_FILTER_NT8: sets of 65...128 frames as one 128-row pass (experiment of record)
    bool oneLaunch = false;     // SSYM_FILTER_ONE_LAUNCH: the set's shape for every pair
    bool longClasses = true;    // SSYM_FILTER_LONG_CLASSES=0: the set's shape for every pair beyond 48 frames
    int pruneNt = 0;            // SSYM_PRUNE_NT=2|4: the pass height of an abandoning call, pinned
};

struct FilterPlanInput {
    const uint32_t *pairLen = nullptr;      // [srcNPad / 2] frames of the longer member of every source pair, in slot order (ascending; 0: padding pair)
    const uint32_t *groupCols = nullptr;    // [tgtGroups] frames of the longest member of every target group of 32
    uint32_t srcN = 0, srcNPad = 0, framesPad = 0;      // sources, their record slots, rows per slot
    uint32_t tgtN = 0, tgtGroups = 0;
    uint64_t tgtTotalFrames = 0;
    int numCus = 0;
    int ku = 2;                         // operand planes the kernels multiply
    bool abandon = false;               // early abandoning (a pruned search)
    float pruneSwept = 1.0f;            // share of its cells the context's previous abandoning call swept
    FilterKnobs knobs;
};

enum class FilterKernel { Mp, Sp, Generic, GenericSkip0, GenericPrune, Wg, Pk };

// One kernel launch: passes of 16 * nt rows over the source pairs [lo, hi), on the last rows_pad - origin rows of their slots.
struct FilterLaunch {
    FilterKernel kind = FilterKernel::Generic;
    int nt = 0, passes = 0, origin = 0, lo = 0, hi = 0;
    int grid = 0, taskChunk = 0;
    int pairBlock = 0;                  // Mp, Sp: pairs (Mp: tasks' pairs) per block of the task order
    int taskPairs = 0;                  // Mp: tasks per target group
    int occ = 0;                        // workgroups per CU the instantiation is bound to
    int ctrSet = 0;                     // its set of 8 task counters
    unsigned long long cells = 0;       // DP cells per lane it adds to n_filter_cells (an abandoning call counts its own; pk: none)
};

// The launches of one unbanded filter call, in order.
//
// Record slots are ordered by segment length, so source pairs fall into contiguous CLASSES by the 16-row tiles their
// longer member needs.  Pairs that fit one, two or three tiles run a single pass of exactly that many (on the last rows
// of their end-aligned slots) -- a dictionary of 8...40-frame segments otherwise paid 48 rows for every pair --, the
// rest the set's own shape or the long classes below.  One launch per non-empty class.
inline std::vector<FilterLaunch> plan_filter(const FilterPlanInput &in)
{
    const FilterKnobs &kn = in.knobs;
    const bool abandon = in.abandon;
    const int nPairs = (int)in.srcNPad / 2;
    const int nRealPairs = (int)((in.srcN + 1) / 2);  // pairs behind them hold padding only: they ride with the last class
    const int rowsPad = (int)in.framesPad;
    const int nTgtGroups = (int)in.tgtGroups;
    const uint32_t *const pairLen = in.pairLen;
    // columns per target group: its longest member's (the sp kernels sweep at least their ring)
    unsigned long long colsPlain = 0, colsRing = 0;
    for (int g = 0; g < nTgtGroups; ++g) {
        const uint32_t m = in.groupCols[g];
        colsPlain += m;
        colsRing += std::max<uint32_t>(m, (uint32_t)kSpRing);
    }
    // tasks per grab: several SHORT tasks at a time so that the L2 atomics stay invisible (at 16 frames a
    // task is ~1 us of work), one at a time once a task is long enough to matter for the tail
    // (a task's size by the MEAN target length, not the longest: a ragged set's typical task is what the grab amortises)
    const long meanTgt = in.tgtN ? (long)((in.tgtTotalFrames + in.tgtN - 1) / in.tgtN) : 1;
    auto chunkFor = [&](long rowsPerTask) {
        return (int)std::max(1L, std::min(8L, 8192 / std::max(1L, rowsPerTask * std::max<long>(meanTgt, 1))));
    };
    // persistent grid: 2 workgroups of 4 waves per CU (2 waves per SIMD), a multiple of 8 so that task & 7 is the XCD group
    const int baseBlocks = std::max(8, in.numCus * 2 / 8 * 8);

    // DP rows (per lane; times the columns: cells) the pairs [lo, hi) evaluate, padding included.  rowBlock > 0, the sp
    // kernels: one pass whose leading row blocks of padding are skipped, every pair of a multi-pair task from the task's
    // first row block.  rowBlock = 0, dtw_filter_kernel: leading passes that hold only padding are skipped, and under SKIP0
    // the first pass's empty first tile.
    auto rows = [&](int lo, int hi, int origin, int passRows, int nPasses, int rowBlock, int pairsPerTask, bool skipTile) {
        unsigned long long r = 0;
        for (int sp = lo; sp < hi; ++sp) {
            int longer = (int)pairLen[sp];
            if (pairsPerTask > 1) {
                const int first = lo + (sp - lo) / pairsPerTask * pairsPerTask;
                for (int k = first; k < std::min(first + pairsPerTask, hi); ++k)
                    longer = std::max(longer, (int)pairLen[k]);
            }
            const int r0min = rowsPad - longer;
            if (rowBlock) {
                const int sk = std::min(std::max(r0min - origin, 0), 15) / rowBlock;
                r += (unsigned long long)(passRows - sk * rowBlock);
            } else {
                const int firstPass = std::min(std::max(r0min - origin, 0) / passRows, nPasses - 1);
                r += (unsigned long long)(nPasses - firstPass) * passRows;
                if (skipTile && r0min - (origin + firstPass * passRows) >= 17)
                    r -= 16;
            }
        }
        return r;
    };

    std::vector<FilterLaunch> plan;
    plan.reserve(kMaxClasses);
    // one class: the kernel that serves it, its grid and chunk, its cells
    auto add = [&](int nt, int passes, int origin, int lo, int hi, int ctrSet, bool skipTile = false) {
        if (hi <= lo)
            return;
        FilterLaunch l;
        l.nt = nt, l.passes = passes, l.origin = origin, l.lo = lo, l.hi = hi, l.ctrSet = ctrSet;
        // sources of at most 16 frames (one tile, one pass): three waves per SIMD, see filter_ring() -- 11 %
        // faster there; at 32 frames the gain was within 3 % and cost spills
        // nt == 8 (experiment, SSYM_FILTER_NT8=1): the whole 128-row column of a pair in ONE wave's registers, one wave per
        // SIMD with the whole register file -- no second pass, no hand-off rows
        const int occ = nt == 1 ? 3 : nt == 8 ? 1 : 2;
        const int gridBlocks = baseBlocks / 2 * occ;
        const int nSrcPairs = hi - lo;
        const int nTasks = nSrcPairs * nTgtGroups;            // one wave's 64 pairs each
        const int blocksWanted = (nTasks + kFilterWavesPerBlock - 1) / kFilterWavesPerBlock;
        l.occ = occ;
        l.grid = std::min(gridBlocks, (blocksWanted + 7) / 8 * 8);
        // ... always at least 16 grabs per wave
        l.taskChunk = std::max(1, std::min(chunkFor(16 * nt * passes), nTasks / (l.grid * kFilterWavesPerBlock * 16)));
        const bool single = !abandon && passes == 1 && kn.sp;
        const int mpn = in.ku == 2 ? 3 : 2;       // source pairs per multi-pair task (three operand planes: LDS)
        // (... when the multi-pair tasks still give every wave slot of the chip one: a 284 x 55 search is 96 of them, each
        //  sweeping its group's longest target three pairs wide while nine tenths of the SIMDs idle -- one pair per wave there)
        const long mpTasksWanted = (long)((nSrcPairs + mpn - 1) / mpn) * nTgtGroups;
        if (nt == 4 && !abandon && kn.pk) {
            l.kind = FilterKernel::Pk;
        } else if (nt == 1 && single && kn.spMultipair != 0 &&
                   (kn.spMultipair == 2 || mpTasksWanted >= (long)gridBlocks / occ * 2 * kFilterWavesPerBlock)) {
            l.kind = FilterKernel::Mp;
            l.occ = 2;
            l.taskPairs = (nSrcPairs + mpn - 1) / mpn;
            const int mpTasks = l.taskPairs * nTgtGroups;
            l.grid = std::min(gridBlocks / occ * 2, ((mpTasks + kFilterWavesPerBlock - 1) / kFilterWavesPerBlock + 7) / 8 * 8);
            l.taskChunk = std::max(1, std::min(chunkFor(16 * mpn), mpTasks / std::max(1, l.grid * kFilterWavesPerBlock * 16)));
            // source pairs per block of the task order: about 1 MB of their records (an XCD's L2 holds 4 MB: the block, the
            // XCD's target groups, the cost rows being written)
            const int pairBlock = kn.spPairBlock > 0    ? kn.spPairBlock
                                  : kn.spPairBlock == 0 ? l.taskPairs
                                                        : std::max(16, (1 << 20) / (mpn * 2 * 16 * kFilterRecHalfs * 2));
            l.pairBlock = std::min(pairBlock, std::max(l.taskPairs, 1));
            l.cells = rows(lo, hi, origin, 16, 1, kSpRowBlock, mpn, false) * colsRing;
        } else if (nt <= 3 && (in.ku == 2 || nt <= 2) && single) {
            // (with three operand planes the sp kernel's LDS -- ring and staging block -- admits two workgroups per CU up to two tiles)
            l.kind = FilterKernel::Sp;
            l.occ = (nt == 1 && in.ku == 2) ? 3 : (nt == 2 && in.ku == 2) ? SSYM_SP_OCC_NT2 : 2;
            l.grid = std::min(gridBlocks / occ * l.occ, (blocksWanted + 7) / 8 * 8);
            const int pairBlock = kn.spPairBlock > 0    ? kn.spPairBlock
                                  : kn.spPairBlock == 0 ? nSrcPairs
                                                        : std::max(16, (1 << 20) / (2 * 16 * nt * kFilterRecHalfs * 2));
            l.pairBlock = std::min(pairBlock, std::max(nSrcPairs, 1));
            l.cells = rows(lo, hi, origin, 16 * nt, 1, kSpRowBlock, 1, false) * colsRing;
        } else if ((nt == 3 || nt == 4) && skipTile && !abandon) {
            l.kind = FilterKernel::GenericSkip0;
            l.cells = rows(lo, hi, origin, 16 * nt, passes, 0, 1, true) * colsPlain;
        } else if (abandon) {
            l.kind = FilterKernel::GenericPrune;
        } else {
            // Equal-pass launches: one ring of target columns per workgroup (dtw_filter_wg_kernel.hpp), its four waves on four
            // consecutive pairs of one target group.  Its barriers need every wave of a workgroup to run the same passes over
            // the same columns: whole blocks of four pairs, none of them padding only (such a pair would start at the last
            // pass), and pass 0 holding a row of the shortest pair -- pairs ascend by length, so of pair lo.
            // (grid and chunk count waves' tasks; a workgroup's task is four of them, so both stay what they are)
            const bool wg = nt == 4 && kn.wg && !skipTile && nSrcPairs % 4 == 0 && hi <= nRealPairs && in.srcN % 2 == 0 &&
                            origin + 16 * nt > rowsPad - (int)pairLen[lo];
            l.kind = wg ? FilterKernel::Wg : FilterKernel::Generic;
            l.cells = rows(lo, hi, origin, 16 * nt, passes, 0, 1, false) * colsPlain;
        }
        plan.push_back(l);
    };

    auto firstAbove = [&](uint32_t frames) {        // first real pair whose longer member exceeds `frames`
        return (int)(std::upper_bound(pairLen, pairLen + nRealPairs, frames) - pairLen);
    };
    // the set's own shape, from its longest segment: the last real slot's
    const FilterShape setShape = filter_shape(nRealPairs ? (int)pairLen[nRealPairs - 1] : 0);
    const int topTiles = setShape.nt;               // (4: multi-pass)
    int bound[4] = {0, 0, 0, 0};                    // bound[c]: first pair that needs more than c tiles
    for (int c = 1; c < 4; ++c)
        bound[c] = c >= topTiles ? nPairs : kn.oneLaunch ? 0 : firstAbove(16u * c);
    // the single-pass classes (a set of at most 48 frames: the last one is its own shape, from row 0)
    for (int c = 1; c <= std::min(topTiles, 3); ++c)
        add(c, 1, rowsPad - 16 * c, bound[c - 1], bound[c], c - 1);
    if (topTiles < 4)
        return plan;

    // Early abandoning: the work of a pruned task is about the area where D <= threshold, counted in whole
    // row passes x columns, so lower passes waste less: with 32-row passes the headline grid takes 3.1 ms
    // instead of 4.6.  But a task that cannot be cut short pays two more hand-offs per 128 rows (+17 % on
    // data without close pairs).  Results do not depend on the pass height, so it follows the data: 32 rows
    // when the previous pruned call on this context swept less than a quarter of its cells, 64 otherwise
    // (and on the first call).  SSYM_PRUNE_NT=2|4 pins it for measurements.
    const int pinned = abandon ? kn.pruneNt : 0;
    const int pruneNt = pinned == 2 || pinned == 4 ? pinned : (in.pruneSwept < 0.25f ? 2 : 4);
    if (abandon && pruneNt == 2) {
        add(2, setShape.rb * 2, 0, bound[3], nPairs, 3);
    } else if (kn.nt8 && setShape.rb == 2 && !abandon) {
        add(8, 1, 0, bound[3], nPairs, 3);
    } else if (abandon || !kn.longClasses || kn.oneLaunch) {
        add(4, setShape.rb, 0, bound[3], nPairs, 3);
    } else {
        // Sources beyond 48 frames, ragged: a pair pays whole row passes, so a 70-frame source swept in passes of 64
        // rows pays 128 -- but 96 in passes of 48.  The pairs (ascending by length) are cut into classes by the shape
        // that pads them least, passes of 64 rows (four tiles) or of 48 (three), the last rows of their end-aligned
        // slots as for the short classes; a class of fewer than kSmallClass pairs rides with the next one (any larger
        // shape holds it), and so does everything beyond the counter sets there are.  Equal lengths: one class, the set's
        // own shape.
        struct LongClass { int nt, passes, lo, hi; };
        LongClass cls[kMaxClasses];
        int nCls = 0;
        auto best = [&](uint32_t len, int &nt, int &passes) {
            const int p4 = (int)((std::max(len, 1u) + 63) / 64), p3 = (int)((std::max(len, 1u) + 47) / 48);
            if (48 * p3 < 64 * p4) { nt = 3; passes = p3; } else { nt = 4; passes = p4; }
        };
        for (int sp = bound[3]; sp < nPairs;) {
            int nt, passes;
            best(sp < nRealPairs ? pairLen[sp] : 0u, nt, passes);
            // the run of pairs this shape is the best for: up to the first pair longer than its rows
            const int end = std::max(sp + 1, std::min(nPairs, sp < nRealPairs ? firstAbove((uint32_t)(16 * nt * passes)) : nPairs));
            cls[nCls++] = LongClass{nt, passes, sp, end == nRealPairs ? nPairs : end};     // (padding pairs ride with the last real one)
            sp = cls[nCls - 1].hi;
            if (nCls == kMaxClasses - 3 && sp < nPairs) {                                   // no counter set left: the set's own shape takes the rest
                cls[nCls - 1] = LongClass{4, setShape.rb, cls[nCls - 1].lo, nPairs};
                break;
            }
        }
        // small classes join their successor (whose rows are at least theirs); the last one keeps its own
        for (int c = 0; c + 1 < nCls;) {
            if (cls[c].hi - cls[c].lo < kSmallClass) {
                cls[c + 1].lo = cls[c].lo;
                for (int k = c; k + 1 < nCls; ++k)
                    cls[k] = cls[k + 1];
                --nCls;
            } else {
                ++c;
            }
        }
        for (int c = 0; c < nCls; ++c) {
            // at least an eighth of the class's pairs leave the first tile of their first pass empty: the variant that
            // skips such tiles' cells (equal lengths and classes that fill their rows keep the plain kernel)
            const int rowsCls = 16 * cls[c].nt * cls[c].passes;
            int skipping = 0;
            for (int sp = cls[c].lo; sp < std::min(cls[c].hi, nRealPairs); ++sp)
                skipping += (rowsCls - (int)pairLen[sp]) % (16 * cls[c].nt) >= 17;
            const bool skipTile = kn.skip0 && 8 * skipping >= cls[c].hi - cls[c].lo && skipping > 0;
            add(cls[c].nt, cls[c].passes, rowsPad - rowsCls, cls[c].lo, cls[c].hi, 3 + c, skipTile);
        }
    }
    return plan;
}

}  // namespace ssym
