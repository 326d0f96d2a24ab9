// dtw_filter_wg2_kernel.hpp -- sibling of dtw_filter_wg_kernel (dtw_filter_wg_kernel.hpp) for launches of exactly TWO row
// passes: the two passes of a source pair run at the same time on two waves of the workgroup, one column group apart, and
// the bottom row of the upper pass reaches the lower one through LDS.  (Included by dtw_filter.hip.)
//
// Why: in dtw_filter_wg_kernel a wave runs pass 0 of its pair, stores the bottom row of its block to a hand-off row in
// global memory (one 4-byte buffer_store per lane and column) and reads it back in pass 1 (one 16-byte LDS-DMA per four
// columns): 8.6 GB written and 8.6 GB read back per headline launch, rows that live for a whole pass and so leave the L2.
// Here nothing of the hand-off leaves the CU: no hand-off row, no buffer_store, no hand-off DMA, no vmcnt wait for a top value.
// The cells, the MFMAs, the record layouts, rowOrigin, outScale and the `res` pick at column fb - 1 are dtw_filter_kernel's;
// per cell the same operations in the same order, so the filter matrix keeps its bits.
// Measured on the headline (LAB.md 5.1): main_ms 31.90 -> 30.94 (-3.0 %; the ceiling, the same kernel with its hand-off
// compiled out, was -2.85 %), 9.07 -> 0.07 GB written and 25.5 -> 6.6 GB through the fabric per launch, the same 17.5
// elapsed cycles per wave-cell at 2.35 instead of 2.32 GHz; 3.21 VALU instructions per wave-cell where the parent has 3.19.
// Launches whose lengths do not differ take the UNIFORM instantiation (described above the kernel): 3.16 instructions and
// 17.29 cycles per wave-cell, ms_per_step 32.01 -> 31.65 (-1.1 %).  What follows describes the general text.
//
//   * Columns.  A group always runs its four columns: the columns behind a task's last one (at most three; none when nCols
//     is a multiple of four) work on the clamped last column and nothing reads what they compute -- the follower picks `res`
//     at column fb - 1 < nCols, and the task's column arrays are set up anew at its successor's start.  (A per-column test
//     in this loop costs every column a copy of the accumulator: LAB.md 5.1.)
//   * Roles.  The four waves are two source pairs x two roles: wave 2 p is the LEADER of pair p (pass 0, rows 0...63 of the
//     launch), wave 2 p + 1 its FOLLOWER (pass 1, rows 64...127).  A workgroup task is (two consecutive source pairs, target
//     group).  A wave keeps its role for the whole launch; the two tick loops are written separately and branched once at
//     kernel entry.  The leader reads no top values (its `up` is +inf; D(r0 - 1, -1) = 0 enters through prevTop and the
//     column arrays, as in every pass), picks no `res` and stores no cost; the follower writes no hand-off.
//   * Ticks.  Time is counted in column groups of four, one s_barrier per TICK.  The workgroup runs ONE sequence of ITEMS
//     (task, column group g of the task), the tasks in the order they were taken, the groups of a task in order; a task of
//     nCols columns has max(1, ceil(nCols / 4)) groups (a target group of padding only, nCols = 0, keeps one group without
//     a column, so that its +inf costs are written like any other task's).  At tick V the leaders run item V, the followers
//     item V - 1, and all four waves stage the columns of item V + 2 (wave w column 4 g + w).  The sequence runs on across
//     tasks: the leader starts the next task's group 0 in the tick in which the follower finishes the last group of the
//     current one -- no tick is lost per task.  An item may be EMPTY (a bubble); that happens only where the sequence waits
//     for the first task of an XCD range (one tick per range: the stager learns that a range is spent from the record it
//     reads, and asks the next range's counter in the same tick) and at the start and the end of the kernel.
//   * Tasks.  They come from the same eight per-XCD counters and ranges as dtw_filter_wg_kernel's, counted in blocks of FOUR
//     pairs (nSrcBlocks = nSrcPairs / 4, taskChunk blocks per grab: the plan's figures); a block is two tasks of this kernel,
//     pairs 4 b, 4 b + 1 and 4 b + 2, 4 b + 3.  The stager (every wave runs the same copy of it) is at item V + 2; in the tick
//     in which it enters the LAST group of its task it requests the next task, and wave 0 -- the front end -- delivers it
//     within that tick: the counter's atomic at the start of the tick (only when the grabbed chunk is used up), the task's
//     target group and its lengths' load (an LDS-DMA of 4 bytes per lane) behind the tick's second column, the reduction to nCols and a RECORD
//     {target group, first pair, nCols} in LDS behind the fourth.  The barrier that opens the next tick publishes the record
//     and the stager of every wave reads it there: the id of a task is fetched one tick before its first column is staged,
//     three ticks before its first cell.  Two records alternate: record n + 2 is written at the end of a tick that every
//     wave entered after reading record n.
//   * Hand-off.  After each column the leader writes its bottom (4 bytes per lane) into an LDS buffer of 4 columns x 256 B
//     of its pair, buffer V & 1 at tick V.  The follower reads its top values from buffer (V - 1) & 1 at tick V, i.e. after
//     the barrier that opens its tick -- which the leader passed with s_waitcnt lgkmcnt(0) behind its writes --, the first
//     column's right behind the barrier, the others' one column ahead.  The leader writes that buffer again in tick V + 1,
//     behind that tick's barrier, which the follower reaches with its reads returned (lgkmcnt(0) again).
//   * Ring.  One ring of 16 column slots (four groups) per workgroup, as in dtw_filter_wg_kernel; the slots of a group follow
//     the TICK, item V in the four slots 4 (V & 3) ..., the global address follows (target group of the item's task, g).  At
//     tick V the groups in use are V - 1 (followers), V (leaders; the followers fetch its first column at their last one),
//     V + 1 (the leaders fetch its first column) and V + 2 (being staged, into the slots of V - 2): exactly four.  The
//     staging DMAs are issued BEHIND the barrier that opens tick V: every wave has then left tick V - 1, the last one in
//     which a follower read group V - 2.  Each wave waits for its own DMAs with s_waitcnt vmcnt in front of the barrier of
//     tick V + 1, after which group V + 2 is complete for every wave; its first reader is the leader's last column of tick
//     V + 1.  A staged column serves both passes of both pairs: KU DMAs per wave and tick, a quarter of dtw_filter_wg_kernel's per pair and pass.
//   * Task starts.  The column pipeline of a wave (the operands of column j + 1 fetched and the first MFMA chain of column
//     j + 1 issued during column j) is not carried over a task boundary: at group 0 of a task the wave loads its A operands
//     and lengths, sets up both column arrays and prevTop, fetches column 0 from the ring and issues its first chain.
//   * vmcnt.  A wave's vector-memory operations in program order, per tick: [wave 0, a request without chunk left: the
//     counter's atomic], the KU staging DMAs, [group 0 of a task: the A operand and length loads], [wave 0, a request: the
//     lengths' DMA of the next task, waited for with vmcnt(0) two columns later, where the record is made], [follower, last group of a task: the cost store].  Everything that returns a value
//     into registers is waited for by the compiler's own count where the value is used, inside the tick.  What is left for
//     the barrier is the wave's staging DMAs: s_waitcnt vmcnt(0) in front of every barrier, except that a follower whose
//     last operation is a cost store waits with vmcnt(1) -- the store is the youngest operation, the DMAs are older, and
//     nothing reads the cost matrix in this launch.  All of these were issued a whole tick (four columns) earlier.
//   * Barriers: one per tick, nothing else.  INVARIANT: every wave of a workgroup executes the same number of barriers,
//     although leaders and followers run different code.  The tick loop of either role ends when the stager has seen all
//     eight ranges spent and the four items V - 1 ... V + 2 are empty; the stager's state -- the items, the range, the
//     request -- is a function of the records alone, every wave reads the same records in the same ticks, and nCols is the
//     task's (the front end reduces the lengths of the task's target group once and every wave takes the record's).  So
//     ticks per task are the same in all four waves, and no wave-dependent condition encloses the barrier: the
//     role- and wave-dependent branches (leader or follower columns, the front end in wave 0, a task start, a cost store)
//     all lie between two barriers and hold none.
//   * LDS: 16 slots x 3 KB + 2 pairs x 2 buffers x 1 KB + 2 records + 256 B for the front end = 52.3 KB per workgroup (dtw_filter_wg_kernel: 56 KB).
#pragma once
#include "dtw_filter_kernel.hpp"

namespace ssym {

#define SSYM_FILTER_SBASE(P_) asm volatile("" : "+s"(P_))
#define SSYM_FILTER_LANEOFF(V_) asm volatile("" : "+v"(V_))

constexpr int kFilterWg2Ring = 16;                       // column slots per workgroup: four groups of four columns
constexpr int kFilterWg2HandBytes = 2 * 2 * 1024;        // two pairs x two buffers of 4 columns x 64 lanes x 4 B
constexpr int kFilterWg2RecBytes = 2 * 16;               // two task records of four words
constexpr int kFilterWg2LenBytes = 256;                  // the front end's landing place for a target group's lengths
constexpr int kFilterWg2Lds = kFilterWg2Ring * kFilterSlotBytes + kFilterWg2HandBytes + kFilterWg2RecBytes + kFilterWg2LenBytes;
// s_waitcnt vmcnt(n) lgkmcnt(0): in front of a tick's barrier (the wave's staging DMAs have landed, its LDS writes are
// done and its LDS reads have returned)
constexpr int wait_vmcnt_lgkm0(int n) { return wait_vmcnt(n) & ~0x0F00; }

// Column 0 of a task whose D(., -1) is +inf in every row of the pass (UNIFORM): dp_column without the column array it would
// read and without its v_min3 -- min3(up, +inf, +inf) is `up`, so D(i, 0) = c(i, 0) + D(i - 1, 0), started from `up`.
template <int NT, bool SQ, int KU>
__device__ __forceinline__ float dp_column_first(const half8 (&A)[NT][KU], const half8 (&Bc)[KU], const half8 (&Bn)[KU],
                                                 f32x16 &acc, float up, float (&Lw)[NT * 16])
{
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        f32x16 accn;
        if (T + 1 < NT)
            accn = mfma_tile<KU>(A[T + 1], Bc);
        else
            accn = mfma_tile<KU>(A[0], Bn);   // first tile of the next column
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float x = acc[r];
            const float c = SQ ? __builtin_fabsf(x) : __builtin_amdgcn_sqrtf(__builtin_fabsf(x));
            const float cur = c + up;
            Lw[T * 16 + r] = cur;
            up = cur;
        }
        acc = accn;
    }
    return up;
}

// UNIFORM = true: the instantiation for launches whose lengths do not differ, picked by the launcher (dtw_filter.hip
// run_kernel), which has checked that
//   * every target of the call is real (mPad targets, no padding) and has uniF frames, uniF >= 4 and a multiple of four;
//   * every source of the launch's pairs has uniFa frames, 64 < uniFa <= 128, and the launch's rows are the slots' last 128
//     (srcRows - rowOrigin == 128).
// What the lengths cost the general text does not exist here:
//   * Stager.  Every task has G = uniF / 4 groups and every group four real columns: an item is {target group, first pair,
//     g}, the last group is g == G - 1, the staged column 4 g + wave needs no clamp.  Tick, request and range counters are
//     scalar and the loop ends on scalar compares.
//   * Front end.  No lengths are fetched or reduced; a record is {target group, first pair}, written in one step behind
//     the tick's second column.  Two records alternate as before: record n + 2 is written behind the barrier of a tick that
//     every wave entered after reading record n.
//   * Follower.  No target length is loaded and no column selects: `res` is the bottom of column 3 of group G - 1.
//   * Task start.  No source length is loaded: r0 = srcRows - uniFa.  The follower's rows all lie below r0 (uniFa > 64), so
//     its D(., -1) is +inf throughout and column 0 is dp_column_first from the leader's bottom; with uniFa == 128 the
//     leader's r0 is its first row, D(r0 - 1, -1) = 0 enters as `up` and its column 0 is dp_column_first from 0.  Neither
//     column array is initialised: column 0 writes the one column 1 reads, column 1 the other.  A leader with uniFa < 128
//     keeps the general set-up and the general column 0 behind one wave-uniform branch.
//   * Same bits: the general text computes column 0's cells as c + min3(up, +inf, +inf) -- v_min3_f32 returns `up`, the
//     costs are finite (a documented limit of the filter) -- and the leader's first real cell as c + min3(+inf, 0, +inf)
//     = c + 0; dp_column_first adds the same two operands in the same order.
//   * Barriers.  INVARIANT, restated: every wave of a workgroup executes the same number of barriers.  The stager's state
//     -- items, ranges spent, requests -- is a function of the records and of the kernel argument uniF alone; every wave
//     reads the same records in the same ticks, so ticks per task (G) and the tick in which the loop ends are the same in
//     all four waves, and no role- or wave-dependent branch (leader or follower columns, the front end in wave 0, a task
//     start, the leader's general set-up, a cost store) holds a barrier.
//   * LDS: the general kernel's less the 256 B of the lengths.
// Ring, hand-off buffers, the vmcnt immediates that remain, MFMAs, record layouts, outScale, task counters and XCD ranges
// are the general text's.  UNIFORM = false is that text, unchanged.
template <bool SQ, int KU, bool UNIFORM = false>
__global__ __launch_bounds__(64 * kFilterWavesPerBlock, 2) void dtw_filter_wg2_kernel(
    const _Float16 *__restrict__ srcRec, const _Float16 *__restrict__ tgtRec,
    const int *__restrict__ srcLen, const int *__restrict__ tgtLen, int srcRows,
    int tgtFramesPad, int mPad, int nSrcBlocks, int taskChunk, float outScale,
    unsigned *__restrict__ taskCtr, float *__restrict__ cmat, int rowOrigin, int spBase, int uniF = 0, int uniFa = 0)
{
    static_assert(KU == 2 || KU == 3, "two or three operand planes per column");
    static_assert(kFilterWavesPerBlock == 4, "two pairs x two roles; a column group is one column per wave");
   if constexpr (UNIFORM) {
    constexpr int NT = 4;
    constexpr int REC = kFilterRecHalfs;
    constexpr int BR = NT * 16;            // rows per pass
    const float INF = __builtin_inff();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int follower = wave & 1;
    const int col = lane & 31;
    const int half = lane >> 5;
    uint32_t laneOff16 = lane * 16;
    __shared__ __attribute__((aligned(16))) char lds[kFilterWg2Lds - kFilterWg2LenBytes];
    char *const ring = lds;
    char *const hand = lds + kFilterWg2Ring * kFilterSlotBytes + (wave >> 1) * 2048;      // the pair's two buffers
    volatile int *const record = reinterpret_cast<volatile int *>(lds + kFilterWg2Ring * kFilterSlotBytes + kFilterWg2HandBytes);

    const unsigned nGroups = (unsigned)mPad >> 5;
    const int lastG = (uniF >> 2) - 1;     // the last group of every task

    // ---- the stager: items V - 1 ... V + 2 (g < 0: empty), the same in every wave of the workgroup ----
    struct Item { int tg, sp0, g; };
    Item im1{0, 0, -1}, i0{0, 0, -1}, i1{0, 0, -1}, i2{0, 0, -1};
    unsigned hop = 0;                      // XCD ranges the stager has seen spent
    unsigned requests = 0;                 // records requested so far
    bool pending = false;                  // a record was requested in the tick before
    bool request = false;                  // ... in this tick
    unsigned tick = 0;
    // ---- the front end (wave 0): the grabbed chunk of four-pair blocks [feGi, feEnd), the half of block feGi that is next ----
    unsigned feGi = 0, feEnd = 0, feHalf = 0, feXcd = 0, feRange = 0;
    bool feOn = false, feAtomic = false;
    unsigned feTk = 0;

    // opens tick `tick`, as in the general text: the barrier, the items, the request, the staging of item V + 2
    auto open_tick = [&](bool storeYoungest) __attribute__((always_inline)) -> bool {
        if (storeYoungest)
            __builtin_amdgcn_s_waitcnt(wait_vmcnt_lgkm0(1));
        else
            __builtin_amdgcn_s_waitcnt(wait_vmcnt_lgkm0(0));
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        im1 = i0;
        i0 = i1;
        i1 = i2;
        if (i2.g >= 0 && i2.g != lastG) {
            ++i2.g;
        } else if (pending) {
            const unsigned slot = (requests - 1u) & 1u;
            const int tg = __builtin_amdgcn_readfirstlane(record[4 * slot + 0]);
            const int sp0 = __builtin_amdgcn_readfirstlane(record[4 * slot + 1]);
            if (tg >= 0) {
                i2 = Item{tg, sp0, 0};
            } else {
                i2.g = -1;
                ++hop;                     // the range is spent
            }
        } else {
            i2.g = -1;
        }
        pending = false;
        if (hop >= 8u && (im1.g & i0.g & i1.g & i2.g) < 0)
            return false;
        request = hop < 8u && (i2.g < 0 || i2.g == lastG);
        if (request) {
            pending = true;
            ++requests;
        }
        feOn = request && wave == 0;
        if (feOn) {
            // front end, step 1: a new chunk from the range's counter when the grabbed one is used up
            feXcd = (blockIdx.x + hop) & 7u;
            feRange = feXcd < nGroups ? ((nGroups - feXcd + 7u) >> 3) * (unsigned)nSrcBlocks : 0u;
            feAtomic = feGi >= feEnd;
            if (feAtomic && lane == 0)
                feTk = atomicAdd(&taskCtr[feXcd * kTaskCtrStride], (unsigned)taskChunk);
        }
        if (i2.g >= 0) {
            // this wave's column of item V + 2: column 4 g + wave of its target group (a real column) -> slot 4 ((V + 2) & 3) + wave
            const int cc = 4 * i2.g + wave;
            char *slot = ring + ((4 * (tick + 2u) + (unsigned)wave) & (unsigned)(kFilterWg2Ring - 1)) * kFilterSlotBytes;
            const char *gb = reinterpret_cast<const char *>(tgtRec) +
                             ((size_t)(unsigned)i2.tg * (unsigned)tgtFramesPad + (unsigned)cc) * (kTgtFrameHalfs * 2);   // wave-uniform, kept scalar
            SSYM_FILTER_SBASE(gb);
            SSYM_FILTER_LANEOFF(laneOff16);
            const __attribute__((address_space(1))) void *gp =
                (const __attribute__((address_space(1))) void *)(gb + laneOff16);
            __attribute__((address_space(3))) void *lp = (__attribute__((address_space(3))) void *)slot;
            __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
            __builtin_amdgcn_global_load_lds(gp, lp, 16, 1024, 0);
            if (KU == 3)
                __builtin_amdgcn_global_load_lds(gp, lp, 16, 2048, 0);
        }
        asm volatile("" ::: "memory");
        return true;
    };
    // front end, step 2 (behind the tick's second column): the task that is next, and its record
    auto front_end = [&]() __attribute__((always_inline)) {
        if (feOn) {
            if (feAtomic) {
                feGi = (unsigned)__builtin_amdgcn_readfirstlane((int)feTk);
                feEnd = min(feGi + (unsigned)taskChunk, feRange);
                feHalf = 0;
            }
            int tg = -1, sp0 = 0;
            if (feGi < feEnd) {
                const unsigned lin = feRange - 1u - feGi;             // position in the XCD's range, walked from its end
                tg = (int)(feXcd + 8u * (lin / (unsigned)nSrcBlocks));
                sp0 = spBase + 4 * (int)(lin % (unsigned)nSrcBlocks) + 2 * (int)feHalf;
                feHalf ^= 1u;
                if (feHalf == 0)
                    ++feGi;
            } else {
                feGi = feEnd = feHalf = 0;  // the next range starts with a grab
            }
            const unsigned slot = (requests - 1u) & 1u;
            if (lane == 0) {
                record[4 * slot + 0] = tg;
                record[4 * slot + 1] = sp0;
            }
        }
    };
    // B operands of the column in slot `s` of the ring
    auto fetch = [&](unsigned s, half8 (&B)[KU]) __attribute__((always_inline)) {
        const char *slot = ring + (s & (unsigned)(kFilterWg2Ring - 1)) * kFilterSlotBytes;
#pragma unroll
        for (int m = 0; m < KU; ++m)
            B[m] = *reinterpret_cast<const half8 *>(slot + m * 1024 + lane * 16);
    };

    // the column state of the wave's pass: lives from group 0 of a task to its last group
    half8 A[NT][KU];
    float L0[BR], L1[BR];
    half8 B0[KU], B1[KU];
    f32x16 acc;
    float prevTop = INF;
    // a task starts (group 0): A operands of the pass, column 0 from the ring (ring group vg) and its first MFMA chain
    auto start_task = [&](const Item &it, int rowBase, unsigned vg) __attribute__((always_inline)) {
        const int sp = it.sp0 + (wave >> 1);
        int ln = lane;
        asm volatile("" : "+v"(ln));       // (the lane's part of the address is worked out here, not kept in registers across the ticks)
        const int arow = ln & 31;
        const int a_src = 2 * sp + ((arow >> 2) & 1);
        const int a_frm = rowBase + (arow & 3) + 4 * (arow >> 3);
        const _Float16 *abase = srcRec + ((size_t)a_src * srcRows + a_frm) * REC + (ln >> 5) * 24;
#pragma unroll
        for (int T = 0; T < NT; ++T)
            load_rec<KU>(abase + (size_t)T * kFilterRowsPerTile * REC, A[T]);
        fetch(4u * vg, B0);
        acc = mfma_tile<KU>(A[0], B0);
    };

    if (!follower) {
        // ================= leader: pass 0, item V at tick V, bottoms into hand-off buffer V & 1 =================
        float up = INF;
        asm volatile("" : "+v"(up));       // (kept a register: the cells' v_min3 reads it like any top value)
        const int zeroRow = srcRows - uniFa - 1 - rowOrigin;      // row of the virtual D(r0 - 1, -1) = 0; -1: above the pass
        for (;; ++tick) {
            if (!open_tick(false))
                break;
            if (i0.g >= 0) {
                const unsigned vg = tick & 3u;
                char *const handW = hand + (tick & 1u) * 1024 + lane * 4;
                auto column = [&](int q) __attribute__((always_inline)) {
                    const float diag = prevTop;
                    prevTop = up;
                    float bottom;
                    if ((q & 1) == 0) {
                        fetch(4u * vg + q + 1, B1);
                        bottom = dp_column<NT, SQ, KU>(A, B0, B1, acc, up, diag, L0, L1);
                    } else {
                        fetch(4u * vg + q + 1, B0);
                        bottom = dp_column<NT, SQ, KU>(A, B1, B0, acc, up, diag, L1, L0);
                    }
                    *reinterpret_cast<float *>(handW + q * 256) = bottom;          // top boundary of the follower's pass
                };
                if (i0.g == 0) {
                    start_task(i0, rowOrigin, vg);
                    prevTop = INF;
                    if (zeroRow >= 0) {
                        // sources shorter than the launch's rows: the general set-up and the general column 0
                        int z = zeroRow;
                        asm volatile("" : "+s"(z));        // (set up here, not once in front of the loop and kept in 64 registers)
#pragma unroll
                        for (int i = 0; i < BR; ++i) {
                            L0[i] = (i == z) ? 0.0f : INF;
                            L1[i] = L0[i];
                        }
                        column(0);
                    } else {
                        fetch(4u * vg + 1, B1);
                        const float bottom = dp_column_first<NT, SQ, KU>(A, B0, B1, acc, 0.0f, L1);
                        *reinterpret_cast<float *>(handW) = bottom;
                    }
                } else {
                    column(0);
                }
                column(1);
                front_end();
                column(2);
                column(3);
            } else {
                front_end();
            }
        }
    } else {
        // ================= follower: pass 1, item V - 1 at tick V, tops from hand-off buffer (V - 1) & 1 =================
        bool stored = false;               // the wave's youngest vector-memory operation is a cost store
        for (;; ++tick) {
            if (!open_tick(stored))
                break;
            stored = false;
            if (im1.g >= 0) {
                const unsigned vg = (tick + 3u) & 3u;
                const char *const handR = hand + ((tick + 1u) & 1u) * 1024 + lane * 4;
                float topN = *reinterpret_cast<const float *>(handR);           // the group's first column: written in the tick before
                float bottom = INF;
                auto column = [&](int q) __attribute__((always_inline)) {
                    const float up = topN;
                    const float diag = prevTop;
                    prevTop = up;
                    if (q < 3)
                        topN = *reinterpret_cast<const float *>(handR + (q + 1) * 256);
                    if ((q & 1) == 0) {
                        fetch(4u * vg + q + 1, B1);
                        bottom = dp_column<NT, SQ, KU>(A, B0, B1, acc, up, diag, L0, L1);
                    } else {
                        fetch(4u * vg + q + 1, B0);
                        bottom = dp_column<NT, SQ, KU>(A, B1, B0, acc, up, diag, L1, L0);
                    }
                };
                if (im1.g == 0) {
                    start_task(im1, rowOrigin + BR, vg);
                    const float up = topN;
                    prevTop = up;
                    topN = *reinterpret_cast<const float *>(handR + 256);
                    fetch(4u * vg + 1, B1);
                    bottom = dp_column_first<NT, SQ, KU>(A, B0, B1, acc, up, L1);
                } else {
                    column(0);
                }
                column(1);
                column(2);
                column(3);
                if (im1.g == lastG) {
                    const int sp = im1.sp0 + (wave >> 1);
                    cmat[(size_t)(2 * sp + half) * mPad + 32 * im1.tg + col] = bottom * outScale;      // D(fa-1, fb-1)
                    stored = true;
                }
            }
        }
    }
   } else {
    constexpr int NT = 4;
    constexpr int REC = kFilterRecHalfs;
    constexpr int BR = NT * 16;            // rows per pass
    const float INF = __builtin_inff();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int follower = wave & 1;         // role: 0 leader (pass 0), 1 follower (pass 1)
    const int col = lane & 31;
    const int half = lane >> 5;
    uint32_t laneOff16 = lane * 16;
    __shared__ __attribute__((aligned(16))) char lds[kFilterWg2Lds];
    char *const ring = lds;
    char *const hand = lds + kFilterWg2Ring * kFilterSlotBytes + (wave >> 1) * 2048;      // the pair's two buffers
    volatile int *const record = reinterpret_cast<volatile int *>(lds + kFilterWg2Ring * kFilterSlotBytes + kFilterWg2HandBytes);

    char *const lenBuf = lds + kFilterWg2Ring * kFilterSlotBytes + kFilterWg2HandBytes + kFilterWg2RecBytes;
    uint32_t laneOff4 = lane * 4;

    const unsigned nGroups = (unsigned)mPad >> 5;

    // ---- the stager: items V - 1 ... V + 2 (g < 0: empty), the same in every wave of the workgroup ----
    struct Item { int tg, sp0, nCols, g; };
    Item im1{0, 0, 0, -1}, i0{0, 0, 0, -1}, i1{0, 0, 0, -1}, i2{0, 0, 0, -1};
    unsigned hop = 0;                      // XCD ranges the stager has seen spent
    unsigned requests = 0;                 // records requested so far
    bool pending = false;                  // a record was requested in the tick before
    bool request = false;                  // ... in this tick
    unsigned tick = 0;
    // ---- the front end (wave 0): the grabbed chunk of four-pair blocks [feGi, feEnd), the half of block feGi that is next ----
    unsigned feGi = 0, feEnd = 0, feHalf = 0, feXcd = 0, feRange = 0;
    bool feOn = false, feAtomic = false, feValid = false;
    unsigned feTk = 0;
    int feTg = 0, feSp0 = 0;

    auto last_group = [](const Item &it) __attribute__((always_inline)) { return 4 * (it.g + 1) >= it.nCols; };

    // opens tick `tick`: the barrier, the items of this tick, the request, the staging of item V + 2.  false: the launch is over.
    // `waitImm`: the s_waitcnt in front of the barrier (header: vmcnt)
    auto open_tick = [&](bool storeYoungest) __attribute__((always_inline)) -> bool {
        if (storeYoungest)
            __builtin_amdgcn_s_waitcnt(wait_vmcnt_lgkm0(1));
        else
            __builtin_amdgcn_s_waitcnt(wait_vmcnt_lgkm0(0));
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        im1 = i0;
        i0 = i1;
        i1 = i2;
        if (i2.g >= 0 && !last_group(i2)) {
            ++i2.g;
        } else if (pending) {
            const unsigned slot = (requests - 1u) & 1u;
            const int tg = __builtin_amdgcn_readfirstlane(record[4 * slot + 0]);
            const int sp0 = __builtin_amdgcn_readfirstlane(record[4 * slot + 1]);
            const int nc = __builtin_amdgcn_readfirstlane(record[4 * slot + 2]);
            if (tg >= 0) {
                i2 = Item{tg, sp0, nc, 0};
            } else {
                i2.g = -1;
                ++hop;                     // the range is spent
            }
        } else {
            i2.g = -1;
        }
        pending = false;
        if (hop >= 8u && im1.g < 0 && i0.g < 0 && i1.g < 0 && i2.g < 0)
            return false;
        request = hop < 8u && (i2.g < 0 || last_group(i2));
        if (request) {
            pending = true;
            ++requests;
        }
        feOn = request && wave == 0;
        if (feOn) {
            // front end, step 1: a new chunk from the range's counter when the grabbed one is used up
            feXcd = (blockIdx.x + hop) & 7u;
            feRange = feXcd < nGroups ? ((nGroups - feXcd + 7u) >> 3) * (unsigned)nSrcBlocks : 0u;
            feAtomic = feGi >= feEnd;
            if (feAtomic && lane == 0)
                feTk = atomicAdd(&taskCtr[feXcd * kTaskCtrStride], (unsigned)taskChunk);
        }
        if (i2.g >= 0) {
            // this wave's column of item V + 2: column 4 g + wave of its target group (clamped to a real column) -> slot 4 ((V + 2) & 3) + wave
            const int cc = max(min(4 * i2.g + wave, i2.nCols - 1), 0);
            char *slot = ring + ((4 * (tick + 2u) + (unsigned)wave) & (unsigned)(kFilterWg2Ring - 1)) * kFilterSlotBytes;
            const char *gb = reinterpret_cast<const char *>(tgtRec) +
                             ((size_t)(unsigned)i2.tg * (unsigned)tgtFramesPad + (unsigned)cc) * (kTgtFrameHalfs * 2);   // wave-uniform, kept scalar
            SSYM_FILTER_SBASE(gb);
            SSYM_FILTER_LANEOFF(laneOff16);
            const __attribute__((address_space(1))) void *gp =
                (const __attribute__((address_space(1))) void *)(gb + laneOff16);
            __attribute__((address_space(3))) void *lp = (__attribute__((address_space(3))) void *)slot;
            __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
            __builtin_amdgcn_global_load_lds(gp, lp, 16, 1024, 0);
            if (KU == 3)
                __builtin_amdgcn_global_load_lds(gp, lp, 16, 2048, 0);
        }
        asm volatile("" ::: "memory");
        return true;
    };
    // front end, step 2 (behind the tick's second column): the task that is next, its target lengths requested
    auto front_end_task = [&]() __attribute__((always_inline)) {
        if (feOn) {
            if (feAtomic) {
                feGi = (unsigned)__builtin_amdgcn_readfirstlane((int)feTk);
                feEnd = min(feGi + (unsigned)taskChunk, feRange);
                feHalf = 0;
            }
            feValid = feGi < feEnd;
            if (feValid) {
                const unsigned lin = feRange - 1u - feGi;             // position in the XCD's range, walked from its end
                feTg = (int)(feXcd + 8u * (lin / (unsigned)nSrcBlocks));
                feSp0 = spBase + 4 * (int)(lin % (unsigned)nSrcBlocks) + 2 * (int)feHalf;
                // (an LDS-DMA, like the staging: a load into a register would hold it, and a wait, across two columns)
                const int *gl = tgtLen + 32 * feTg;
                SSYM_FILTER_SBASE(gl);
                SSYM_FILTER_LANEOFF(laneOff4);
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(reinterpret_cast<const char *>(gl) + (laneOff4 & 127u)),
                    (__attribute__((address_space(3))) void *)lenBuf, 4, 0, 0);
            }
        }
    };
    // front end, step 3 (behind the tick's fourth column): the record
    auto front_end_record = [&]() __attribute__((always_inline)) {
        if (feOn) {
            int nc = 0;
            if (feValid) {
                // the lengths requested two columns ago have landed (and with them everything older of this wave)
                __builtin_amdgcn_s_waitcnt(wait_vmcnt(0));
                asm volatile("" ::: "memory");
                nc = *reinterpret_cast<volatile int *>(lenBuf + laneOff4);
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1)
                    nc = max(nc, __shfl_xor(nc, o));
                nc = __builtin_amdgcn_readfirstlane(nc);
            }
            const unsigned slot = (requests - 1u) & 1u;
            if (lane == 0) {
                record[4 * slot + 0] = feValid ? feTg : -1;
                record[4 * slot + 1] = feSp0;
                record[4 * slot + 2] = nc;
            }
            if (feValid) {
                feHalf ^= 1u;
                if (feHalf == 0)
                    ++feGi;
            } else {
                feGi = feEnd = feHalf = 0;  // the next range starts with a grab
            }
        }
    };
    // B operands of the column in slot `s` of the ring
    auto fetch = [&](unsigned s, half8 (&B)[KU]) __attribute__((always_inline)) {
        const char *slot = ring + (s & (unsigned)(kFilterWg2Ring - 1)) * kFilterSlotBytes;
#pragma unroll
        for (int m = 0; m < KU; ++m)
            B[m] = *reinterpret_cast<const half8 *>(slot + m * 1024 + lane * 16);
    };

    // the column state of the wave's pass: lives from group 0 of a task to its last group
    half8 A[NT][KU];
    float L0[BR], L1[BR];
    half8 B0[KU], B1[KU];
    f32x16 acc;
    float prevTop = INF;
    // a task starts (group 0): A operands of the pass (the pad rows above a source carry |a|^2 = +inf), both column arrays,
    // column 0 from the ring (ring group vg) and its first MFMA chain.  Returns the lane's source length.
    auto start_task = [&](const Item &it, int rowBase, unsigned vg) __attribute__((always_inline)) {
        const int sp = it.sp0 + (wave >> 1);
        const int fa = srcLen[2 * sp + half];
        {
            const int arow = lane & 31;
            const int a_src = 2 * sp + ((arow >> 2) & 1);
            const int a_frm = rowBase + (arow & 3) + 4 * (arow >> 3);
            const _Float16 *abase = srcRec + ((size_t)a_src * srcRows + a_frm) * REC + half * 24;
#pragma unroll
            for (int T = 0; T < NT; ++T)
                load_rec<KU>(abase + (size_t)T * kFilterRowsPerTile * REC, A[T]);
        }
        const int r0 = srcRows - fa;   // first real row: sources are END-ALIGNED in their row slots
        // D(., -1): +inf, except the virtual D(r0-1, -1) = 0 that starts the recurrence
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            L0[i] = (rowBase + i == r0 - 1) ? 0.0f : INF;
            L1[i] = L0[i];
        }
        prevTop = (rowBase == r0) ? 0.0f : INF;
        fetch(4u * vg, B0);
        acc = mfma_tile<KU>(A[0], B0);
    };

    if (!follower) {
        // ================= leader: pass 0, item V at tick V, bottoms into hand-off buffer V & 1 =================
        float up = INF;
        asm volatile("" : "+v"(up));       // (kept a register: the cells' v_min3 reads it like any top value)
        for (;; ++tick) {
            if (!open_tick(false))
                break;
            if (i0.g >= 0) {
                const unsigned vg = tick & 3u;
                if (i0.g == 0)
                    start_task(i0, rowOrigin, vg);
                char *const handW = hand + (tick & 1u) * 1024 + lane * 4;
                auto column = [&](int q) __attribute__((always_inline)) {
                    const float diag = prevTop;
                    prevTop = up;
                    float bottom;
                    if ((q & 1) == 0) {
                        fetch(4u * vg + q + 1, B1);
                        bottom = dp_column<NT, SQ, KU>(A, B0, B1, acc, up, diag, L0, L1);
                    } else {
                        fetch(4u * vg + q + 1, B0);
                        bottom = dp_column<NT, SQ, KU>(A, B1, B0, acc, up, diag, L1, L0);
                    }
                    *reinterpret_cast<float *>(handW + q * 256) = bottom;          // top boundary of the follower's pass
                };
                column(0);
                column(1);
                front_end_task();
                column(2);
                column(3);
                front_end_record();
            } else {
                front_end_task();
                front_end_record();
            }
        }
    } else {
        // ================= follower: pass 1, item V - 1 at tick V, tops from hand-off buffer (V - 1) & 1 =================
        float res = INF;
        int fb_m1 = -1;
        bool stored = false;               // the wave's youngest vector-memory operation is a cost store
        for (;; ++tick) {
            if (!open_tick(stored))
                break;
            stored = false;
            if (im1.g >= 0) {
                const unsigned vg = (tick + 3u) & 3u;
                const char *const handR = hand + ((tick + 1u) & 1u) * 1024 + lane * 4;
                float topN = *reinterpret_cast<const float *>(handR);           // the group's first column: written in the tick before
                if (im1.g == 0) {
                    fb_m1 = tgtLen[32 * im1.tg + col] - 1;
                    res = INF;
                    start_task(im1, rowOrigin + BR, vg);
                }
                const int j0 = 4 * im1.g;
                auto column = [&](int q) __attribute__((always_inline)) {
                    const float up = topN;
                    const float diag = prevTop;
                    prevTop = up;
                    if (q < 3)
                        topN = *reinterpret_cast<const float *>(handR + (q + 1) * 256);
                    float bottom;
                    if ((q & 1) == 0) {
                        fetch(4u * vg + q + 1, B1);
                        bottom = dp_column<NT, SQ, KU>(A, B0, B1, acc, up, diag, L0, L1);
                    } else {
                        fetch(4u * vg + q + 1, B0);
                        bottom = dp_column<NT, SQ, KU>(A, B1, B0, acc, up, diag, L1, L0);
                    }
                    res = (j0 + q == fb_m1) ? bottom : res;         // D(fa-1, fb-1)
                };
                column(0);
                column(1);
                column(2);
                column(3);
                if (last_group(im1)) {
                    const int sp = im1.sp0 + (wave >> 1);
                    cmat[(size_t)(2 * sp + half) * mPad + 32 * im1.tg + col] = res * outScale;
                    stored = true;
                }
            }
        }
    }
   }
}

#undef SSYM_FILTER_SBASE
#undef SSYM_FILTER_LANEOFF

}  // namespace ssym
