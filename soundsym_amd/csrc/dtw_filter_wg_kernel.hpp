// dtw_filter_wg_kernel.hpp -- sibling of dtw_filter_kernel<4, SQ, 2, false, KU, false> (dtw_filter_kernel.hpp) for launches
// whose pairs all run the same passes: the four waves of a workgroup take the SAME target group and four consecutive
// source pairs, and share ONE ring of target columns in LDS.  (Included by dtw_filter.hip behind dtw_filter_kernel.hpp.)
//
// Why: in dtw_filter_kernel every wave stages its target group's column for itself -- KU KB by KU global_load_lds DMAs
// per wave and column, 137 GB of L2 -> LDS traffic per headline launch, almost all of it the same bytes four times.  Here a
// column is staged once per workgroup: a quarter of the DMAs, of their scalar address arithmetic and of the L2 requests.
// The cells, the MFMAs, the record layouts, the per-wave hand-off row (buffer-addressed, column-major) and the per-wave
// top buffers are those of dtw_filter_kernel; per cell the same operations in the same order, so the filter matrix keeps
// its bits.
// Measured on the headline (LAB.md 5.1): 32.90 -> 32.24 ms (-2.0 %).  The instruction stream is unchanged (3.19 VALU
// instructions per wave-cell) and the barriers cost cycles (17.18 -> 17.51 elapsed per wave-cell), but with a third of the
// vector-memory instructions and 44 % of the L2 requests the power-limited chip clocks 2.16 -> 2.29 GHz.
//
//   * Tasks.  A workgroup task is (block of 4 source pairs, target group); wave w takes pair spBase + 4 block + w.  Tasks
//     come from the same eight per-XCD counters and ranges as dtw_filter_kernel's, counted in blocks (nSrcBlocks =
//     nSrcPairs / 4: the host launches this kernel only on a multiple of four pairs).  Lane 0 of wave 0 takes the chunk; the
//     value reaches the other waves through an LDS word and a barrier.  (The word lies in wave 0's top buffer, which nothing
//     else uses between tasks; two words alternate so that wave 0 may write the next one while a wave still reads this one.)
//   * Ring.  16 column slots per workgroup, stride kFilterSlotBytes: virtual column c lives in slot c & 15, column GROUP
//     g = c >> 2 in the four slots 4 (g & 3) ...  Slot 4 k + w is only ever written by wave w (whose DMAs land in order).
//   * Staging and waits.  At the top of group g wave w stages column 4 (g + 2) + w (clamped to the last real column) with KU
//     DMAs, waits with s_waitcnt vmcnt until ITS share of group g + 1 has landed, and executes one s_barrier.  After that
//     barrier group g + 1 is complete for every wave (the last column of group g fetches its first column), and every
//     wave has finished group g - 1: a wave that stages group g + 3 at the top of group g + 1 overwrites the slots of group
//     g - 1, and got there through this barrier.  The prologue of a pass stages groups 0 and 1, waits for its share of
//     group 0, and has a barrier of its own before column 0 is fetched.
//   * vmcnt immediates, per pass kind.  A wave's vector-memory operations in program order are, per group g: S(g + 2) (KU
//     DMAs, top of the group), T(g + 1) (the hand-off DMA of the next group's top values, after column 4 g's fetch, in every
//     pass but a task's first) and one hand-off store behind each column (in every pass but the last).  Loads, DMAs and
//     stores of one wave retire in order as far as vmcnt counts them.
//       - top of group g >= 1, for S(g + 1): younger are T(g) [0 or 1], the stores of group g - 1 [0 or 4] and S(g + 2)
//         [KU]: KU + 5 in a middle pass, KU + 4 in a first pass of several, KU + 1 in a last pass of several, KU in a single
//         pass.  The kernel uses vmcnt(KU + 4) in every pass but the last and vmcnt(KU) in the last: never more lenient
//         than the count, and what it waits for beyond S(g + 1) is T(g), issued four columns earlier;
//       - top of group 0: nothing lies between S(1) and S(2): vmcnt(KU) whatever the pass;
//       - prologue, for S(0) (and everything older: the A operands, T(0), whatever an earlier pass left in flight): S(1)
//         is younger: vmcnt(KU);
//       - before column 4 g + 3 fetches the first top value of group g + 1, for T(g + 1): younger are the stores of columns
//         4 g ... 4 g + 2: vmcnt(3) in a middle pass, vmcnt(0) in a last pass (S(g + 2) is older than T(g + 1): no stall
//         beyond T(g + 1)'s own, three columns after its issue); a first pass has no T and no wait.
//     More operations in flight than counted (the cost store and the length loads of the task before) only make a wait
//     stricter.
//   * Barriers: one per four columns, one in the prologue (group 0 has landed), one at each pass start -- before the
//     prologue's staging overwrites slots a slower wave may still read -- and one per task fetch.
//     INVARIANT: every wave of a workgroup executes the same sequence of barriers.  The task (block, target group) is the
//     workgroup's, so nCols -- the longest target of the shared group -- is the same in all four waves; nPasses is the
//     launch's; every pair starts at pass 0 (the host launches this kernel only where pass 0 holds a row of the shortest
//     pair of the range, dtw_filter_plan.hpp plan_filter, so firstPass is not computed here); hop, got, rangeLen and the chunk's
//     bounds are the workgroup's.  No condition that differs between the waves of a workgroup encloses a barrier: the only
//     wave-dependent branch (wave 0 takes the chunk) holds none.
//   * LDS: 16 slots x 3 KB + 4 waves x 2 KB of top buffers = 56 KB per workgroup, as much as dtw_filter_kernel's four rings of four slots.
#pragma once
#include "dtw_filter_kernel.hpp"

namespace ssym {

#define SSYM_FILTER_SBASE(P_) asm volatile("" : "+s"(P_))
#define SSYM_FILTER_LANEOFF(V_) asm volatile("" : "+v"(V_))

constexpr int kFilterWgRing = 16;                      // column slots per workgroup: four groups of four columns
constexpr int kFilterWgLds = kFilterWgRing * kFilterSlotBytes + kFilterWavesPerBlock * kFilterTopBytes;

template <bool SQ, int KU>
__global__ __launch_bounds__(64 * kFilterWavesPerBlock, 2) void dtw_filter_wg_kernel(
    const _Float16 *__restrict__ srcRec, const _Float16 *__restrict__ tgtRec,
    const int *__restrict__ srcLen, const int *__restrict__ tgtLen, int srcRows, int nPasses,
    int tgtFramesPad, int mPad, int nSrcBlocks, int taskChunk, float outScale,
    float *__restrict__ handoff, unsigned *__restrict__ taskCtr, float *__restrict__ cmat,
    int rowOrigin, int spBase)
{
    static_assert(KU == 2 || KU == 3, "two or three operand planes per column");
    static_assert(kFilterWavesPerBlock == 4, "a column group is one column per wave");
    constexpr int NT = 4;
    constexpr int REC = kFilterRecHalfs;
    constexpr int BR = NT * 16;            // rows per pass
    const float INF = __builtin_inff();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31;
    const int half = lane >> 5;
    // this wave's hand-off row, as in dtw_filter_kernel
    const size_t handGroups = ((size_t)tgtFramesPad + 3) / 4;
    char *const handRow = reinterpret_cast<char *>(handoff + ((size_t)blockIdx.x * kFilterWavesPerBlock + wave) * handGroups * 256);
    uint32_t laneOff16 = lane * 16;
    const __amdgpu_buffer_rsrc_t handBuf = __builtin_amdgcn_make_buffer_rsrc(handRow, 0, (int)(handGroups * 1024), 0x00020000);
    constexpr int kWaitStaged = wait_vmcnt(KU), kWaitStagedStores = wait_vmcnt(KU + 4);
    __shared__ __attribute__((aligned(16))) char lds[kFilterWgLds];
    char *const ring = lds;
    char *const myTop = lds + kFilterWgRing * kFilterSlotBytes + wave * kFilterTopBytes;
    volatile unsigned *const taskWord = reinterpret_cast<volatile unsigned *>(lds + kFilterWgRing * kFilterSlotBytes);
    unsigned fetches = 0;                  // task fetches so far: the same in every wave of the workgroup

    const unsigned nGroups = (unsigned)mPad >> 5;
    for (unsigned hop = 0; hop < 8; ++hop) {
      const unsigned xcd = (blockIdx.x + hop) & 7u;
      const unsigned rangeLen = xcd < nGroups ? ((nGroups - xcd + 7u) >> 3) * (unsigned)nSrcBlocks : 0u;
      for (;;) {
        // one lane of wave 0 takes the chunk for the workgroup
        if (wave == 0) {
            // (a hand-off DMA this wave left in flight targets the buffer the word lies in)
            __builtin_amdgcn_s_waitcnt(wait_vmcnt(0));
            asm volatile("" ::: "memory");
            if (lane == 0)
                taskWord[fetches & 1u] = atomicAdd(&taskCtr[xcd * kTaskCtrStride], (unsigned)taskChunk);
        }
        __syncthreads();
        const unsigned got = (unsigned)__builtin_amdgcn_readfirstlane((int)taskWord[fetches & 1u]);
        ++fetches;
        if (got >= rangeLen)
            break;
        const unsigned gotEnd = min(got + (unsigned)taskChunk, rangeLen);
        int preFa = 0, preFb = 0;
        bool havePre = false;                   // workgroup-uniform
       for (unsigned gi = got; gi < gotEnd; ++gi) {
        const unsigned lin = rangeLen - 1u - gi;                      // position in the XCD's range, walked from its end
        const int tg = (int)(xcd + 8u * (lin / (unsigned)nSrcBlocks));
        const int sp = spBase + 4 * (int)(lin % (unsigned)nSrcBlocks) + wave;    // source pair of this wave

        const int fa = havePre ? preFa : srcLen[2 * sp + half];
        const int fb_m1 = (havePre ? preFb : tgtLen[32 * tg + col]) - 1;
        havePre = gi + 1 < gotEnd;
        if (havePre) {
            const unsigned linN = lin - 1u;
            preFa = srcLen[2 * (spBase + 4 * (int)(linN % (unsigned)nSrcBlocks) + wave) + half];
            preFb = tgtLen[32 * (int)(xcd + 8u * (linN / (unsigned)nSrcBlocks)) + col];
        }
        const int r0 = srcRows - fa;   // first real row: sources are END-ALIGNED in their row slots

        // columns up to the longest target of the group: the same in every wave of the workgroup
        int nCols = fb_m1 + 1;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1)
            nCols = max(nCols, __shfl_xor(nCols, o));
        nCols = __builtin_amdgcn_readfirstlane(nCols);

        float res = INF;
        const char *const tgtGroup = reinterpret_cast<const char *>(tgtRec) + (size_t)tg * tgtFramesPad * (kTgtFrameHalfs * 2);

        for (int pass = nCols > 0 ? 0 : nPasses; pass < nPasses; ++pass) {
            const int rowBase = rowOrigin + pass * BR;
            // the pass kind, workgroup-uniform.  (Opaque scalar integers: as booleans the two live through the column loop as
            // lane masks that the compiler negates through a VGPR, two vector instructions per four columns each.)
#ifdef SSYM_ABL_NOHAND      // tools only (as in dtw_filter_kernel): no hand-off DMA and no hand-off store -- wrong values, valid timing
            int haveTop = 0, passesLeft = nPasses - 1 - pass;
#else
            int haveTop = pass, passesLeft = nPasses - 1 - pass;      // a row above this pass; 0 in the last pass
#endif
            asm volatile("" : "+s"(haveTop), "+s"(passesLeft));     // (and again before each test in the column loop: a hoisted compare is a mask again)

            // this wave's column of group gr: virtual column 4 gr + wave (clamped to the last real column) -> slot (4 gr + wave) & 15
            auto stage = [&](int gr) {
                const int c = 4 * gr + wave;
                const int cc = min(c, nCols - 1);
                char *slot = ring + (c & (kFilterWgRing - 1)) * kFilterSlotBytes;
                const char *gb = tgtGroup + (size_t)(unsigned)cc * (kTgtFrameHalfs * 2);       // wave-uniform, kept scalar
                SSYM_FILTER_SBASE(gb);
                SSYM_FILTER_LANEOFF(laneOff16);
                const __attribute__((address_space(1))) void *gp =
                    (const __attribute__((address_space(1))) void *)(gb + laneOff16);
                __attribute__((address_space(3))) void *lp = (__attribute__((address_space(3))) void *)slot;
                __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
                __builtin_amdgcn_global_load_lds(gp, lp, 16, 1024, 0);
                if (KU == 3)
                    __builtin_amdgcn_global_load_lds(gp, lp, 16, 2048, 0);
            };
            // hand-off values of column group g (4 columns x 64 lanes, as stored) -> top buffer g & 1
            auto stageTop = [&](int g) {
                const int gg = min(g, (nCols - 1) >> 2);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(handBuf, (__attribute__((address_space(3))) void *)(myTop + (g & 1) * 1024),
                                                         16, laneOff16, gg * 1024, 0, 0);
            };
            auto fetch = [&](int c, half8 (&B)[KU], float &top) {
                const char *slot = ring + (c & (kFilterWgRing - 1)) * kFilterSlotBytes;
#pragma unroll
                for (int m = 0; m < KU; ++m)
                    B[m] = *reinterpret_cast<const half8 *>(slot + m * 1024 + lane * 16);
                top = *reinterpret_cast<const float *>(myTop + ((c >> 2) & 1) * 1024 + (c & 3) * 256 + lane * 4);
            };
            // A operands of this pass: the pad rows above a source carry |a|^2 = +inf
            half8 A[NT][KU];
            {
                const int arow = lane & 31;
                const int a_src = 2 * sp + ((arow >> 2) & 1);
                const int a_frm = rowBase + (arow & 3) + 4 * (arow >> 3);
                const _Float16 *abase = srcRec + ((size_t)a_src * srcRows + a_frm) * REC + half * 24;
#pragma unroll
                for (int T = 0; T < NT; ++T)
                    load_rec<KU>(abase + (size_t)T * kFilterRowsPerTile * REC, A[T]);
            }

            // pass start: every wave has left the pass (or the task) before -- the staging below overwrites slots a slower
            // wave would still read
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");      // A loads are issued (program order) before the staging DMAs
            if (haveTop)
                stageTop(0);
            stage(0);
            stage(1);

            // D(., -1): +inf, except the virtual D(r0-1, -1) = 0 that starts the recurrence
            float L0[BR], L1[BR];
#pragma unroll
            for (int i = 0; i < BR; ++i) {
                L0[i] = (rowBase + i == r0 - 1) ? 0.0f : INF;
                L1[i] = L0[i];
            }
            float prevTop = (rowBase == r0) ? 0.0f : INF;

            half8 B0[KU], B1[KU];
            float topN = INF;
            // this wave's column of group 0 has landed, and everything older (header: prologue)
            __builtin_amdgcn_s_waitcnt(kWaitStaged);
            asm volatile("" ::: "memory");
            // a pass without a row above it reads +inf as its top values (both buffers are this wave's own; the wait above
            // has landed every hand-off DMA an earlier pass left in flight, and the other waves have read the task word)
            if (!haveTop) {
                typedef float f32x4 __attribute__((ext_vector_type(4)));
                *reinterpret_cast<f32x4 *>(myTop + lane * 16) = f32x4{INF, INF, INF, INF};
                *reinterpret_cast<f32x4 *>(myTop + 1024 + lane * 16) = f32x4{INF, INF, INF, INF};
            }
            __builtin_amdgcn_s_barrier();       // group 0 is complete
            asm volatile("" ::: "memory");
            fetch(0, B0, topN);
            f32x16 acc = mfma_tile<KU>(A[0], B0);

            for (int j0 = 0; j0 < nCols; j0 += 4) {
                const int g = j0 >> 2;
                stage(g + 2);                   // into the slots group g - 2 left
                // this wave's column of group g + 1 has landed (header: the immediates per pass kind)
                SSYM_FILTER_SBASE(passesLeft);
                if (passesLeft == 0 || j0 == 0)
                    __builtin_amdgcn_s_waitcnt(kWaitStaged);
                else
                    __builtin_amdgcn_s_waitcnt(kWaitStagedStores);
                asm volatile("" ::: "memory");
                __builtin_amdgcn_s_barrier();   // group g + 1 is complete; every wave has finished group g - 1
                asm volatile("" ::: "memory");
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + q;
                    if (j < nCols) {                                // workgroup-uniform
                        const float up = topN;
                        const float diag = prevTop;
                        prevTop = up;
                        SSYM_FILTER_SBASE(haveTop);
                        SSYM_FILTER_SBASE(passesLeft);
                        if (q == 3 && haveTop) {
                            // the next group's top values, requested at this group's first column, have landed
                            if (passesLeft == 0)
                                __builtin_amdgcn_s_waitcnt(wait_vmcnt(0));
                            else
                                __builtin_amdgcn_s_waitcnt(wait_vmcnt(3));
                            asm volatile("" ::: "memory");
                        }
                        if ((q & 1) == 0)
                            fetch(j + 1, B1, topN);
                        else
                            fetch(j + 1, B0, topN);
                        if (q == 0 && haveTop)
                            stageTop(g + 1);                        // the next group's top values
                        float bottom;
                        if ((q & 1) == 0)
                            bottom = dp_column<NT, SQ, KU>(A, B0, B1, acc, up, diag, L0, L1);
                        else
                            bottom = dp_column<NT, SQ, KU>(A, B1, B0, acc, up, diag, L1, L0);
                        SSYM_FILTER_SBASE(passesLeft);
                        if (passesLeft != 0) {
                            // top boundary of the next pass: a column's bottoms are 256 contiguous bytes
#ifndef SSYM_ABL_NOHAND
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(bottom), handBuf, lane * 4, g * 1024 + q * 256, 0);
#else
                            res = (j == fb_m1 - 1) ? bottom : res;
#endif
                        } else {
                            res = (j == fb_m1) ? bottom : res;      // D(fa-1, fb-1)
                        }
                    }
                }
            }
        }
        cmat[(size_t)(2 * sp + half) * mPad + 32 * tg + col] = res * outScale;
       }
      }
    }
}

#undef SSYM_FILTER_SBASE
#undef SSYM_FILTER_LANEOFF

}  // namespace ssym
