// dtw_cover_chain.hpp -- one step of the cover's chain (DESIGN.md 2 "Cover", "Cover with gaps"): best(e) and its back-pointer
// from the folded M / src tables, the ring of earlier best values and the price of leaving frame e uncovered.  cover_chain_kernel (dtw_cover.hip) runs it over a whole target,
// coverer_chain_kernel (dtw_coverer.hip) over the frames a push brought: one body, so the two cannot drift apart.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ssym {

constexpr uint32_t kCoverNone = 0xffffffffu;
constexpr uint32_t kCoverGap = 0xfffffffeu;              // SSYM_COVER_GAP: the "source" of a frame left uncovered

struct CoverPick {
    double v, m;                 // best(e) and the cost M of its last piece
    uint32_t len, src;           // ... its length and source; kCoverNone without one
};

// One wave (64 lanes, all of them here).  tabM / tabSrc: [width][frames]; col: the table column of end e (row L - 1 holds the
// window that STARTS at the column, so the window of L frames that ends at e is read at col + 1 - L); lMax: the longest
// window that ends at e; ring: best(x) at (x + 1) & ringMask, e counted as the ring counts it.  The <= 2 Fmax candidates
// are spread over the lanes (L ascending within a lane, strict <) and reduced by (v, L); every lane returns the result.
// gapCost: the price of leaving frame e uncovered, >= 0 or +inf.  The gap candidate gapCost + best(e-1) is read in LDS alone
// (best(e-1) is in the ring already) and wins under strict < only, so a piece keeps a tie and +inf never wins: with
// gapCost = +inf the step is the plain cover's.  A gap is the pick (len 1, kCoverGap, gapCost); no penalty is charged on it.
__device__ __forceinline__ CoverPick cover_chain_step(const double *tabM, const uint32_t *tabSrc, uint64_t frames, uint64_t col,
                                                      uint32_t lMax, double penalty, double gapCost, const double *ring,
                                                      uint32_t ringMask, uint64_t e, uint32_t lane)
{
    const double INF = __builtin_inf();
    const double gapV = __dadd_rn(gapCost, ring[e & ringMask]);          // gap_cost + best(e-1)
    double bestV = INF, bestM = INF;
    uint32_t bestL = kCoverNone, bestS = kCoverNone;
    for (uint32_t L = lane + 1; L <= lMax; L += 64) {
        const size_t o = (size_t)(L - 1) * frames + col + 1 - L;
        const uint32_t src = tabSrc[o];
        if (src == kCoverNone)
            continue;
        const double m = tabM[o];
        const double v = __dadd_rn(__dadd_rn(m, penalty), ring[(e + 1 - L) & ringMask]);
        if (v < bestV) {                         // L ascends within a lane: the shorter piece stays
            bestV = v;
            bestM = m;
            bestL = L;
            bestS = src;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oV = __shfl_xor(bestV, m), oM = __shfl_xor(bestM, m);
        const uint32_t oL = (uint32_t)__shfl_xor((int)bestL, m), oS = (uint32_t)__shfl_xor((int)bestS, m);
        if (oV < bestV || (oV == bestV && oL < bestL)) {
            bestV = oV;
            bestM = oM;
            bestL = oL;
            bestS = oS;
        }
    }
    if (gapV < bestV)
        return CoverPick{gapV, gapCost, 1u, kCoverGap};
    return CoverPick{bestV, bestM, bestL, bestS};
}

}  // namespace ssym
