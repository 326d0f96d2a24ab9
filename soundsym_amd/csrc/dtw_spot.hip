// dtw_spot.hip -- DTW spotting (subsequence DTW): where inside an unsegmented source a target aligns best, for a list of
// (source, target) pairs, and the best source per target (DESIGN.md 2 "Spotting", 5.15).
//
// Role on the path: every search compares a target with whole dictionary segments; this one leaves the source open at
// both ends, so a dictionary of uncut recordings can be asked where a target sounds.  Per pair: the inclusive span
// [start, end] of source frames and its cost, which is the plain DTW cost of (source[start ... end], target).
//
// Definition (i = source frame, j = target frame, c = the local cost of the context):
//   D(i,0) = c(i,0), st(i,0) = i;   D(i,j) = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)), outside the matrix +inf;
//   st(i,j) = st of the predecessor the alignment rule picks: dg = D(i-1,j-1), up = D(i-1,j), lf = D(i,j-1):
//             diagonal if dg <= up && dg <= lf, else up if up <= lf, else left;
//   end = the smallest i at which D(i,Fb-1) is least (strict <, from +inf: NaN and +inf never win), cost = D(end,Fb-1),
//   start = st(end,Fb-1).
//
// Arithmetic and mapping: dtw_wave.hpp's wavefront, one wave per pair, grid-stride over the list, with a free start in
// column 0.  Everything carried between lanes and through the hand-off row is a pair (D f64, st u32); the row has Fb
// entries, so the LDS a pair needs does not grow with the source.  Every lane keeps the best D(r, Fb-1) of its own rows
// (chunks ascend, strict <: its lowest such row); one wave reduction per pair orders the 64 candidates by (D, row).  No
// direction matrix, no backward walk: three scalars per pair, written by lane 0.
//
// Occurrences (ssym_dtw_spot_all; DESIGN.md 2 "Occurrences", 5.16): the same forward pass with the end column kept.  A
// lane's last value of a chunk IS (D(r, Fb-1), st(r, Fb-1)), so the profile costs no register: one 8-byte and one 4-byte
// store per lane per chunk into the workgroup's scratch slot.  The wave then picks up to K disjoint spans from its slot:
// pick 0 is the end reduction above; every further pick is one pass that kills what the previous pick overlaps (+inf into
// the profile) and finds the first least survivor.  Lane l only ever touches entries i = l (mod 64), the ones it wrote
// itself, so the passes need no exchange through memory, only the (D, row) butterfly.
#include "dtw_wave.hpp"

#include <algorithm>
#include <type_traits>

namespace ssym {

// Limits of ssym_dtw_spot / ssym_spot_queries (soundsym_amd.h): frames of a target, values per frame.
// A source has as many frames as a dictionary segment can (2^31 - 1).
constexpr int kSpotMaxTargetFrames = 4096;
constexpr int kSpotMaxDim = 64;
// Limit of the paced step pattern (the _step entry points with SSYM_STEP_PACED): two hand-off rows take 24 bytes per target
// frame, and with the ring (66 KiB at DIMR = 64) 4096 frames would need 162 KiB of the 160 KiB of LDS
constexpr int kPacedMaxTargetFrames = 2048;
// Limits of ssym_dtw_spot_all: occurrences per pair, and frames of a listed source -- the profile lives in global scratch
// at 12 bytes per source frame, 192 MiB for one pair at this length.  The scratch of a call stays within
// kSpotAllScratchBytes: one slot per workgroup, fewer workgroups for longer sources.
constexpr uint32_t kSpotAllMaxSpots = 64;
constexpr uint64_t kSpotAllMaxSourceFrames = 16777216;          // 2^24
constexpr size_t kSpotAllScratchBytes = (size_t)512 << 20;

namespace {

struct SpotArgs {
    const double *srcRaw;
    const uint64_t *srcOff;
    const double *tgtRaw;
    const uint64_t *tgtOff;
    uint32_t dim;
    int squared;
    const uint2 *pairs;          // (source, target); source 0xffffffff = no match; NULL: pair k = (k / nTgt, k % nTgt)
    uint32_t nTgt;
    uint32_t nPairs;
    double *cost;                // [nPairs]
    uint32_t *start, *end;       // [nPairs]
    uint32_t fbCap;              // even, >= the longest listed target
    uint32_t ringRows;           // 64 or 128
};

// ssym_dtw_spot_all: cost / start / end are [nPairs][maxSpots].  A struct of its own: the spot kernels' arguments, and
// with them their register figures, stay what they were.
struct SpotAllArgs : SpotArgs {
    uint32_t maxSpots;           // K
    uint32_t *count;             // [nPairs]
    const double *maxCost;       // [nPairs], NULL: none
    double *profD;               // [gridDim.x][slotFrames]  the end column of the workgroup's current pair: D ...
    uint32_t *profS;             // [gridDim.x][slotFrames]  ... and st
    uint64_t slotFrames;         // >= the longest listed source
};

// pair k of ssym_dtw_spot_all has cnt occurrences: the count, and the slots behind them (maxSpots <= 64: one per lane)
__device__ __forceinline__ void spot_all_pad(const SpotAllArgs &a, uint32_t k, uint32_t cnt)
{
    const uint32_t m = threadIdx.x;
    if (m == 0)
        a.count[k] = cnt;
    if (m >= cnt && m < a.maxSpots) {
        const size_t o = (size_t)k * a.maxSpots + m;
        a.cost[o] = __builtin_inf();
        a.start[o] = 0xffffffffu;
        a.end[o] = 0xffffffffu;
    }
}

// the selection passes of the occurrences, after the end reduction has left the first least end of the
// profile in (bestD, bestEnd, bestSt): write the pick, kill every end whose span [st(i), i] shares a frame with it, find the
// first least survivor, until K picks are made or no candidate is left (the least survivor is a candidate or nothing is:
// bestEnd names a row, so bestD is finite), then the count and the padding.  One text for dtw_spot_kernel and
// dtw_paced_kernel, as a macro for the reason SSYM_SPOT_FIRST_MIN gives (INF: the kernel's own constant)
#define SSYM_SPOT_SELECT(a, k, Fa, lane, bestD, bestEnd, bestSt)                                                          \
    {                                                                                                                     \
        double *pD = a.profD + (size_t)blockIdx.x * a.slotFrames;                                                         \
        uint32_t *pS = a.profS + (size_t)blockIdx.x * a.slotFrames;                                                       \
        const double maxCost = a.maxCost ? a.maxCost[k] : INF;                                                            \
        const size_t o = (size_t)k * a.maxSpots;                                                                          \
        uint32_t cnt = 0;                                                                                                 \
        __threadfence_block();                                                                                            \
        while (bestEnd != 0xffffffffu && bestD <= maxCost) {                                                              \
            if (lane == 0) {                                                                                              \
                a.cost[o + cnt] = bestD;                                                                                  \
                a.start[o + cnt] = bestSt;                                                                                \
                a.end[o + cnt] = bestEnd;                                                                                 \
            }                                                                                                             \
            if (++cnt == a.maxSpots)                                                                                      \
                break;                                                                                                    \
            const uint32_t pickS = bestSt, pickE = bestEnd;                                                               \
            bestD = INF;                                                                                                  \
            bestEnd = bestSt = 0xffffffffu;                                                                               \
            _Pragma("unroll 4")                                                                                           \
            for (uint32_t i = (uint32_t)lane; i < Fa; i += 64) {                                                          \
                const double d = pD[i];                                                                                   \
                const uint32_t s = pS[i];                                                                                 \
                if (s <= pickE && i >= pickS) {                                                                           \
                    pD[i] = INF;                                                                                          \
                } else if (d < bestD) {                                                                                   \
                    bestD = d;                                                                                            \
                    bestEnd = i;                                                                                          \
                    bestSt = s;                                                                                           \
                }                                                                                                         \
            }                                                                                                             \
            SSYM_SPOT_FIRST_MIN(bestD, bestEnd, bestSt)                                                                   \
        }                                                                                                                 \
        spot_all_pad(a, k, cnt);                                                                                          \
    }

// ALL (ssym_dtw_spot_all, Args = SpotAllArgs): keep the end column and pick up to a.maxSpots disjoint spans from it
template <int DIMR, bool ALL = false, class Args = SpotArgs>
__global__ __launch_bounds__(64) void dtw_spot_kernel(const Args a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int LD = wave_ld(DIMR);
    double *boundD = smem;                                          // [fbCap]   bottom row of the chunk above: D ...
    double *ring = smem + a.fbCap;                                  // [ringRows][LD]
    uint32_t *boundS = reinterpret_cast<uint32_t *>(ring + (size_t)a.ringRows * LD);      // [fbCap]   ... and st
    const double INF = __builtin_inf();
    const int lane = threadIdx.x;
    const int dim = (int)a.dim;
    const uint32_t ringMask = a.ringRows - 1;

    for (uint32_t k = blockIdx.x; k < a.nPairs; k += gridDim.x) {
        uint2 p;
        if (a.pairs)
            p = a.pairs[k];
        else
            p = make_uint2(k / a.nTgt, k % a.nTgt);
        uint32_t Fa = 0;             // (a dictionary segment has at most 2^31 - 1 frames: row numbers fit 32 bits)
        int Fb = 0;
        if (p.x != 0xffffffffu) {
            Fa = (uint32_t)(a.srcOff[p.x + 1] - a.srcOff[p.x]);
            Fb = (int)(a.tgtOff[p.y + 1] - a.tgtOff[p.y]);
        }
        if (Fa == 0 || Fb == 0) {
            if constexpr (ALL) {
                spot_all_pad(a, k, 0u);
            } else if (lane == 0) {
                a.cost[k] = INF;
                a.start[k] = 0xffffffffu;
                a.end[k] = 0xffffffffu;
            }
            continue;
        }
        const double *a0 = a.srcRaw + a.srcOff[p.x] * dim;
        const double *b0 = a.tgtRaw + a.tgtOff[p.y] * dim;

        double bestD = INF;                 // this lane's rows: the least D(r, Fb-1) so far, its row and its start
        uint32_t bestEnd = 0xffffffffu, bestSt = 0xffffffffu;
        for (uint32_t c0 = 0; c0 < Fa; c0 += 64) {
            const uint32_t r = c0 + (uint32_t)lane;
            const bool rowValid = r < Fa;
            const int rowsHere = (int)min(64u, Fa - c0);
            double ar[DIMR];
            wave_load_frame(ar, a0 + (size_t)(rowValid ? r : c0) * dim, dim);
            double mineD = INF;             // D(r, j-1)
            uint32_t mineS = 0xffffffffu;
            double diagD = INF;             // D(r-1, j-1)
            uint32_t diagS = 0xffffffffu;
            const int tauEnd = Fb - 1 + rowsHere;     // exclusive: lane l works on column tau - l
            for (int tau = 0; tau < tauEnd; ++tau) {
                // (the refill's barrier also orders the hand-off row: the previous chunk's writes, and the previous pair's
                // reads, are done before tau = 0 goes on)
                if ((tau & 63) == 0)
                    wave_refill<DIMR>(ring, ringMask, b0, dim, Fb, tau);
                const int j = tau - lane;
                const double c = wave_cell_cost(ar, ring, ringMask, min(max(j, 0), Fb - 1), a.squared);
                double upD = shfl_up1(mineD);             // D(r-1, j) and its start, for lanes >= 1
                uint32_t upS = (uint32_t)shfl_up1((int)mineS);
                double dgD = diagD;
                uint32_t dgS = diagS;
                if (lane == 0) {
                    upD = dgD = INF;                      // above row 0 there is nothing
                    upS = dgS = 0xffffffffu;
                    if (c0 != 0) {
                        if (j >= 0 && j < Fb) {
                            upD = boundD[j];
                            upS = boundS[j];
                        }
                        if (j >= 1 && j <= Fb) {
                            dgD = boundD[j - 1];
                            dgS = boundS[j - 1];
                        }
                    }
                }
                const bool active = rowValid && j >= 0 && j < Fb;
                if (active) {
                    double cur = c;                       // column 0: a path may start at any source frame
                    uint32_t st = r;
                    if (j > 0) {
                        cur = __dadd_rn(c, wave_min3(upD, mineD, dgD));
                        const uint32_t pred = wave_pred(upD, mineD, dgD);
                        st = pred == 0u ? dgS : pred == 1u ? upS : mineS;
                    }
                    if (lane == 63) {
                        boundD[j] = cur;
                        boundS[j] = st;
                    }
                    if (j == Fb - 1 && cur < bestD) {
                        bestD = cur;
                        bestEnd = r;
                        bestSt = st;
                    }
                    mineD = cur;
                    mineS = st;
                }
                diagD = upD;
                diagS = upS;
            }
            // a valid row's last active step was column Fb - 1: what the lane carries is its entry of the profile
            if constexpr (ALL) {
                if (rowValid) {
                    a.profD[(size_t)blockIdx.x * a.slotFrames + r] = mineD;
                    a.profS[(size_t)blockIdx.x * a.slotFrames + r] = mineS;
                }
            }
        }
        // the first minimum of the end column
        SSYM_SPOT_FIRST_MIN(bestD, bestEnd, bestSt)
        if constexpr (ALL) {
            SSYM_SPOT_SELECT(a, k, Fa, lane, bestD, bestEnd, bestSt)
        } else if (lane == 0) {
            a.cost[k] = bestD;
            a.start[k] = bestSt;
            a.end[k] = bestEnd;
        }
    }
}

// Paced spotting (ssym_dtw_spot_step and its kin with SSYM_STEP_PACED; DESIGN.md 2 "Paced spotting", 5.18): the
// asymmetric step pattern with Itakura's rule.  Every target frame takes exactly one source frame; a source frame may be
// skipped but never two in a row, and repeated but never twice in a row.  Per cell two states, N (entered by a source
// step) and H (entered by repeating the source frame), and E, the better of them (strict <: a tie keeps N):
//   N(i,0) = c(i,0), sN(i,0) = i, H(i,0) = +inf;   j >= 1:  P = E(i-1,j-1), replaced by E(i-2,j-1) if that is < P;
//   N(i,j) = c(i,j) + P, sN = P's start;   H(i,j) = c(i,j) + N(i,j-1), sH = sN(i,j-1);   outside the matrix +inf.
// The cell is dtw_wave.hpp's paced cell, the one text of all six kernels of the pattern, taken here as its two macros
// (SSYM_PACED_PRED, SSYM_PACED_STATES) with the start words handed in as the statements that ride on the comparisons.
// The end column is E(., Fb-1); end, cost, start and the occurrences are taken from it as dtw_spot_kernel takes them.
//
// The wavefront is dtw_spot_kernel's.  What differs: the lane keeps (N, sN) of its previous column beside E; what passes
// between lanes is E.  E(r-1, j-1) is what shfl_up1 brought one step earlier (d1).  E(r-2, j-1) is the d1 lane l - 1 used
// one step earlier, so every step ends by moving d1 one lane up for the next step (d2): one more DPP triple, and it is taken
// AFTER lane 0 has put the hand-off row's entry into its d1, because lane 1's second diagonal is row c0 - 1, which only
// lane 0 read.  Two hand-off rows: lane 63 writes row c0 + 63 (bound1), lane 62 row c0 + 62 (bound2), both in place.
// In-place order: the lanes of a wave run in lockstep and LDS keeps a wave's accesses in order.  Lane 0 reads entry
// tau - 1 of both rows at step tau; entry x of bound1 is overwritten at step x + 63 and entry x of bound2 at step x + 62
// (lane 62 is one column ahead of lane 63), both later than step x + 1.  Only a chunk of 64 rows is followed by another,
// and it has written every entry of both rows by its last step; a pair's first chunk reads neither row (c0 = 0: +inf),
// so what the previous pair of the grid stride left there is never seen.
template <int DIMR, bool ALL = false, class Args = SpotArgs>
__global__ __launch_bounds__(64) void dtw_paced_kernel(const Args a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int LD = wave_ld(DIMR);
    double *bound1D = smem;                                         // [fbCap]   E of row c0 - 1: value ...
    double *bound2D = smem + a.fbCap;                               // [fbCap]   E of row c0 - 2: value ...
    double *ring = smem + 2 * (size_t)a.fbCap;                      // [ringRows][LD]
    uint32_t *bound1S = reinterpret_cast<uint32_t *>(ring + (size_t)a.ringRows * LD);     // [fbCap]   ... and start
    uint32_t *bound2S = bound1S + a.fbCap;                          // [fbCap]   ... and start
    const double INF = __builtin_inf();
    const int lane = threadIdx.x;
    const int dim = (int)a.dim;
    const uint32_t ringMask = a.ringRows - 1;

    for (uint32_t k = blockIdx.x; k < a.nPairs; k += gridDim.x) {
        uint2 p;
        if (a.pairs)
            p = a.pairs[k];
        else
            p = make_uint2(k / a.nTgt, k % a.nTgt);
        uint32_t Fa = 0;
        int Fb = 0;
        if (p.x != 0xffffffffu) {
            Fa = (uint32_t)(a.srcOff[p.x + 1] - a.srcOff[p.x]);
            Fb = (int)(a.tgtOff[p.y + 1] - a.tgtOff[p.y]);
        }
        if (Fa == 0 || Fb == 0) {
            if constexpr (ALL) {
                spot_all_pad(a, k, 0u);
            } else if (lane == 0) {
                a.cost[k] = INF;
                a.start[k] = 0xffffffffu;
                a.end[k] = 0xffffffffu;
            }
            continue;
        }
        const double *a0 = a.srcRaw + a.srcOff[p.x] * dim;
        const double *b0 = a.tgtRaw + a.tgtOff[p.y] * dim;

        double bestD = INF;                 // this lane's rows: the least E(r, Fb-1) so far, its row and its start
        uint32_t bestEnd = 0xffffffffu, bestSt = 0xffffffffu;
        for (uint32_t c0 = 0; c0 < Fa; c0 += 64) {
            const uint32_t r = c0 + (uint32_t)lane;
            const bool rowValid = r < Fa;
            const int rowsHere = (int)min(64u, Fa - c0);
            double ar[DIMR];
            wave_load_frame(ar, a0 + (size_t)(rowValid ? r : c0) * dim, dim);
            double mineN = INF, mineE = INF;                        // N(r, j-1), E(r, j-1)
            uint32_t mineNS = 0xffffffffu, mineES = 0xffffffffu;
            double d1D = INF, d2D = INF;                            // E(r-1, j-1), E(r-2, j-1)
            uint32_t d1S = 0xffffffffu, d2S = 0xffffffffu;
            const int tauEnd = Fb - 1 + rowsHere;     // exclusive: lane l works on column tau - l
            for (int tau = 0; tau < tauEnd; ++tau) {
                // (the refill's barrier also orders the hand-off rows, as in dtw_spot_kernel)
                if ((tau & 63) == 0)
                    wave_refill<DIMR>(ring, ringMask, b0, dim, Fb, tau);
                const int j = tau - lane;
                const double c = wave_cell_cost(ar, ring, ringMask, min(max(j, 0), Fb - 1), a.squared);
                const double upD = shfl_up1(mineE);       // E(r-1, j) and its start, for lanes >= 1: the next step's d1
                const uint32_t upS = (uint32_t)shfl_up1((int)mineES);
                if (lane == 0) {
                    d1D = d2D = INF;                      // above row 0 there is nothing
                    d1S = d2S = 0xffffffffu;
                    if (c0 != 0 && j >= 1 && j < Fb) {
                        d1D = bound1D[j - 1];
                        d1S = bound1S[j - 1];
                        d2D = bound2D[j - 1];
                        d2S = bound2S[j - 1];
                    }
                }
                // E(r-2, j) for the next step: the d1 of lane l - 1, lane 0's being what it read from the hand-off row
                const double nxD = shfl_up1(d1D);
                const uint32_t nxS = (uint32_t)shfl_up1((int)d1S);
                const bool active = rowValid && j >= 0 && j < Fb;
                if (active) {
                    double nD = c, eD = c;                // column 0: a path may start at any source frame, in state N
                    uint32_t nS = r, eS = r;
                    if (j > 0) {
                        double pD;
                        uint32_t pS = d1S;                // the start words ride on the cell's two comparisons
                        SSYM_PACED_PRED(pD, d1D, d2D, pS = d2S)
                        nS = eS = pS;
                        SSYM_PACED_STATES(nD, eD, c, pD, mineN, eS = mineNS)
                    }
                    if (lane == 63) {
                        bound1D[j] = eD;
                        bound1S[j] = eS;
                    }
                    if (lane == 62) {
                        bound2D[j] = eD;
                        bound2S[j] = eS;
                    }
                    if (j == Fb - 1 && eD < bestD) {
                        bestD = eD;
                        bestEnd = r;
                        bestSt = eS;
                    }
                    mineN = nD;
                    mineNS = nS;
                    mineE = eD;
                    mineES = eS;
                }
                d1D = upD;
                d1S = upS;
                d2D = nxD;
                d2S = nxS;
            }
            // a valid row's last active step was column Fb - 1: what the lane carries is its entry of the profile
            if constexpr (ALL) {
                if (rowValid) {
                    a.profD[(size_t)blockIdx.x * a.slotFrames + r] = mineE;
                    a.profS[(size_t)blockIdx.x * a.slotFrames + r] = mineES;
                }
            }
        }
        // the first minimum of the end column
        SSYM_SPOT_FIRST_MIN(bestD, bestEnd, bestSt)
        if constexpr (ALL) {
            SSYM_SPOT_SELECT(a, k, Fa, lane, bestD, bestEnd, bestSt)
        } else if (lane == 0) {
            a.cost[k] = bestD;
            a.start[k] = bestSt;
            a.end[k] = bestEnd;
        }
    }
}

// the best source per target of an [nSrc][nTgt] result: the first minimum over ascending source index, strict < from
// (SSYM_NO_MATCH, +inf).  One thread per target; consecutive threads read consecutive entries of a row.
__global__ __launch_bounds__(256) void spot_fold_kernel(const double *cost, const uint32_t *start, const uint32_t *end,
                                                        uint32_t nSrc, uint32_t nTgt, uint32_t indexBase,
                                                        uint32_t *outIdx, double *outCost, uint32_t *outStart,
                                                        uint32_t *outEnd)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nTgt)
        return;
    double best = __builtin_inf();
    uint32_t bi = 0xffffffffu;
    for (uint32_t s = 0; s < nSrc; ++s) {
        const double c = cost[(size_t)s * nTgt + t];
        if (c < best) {
            best = c;
            bi = s;
        }
    }
    uint32_t st = 0xffffffffu, en = 0xffffffffu;
    if (bi != 0xffffffffu) {
        st = start[(size_t)bi * nTgt + t];
        en = end[(size_t)bi * nTgt + t];
    }
    outIdx[t] = bi == 0xffffffffu ? bi : bi + indexBase;
    outCost[t] = best;
    outStart[t] = st;
    outEnd[t] = en;
}

// what every driver refuses first, in this order: no context, an unknown step, the context's metric, its band
int32_t spot_check_entry(ssym_ctx *ctx, const char *fn, uint32_t step)
{
    if (!ctx)
        return SSYM_E_INVALID;
    if (step != SSYM_STEP_SYMMETRIC && step != SSYM_STEP_PACED) {
        ctx->err = std::string(fn) + ": step must be SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED";
        return SSYM_E_INVALID;
    }
    return check_spot_ctx(ctx, fn);
}

int32_t spot_limits(ssym_ctx *ctx, const char *fn, uint64_t maxFb, uint32_t dim, uint32_t step)
{
    return check_spot_limits(ctx, fn, maxFb, dim, step == SSYM_STEP_PACED ? kPacedMaxTargetFrames : kSpotMaxTargetFrames,
                             kSpotMaxDim);
}

// the SpotArgs of a launch (SpotAllArgs' base too): pairs (device, NULL = every (source, target)) -> cost / start / end
// (device)
void spot_fill(SpotArgs &a, const ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, const uint2 *pairs,
               uint32_t n_pairs, const WaveGeom &g, double *cost, uint32_t *start, uint32_t *end)
{
    a.srcRaw = src.raw;
    a.srcOff = src.off;
    a.tgtRaw = tgt.raw;
    a.tgtOff = tgt.off;
    a.dim = src.dim;
    a.squared = ctx->squared;
    a.pairs = pairs;
    a.nTgt = tgt.n;
    a.nPairs = n_pairs;
    a.cost = cost;
    a.start = start;
    a.end = end;
    a.fbCap = g.fbCap;
    a.ringRows = g.ringRows;
}

// the kernel of `step` for a (SpotAllArgs: the one that keeps the end column) on ctx's stream, between ev[0] and ev[1]
template <class Args>
int32_t launch_spot(ssym_ctx *ctx, const Args &a, const WaveGeom &g, unsigned grid, uint32_t step)
{
    constexpr bool ALL = std::is_same<Args, SpotAllArgs>::value;
    const size_t lds = spot_lds_bytes(g, step);
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    const int32_t rc = step == SSYM_STEP_PACED
                           ? wave_launch(ctx, SSYM_WAVE_KERNEL(dtw_paced_kernel, g.dimr, ALL, Args), grid, lds, a)
                           : wave_launch(ctx, SSYM_WAVE_KERNEL(dtw_spot_kernel, g.dimr, ALL, Args), grid, lds, a);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    return SSYM_OK;
}

// what ends a call: the outputs back (the call's one synchronisation) and the timings (folded: spot_queries' fold ran
// between ev[1] and ev[2])
int32_t spot_finish(ssym_ctx *ctx, StagedOut &out, uint32_t n_pairs, bool folded = false)
{
    const int32_t rc = out.finish(ctx);
    if (rc != SSYM_OK)
        return rc;
    ssym_timings tm{};
    tm.main_ms = tm.total_ms = ev_ms(ctx->ev[0], ctx->ev[1]);
    if (folded) {
        tm.reduce_ms = ev_ms(ctx->ev[1], ctx->ev[2]);
        tm.total_ms = ev_ms(ctx->ev[0], ctx->ev[2]);
    }
    tm.main_launches = 1;
    tm.n_pairs = n_pairs;
    ctx->timings = tm;
    return SSYM_OK;
}

int32_t dtw_spot(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                 const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, double *out_cost, uint32_t *out_start,
                 uint32_t *out_end, uint32_t flags, uint32_t step = SSYM_STEP_SYMMETRIC, const char *fn = "ssym_dtw_spot")
{
    int32_t rc = spot_check_entry(ctx, fn, step);
    if (rc != SSYM_OK)
        return rc;
    rc = check_pair_list(ctx->err, fn, dict, q, src_idx, tgt_idx, n_pairs, index_base);
    if (rc != SSYM_OK || n_pairs == 0)
        return rc;
    if (!out_cost || !out_start || !out_end) {
        ctx->err = std::string(fn) + ": out_cost, out_start and out_end must not be NULL";
        return SSYM_E_INVALID;
    }
    const SegmentSet &src = dict->set, &tgt = q->set;
    // the pair list and the shape limits: on the host, before any device work
    PairList pairs(src_idx, tgt_idx, index_base, n_pairs);
    uint64_t maxFb = 0;
    for (const uint2 &p : pairs.host)
        if (p.x != SSYM_NO_MATCH && src.h_off[p.x + 1] > src.h_off[p.x])
            maxFb = std::max(maxFb, tgt.h_off[p.y + 1] - tgt.h_off[p.y]);
    rc = spot_limits(ctx, fn, maxFb, src.dim, step);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));

    Blocks bl(ctx);
    StagedOut out(flags, {{out_cost, n_pairs}}, {{out_start, n_pairs}, {out_end, n_pairs}});
    rc = out.alloc(bl);
    if (rc == SSYM_OK)
        rc = pairs.upload(ctx, bl);
    if (rc != SSYM_OK)
        return rc;
    const WaveGeom g = wave_geom(ctx, maxFb, src.dim, n_pairs);
    SpotArgs a{};
    spot_fill(a, ctx, src, tgt, pairs.dev, n_pairs, g, out.f64[0], out.u32[0], out.u32[1]);
    rc = launch_spot(ctx, a, g, g.grid, step);
    if (rc != SSYM_OK)
        return rc;
    return spot_finish(ctx, out, n_pairs);
}

int32_t dtw_spot_all(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                     const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint32_t max_spots,
                     const double *max_cost, uint32_t *out_count, double *out_cost, uint32_t *out_start, uint32_t *out_end,
                     uint32_t flags, uint32_t step = SSYM_STEP_SYMMETRIC, const char *fn = "ssym_dtw_spot_all")
{
    int32_t rc = spot_check_entry(ctx, fn, step);
    if (rc != SSYM_OK)
        return rc;
    rc = check_pair_list(ctx->err, fn, dict, q, src_idx, tgt_idx, n_pairs, index_base);
    if (rc != SSYM_OK || n_pairs == 0)
        return rc;
    if (max_spots == 0 || max_spots > kSpotAllMaxSpots) {
        ctx->err = std::string(fn) + ": max_spots must be 1 ... " + std::to_string(kSpotAllMaxSpots);
        return SSYM_E_INVALID;
    }
    if (!out_count || !out_cost || !out_start || !out_end) {
        ctx->err = std::string(fn) + ": out_count, out_cost, out_start and out_end must not be NULL";
        return SSYM_E_INVALID;
    }
    const SegmentSet &src = dict->set, &tgt = q->set;
    // the pair list, the thresholds and the shape limits: on the host, before any device work
    PairList pairs(src_idx, tgt_idx, index_base, n_pairs);
    uint64_t maxFa = 0, maxFb = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        if (max_cost && max_cost[p] != max_cost[p]) {
            ctx->err = std::string(fn) + ": max_cost[" + std::to_string(p) + "] is NaN";
            return SSYM_E_INVALID;
        }
        const uint32_t s = pairs.host[p].x, t = pairs.host[p].y;
        if (s == SSYM_NO_MATCH)
            continue;
        const uint64_t fa = src.h_off[s + 1] - src.h_off[s], fb = tgt.h_off[t + 1] - tgt.h_off[t];
        maxFa = std::max(maxFa, fa);
        if (fa)
            maxFb = std::max(maxFb, fb);
    }
    rc = spot_limits(ctx, fn, maxFb, src.dim, step);
    if (rc != SSYM_OK)
        return rc;
    if (maxFa > kSpotAllMaxSourceFrames) {
        ctx->err = std::string(fn) + ": a listed source has more than " + std::to_string(kSpotAllMaxSourceFrames) +
                   " frames (the end-column profile takes 12 bytes of scratch per source frame)";
        return SSYM_E_UNSUPPORTED;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t nOut = (size_t)n_pairs * max_spots;

    // one profile slot per workgroup, as many workgroups as kSpotAllScratchBytes holds (2 for a 2^24-frame source)
    const WaveGeom g = wave_geom(ctx, maxFb, src.dim, n_pairs);
    SpotAllArgs a{};
    a.slotFrames = std::max<uint64_t>(maxFa, 1);
    const unsigned grid = (unsigned)std::min<uint64_t>(
        g.grid, std::max<uint64_t>(1, kSpotAllScratchBytes / (a.slotFrames * (sizeof(double) + sizeof(uint32_t)))));

    Blocks bl(ctx);
    StagedOut out(flags, {{out_cost, nOut}}, {{out_start, nOut}, {out_end, nOut}, {out_count, n_pairs}});
    double *dMax = nullptr;
    if (max_cost)
        rc = bl.get(&dMax, n_pairs);
    if (rc == SSYM_OK)
        rc = bl.get(&a.profD, (size_t)grid * a.slotFrames);
    if (rc == SSYM_OK)
        rc = bl.get(&a.profS, (size_t)grid * a.slotFrames);
    if (rc == SSYM_OK)
        rc = out.alloc(bl);
    if (rc == SSYM_OK)
        rc = pairs.upload(ctx, bl);
    if (rc != SSYM_OK)
        return rc;
    if (max_cost)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dMax, max_cost, sizeof(double) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
    spot_fill(a, ctx, src, tgt, pairs.dev, n_pairs, g, out.f64[0], out.u32[0], out.u32[1]);
    a.maxSpots = max_spots;
    a.count = out.u32[2];
    a.maxCost = dMax;
    rc = launch_spot(ctx, a, g, grid, step);
    if (rc != SSYM_OK)
        return rc;
    return spot_finish(ctx, out, n_pairs);
}

int32_t spot_queries(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, uint32_t index_base, uint32_t *out_idx,
                     double *out_cost, uint32_t *out_start, uint32_t *out_end, uint32_t flags,
                     uint32_t step = SSYM_STEP_SYMMETRIC, const char *fn = "ssym_spot_queries")
{
    int32_t rc = spot_check_entry(ctx, fn, step);
    if (rc != SSYM_OK)
        return rc;
    rc = check_handles(ctx->err, fn, dict, q);
    if (rc != SSYM_OK)
        return rc;
    const SegmentSet &src = dict->set, &tgt = q->set;
    const uint32_t N = src.n, M = tgt.n;
    if (M == 0)
        return SSYM_OK;
    rc = check_sets(ctx->err, src, tgt);
    if (rc != SSYM_OK)
        return rc;
    if (!out_idx || !out_cost || !out_start || !out_end) {
        ctx->err = std::string(fn) + ": out_idx, out_cost, out_start and out_end must not be NULL";
        return SSYM_E_INVALID;
    }
    if ((uint64_t)N * M > 0xffffffffull) {
        ctx->err = std::string(fn) + ": more than 2^32 - 1 (source, target) pairs in one call";
        return SSYM_E_UNSUPPORTED;
    }
    const uint64_t maxFb = src.max_frames ? tgt.max_frames : 0;      // (sources without frames: nothing to run)
    rc = spot_limits(ctx, fn, maxFb, src.dim, step);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t nPairs = N * M;

    // every (source, target) into scratch, then the fold into the outputs
    Blocks bl(ctx);
    StagedOut out(flags, {{out_cost, M}}, {{out_idx, M}, {out_start, M}, {out_end, M}});
    double *mCost = nullptr;
    uint32_t *mSpan = nullptr;
    rc = bl.get(&mCost, nPairs);
    if (rc == SSYM_OK)
        rc = bl.get(&mSpan, 2 * (size_t)nPairs);
    if (rc == SSYM_OK)
        rc = out.alloc(bl);
    if (rc != SSYM_OK)
        return rc;
    const WaveGeom g = wave_geom(ctx, maxFb, src.dim, nPairs);
    SpotArgs a{};
    spot_fill(a, ctx, src, tgt, nullptr, nPairs, g, mCost, mSpan, mSpan + nPairs);
    rc = launch_spot(ctx, a, g, g.grid, step);
    if (rc != SSYM_OK)
        return rc;
    spot_fold_kernel<<<(M + 255) / 256, 256, 0, st>>>(mCost, mSpan, mSpan + nPairs, N, M, index_base, out.u32[0], out.f64[0],
                                                      out.u32[1], out.u32[2]);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[2], st));
    return spot_finish(ctx, out, nPairs, true);
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_dtw_spot(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                      const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, double *out_cost,
                      uint32_t *out_start, uint32_t *out_end, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_spot(ctx, dict, q, src_idx, tgt_idx, n_pairs, index_base, out_cost, out_start, out_end, flags);
    });
}

int32_t ssym_dtw_spot_all(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                          const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint32_t max_spots,
                          const double *max_cost, uint32_t *out_count, double *out_cost, uint32_t *out_start,
                          uint32_t *out_end, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_spot_all(ctx, dict, q, src_idx, tgt_idx, n_pairs, index_base, max_spots, max_cost, out_count, out_cost,
                            out_start, out_end, flags);
    });
}

int32_t ssym_spot_queries(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, uint32_t index_base,
                          uint32_t *out_idx, double *out_cost, uint32_t *out_start, uint32_t *out_end, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        return spot_queries(ctx, dict, q, index_base, out_idx, out_cost, out_start, out_end, flags);
    });
}

// the three calls above with the step pattern as an argument: SSYM_STEP_SYMMETRIC is the call above itself
int32_t ssym_dtw_spot_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                           const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint32_t step, double *out_cost,
                           uint32_t *out_start, uint32_t *out_end, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_spot(ctx, dict, q, src_idx, tgt_idx, n_pairs, index_base, out_cost, out_start, out_end, flags, step,
                        "ssym_dtw_spot_step");
    });
}

int32_t ssym_spot_queries_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, uint32_t index_base,
                               uint32_t step, uint32_t *out_idx, double *out_cost, uint32_t *out_start, uint32_t *out_end,
                               uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        return spot_queries(ctx, dict, q, index_base, out_idx, out_cost, out_start, out_end, flags, step,
                            "ssym_spot_queries_step");
    });
}

int32_t ssym_dtw_spot_all_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                               const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint32_t step,
                               uint32_t max_spots, const double *max_cost, uint32_t *out_count, double *out_cost,
                               uint32_t *out_start, uint32_t *out_end, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_spot_all(ctx, dict, q, src_idx, tgt_idx, n_pairs, index_base, max_spots, max_cost, out_count, out_cost,
                            out_start, out_end, flags, step, "ssym_dtw_spot_all_step");
    });
}

}  // extern "C"
