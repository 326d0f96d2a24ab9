// dtw_spotter.hip -- streaming DTW spotting: the targets of a query set watched in growing sources (DESIGN.md 2 "Watching",
// 5.17).
//
// Role on the path: ssym_dtw_spot / ssym_dtw_spot_all locate targets in recordings that are complete; a spotter does it for
// sources that grow.  Subsequence DTW is incremental along the source axis -- everything row i + 1 needs of rows 0 ... i is
// row i of (D, st) -- so the spotter keeps that row per (lane, target) pair in device memory, and a push costs the new rows
// alone.  Per pair it holds: the hand-off row (Fb x (f64 + u32)), the running best (ssym_dtw_spot's result for what was
// consumed so far), and the reporting state (pend, last).
//
// Forward pass (dtw_watch_kernel): dtw_spot_kernel<..., true>'s wavefront on dtw_wave.hpp's functions, one wave per pair,
// grid-stride.  What differs: row numbers are absolute (first + local row); the LDS hand-off row is loaded from the pair's
// state before the first chunk and stored back after the last; the lane that owns a chunk's bottom row writes the hand-off
// row (lane rowsHere - 1, not always lane 63); the best starts from the stored best.  The new rows' (delta, s) go to a
// profile scratch laid out [lane][target][new row], which is also the layout of the optional profile outputs.
//
// Reporting (spotter_report_kernel): the rule is sequential in i, so one thread per pair walks its new rows.  A workgroup
// serves 4 pairs: all 64 lanes load 64-row tiles of the 4 profiles into LDS (coalesced), then lanes 0 ... 3 walk their
// tile.  Events reach the caller without a capacity that could drop one: a first pass that mutates nothing counts the
// events per pair, an exclusive scan turns counts into places, the second pass writes into a log the spotter owns and
// grows, ordered by (lane, target, end).
//
// Paced watching (ssym_spotter_create_step with SSYM_STEP_PACED; DESIGN.md 2 "Paced watching", 5.20):
// dtw_watch_paced_kernel is to dtw_paced_kernel what dtw_watch_kernel is to dtw_spot_kernel.  Row i of the paced
// recurrence needs rows i - 1 and i - 2 of E alone, so the state is TWO hand-off rows per pair (24 bytes per target frame)
// and the cell is the text dtw_paced_kernel runs (dtw_wave.hpp: SSYM_PACED_PRED, SSYM_PACED_STATES); the step loop is the
// kernel's own, in the form that allows a row above a short chunk.  The reporting kernels, the log and the slices do not
// know the step.
// In-place order of the two LDS rows (bound1 = the row above the chunk, bound2 = the one above that).  A chunk of R rows
// (R = rowsHere, 1 ... 64; only R = 64 is followed by another chunk) has its bottom row in lane R - 1, which writes
// bound1[x] at step x + R - 1, and the row above it in lane R - 2, which writes bound2[x] at step x + R - 2; for R = 1
// the second row above is the OLD bound1, which lane 0 copies into bound2[x] at step x.  So entry x of either row is
// overwritten at step x at the earliest, and at step x only by lane 0 itself (bound1: R = 1; bound2: R = 1 or 2).  Lane 0
// reads entry tau of both rows at step tau, in program order BEFORE that step's stores, and uses it one step later
// (its diagonals are column j - 1 = tau - 1), carried in registers.  The lanes of a wave run in lockstep and LDS keeps a
// wave's accesses in order, so every read sees the row as the previous chunk (or the state load) left it.  Every valid
// lane is active for every column, so after a chunk both rows hold Fb fresh entries: bound1 = row c0 + R - 1, bound2 = row
// c0 + R - 2 (for first + c0 + R = 1 a row that does not exist, written as (+inf, none) and never read: "second row above
// exists" is first + c0 >= 2).  A row that does not exist yet is neither loaded from the state nor read from LDS.
//
// Host: the checks, the upload and the bodies of push / follow / flush / reset and of destroy are lane_feed.hpp's; the
// spotter hands in its feed and spotter_run, with the profile outputs of the call.  spotter_run, the event log that grows and
// is sorted, and the reads are here.
#include "dtw_wave.hpp"
#include "lane_feed.hpp"

#include <algorithm>
#include <numeric>

namespace ssym {

// Limits (soundsym_amd.h "Watching"; ssym_dtw_spot's for a target, refused by the same check_spot_limits): frames of a
// target, values per frame; the frames a lane may consume are lane_feed.hpp's kLaneMaxFrames (st is u32 and 0xffffffff
// means none: the dictionary's own limit)
constexpr uint64_t kSpotterMaxTargetFrames = 4096;
constexpr uint32_t kSpotterMaxDim = 64;
// under SSYM_STEP_PACED: dtw_spot.hip's kPacedMaxTargetFrames, for its reason (two hand-off rows and the ring within LDS)
constexpr uint64_t kSpotterPacedMaxTargetFrames = 2048;
// the profile of one forward launch stays within ssym_dtw_spot_all's scratch limit: a longer push runs as several slices
// of rows, which the carried state makes exact
constexpr size_t kSpotterScratchBytes = (size_t)512 << 20;

namespace {

constexpr uint32_t kNone = 0xffffffffu;

// what one launch consumes of a lane
struct LaneStep {
    const double *rows;          // the first new frame
    uint64_t profOff;            // the lane's place in the profile scratch: pair (l, t) starts at profOff + t * m
    uint32_t first;              // its absolute row number
    uint32_t m;                  // new rows
};

struct WatchArgs {
    const LaneStep *steps;       // [nLanes]
    const double *tgtRaw;
    const uint64_t *tgtOff;
    uint32_t dim;
    int squared;
    uint32_t nTgt;
    uint32_t nPairs;             // pair k = (lane k / nTgt, target k % nTgt)
    uint64_t sumFb;              // frames of all targets: a lane's stride in stateD / stateS
    double *stateD;              // [nLanes][sumFb]  the last consumed row of every target: D ...
    uint32_t *stateS;            //                  ... and st
    double *bestD;               // [nPairs]
    uint32_t *bestE, *bestS;     // [nPairs]
    double *profD;               // the new rows' end column: D ...
    uint32_t *profS;             // ... and st
    uint32_t fbCap;              // even, >= the longest target
    uint32_t ringRows;           // 64 or 128
};

template <int DIMR>
__global__ __launch_bounds__(64) void dtw_watch_kernel(const WatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int LD = wave_ld(DIMR);
    double *boundD = smem;                                          // [fbCap]   the row above the chunk: D ...
    double *ring = smem + a.fbCap;                                  // [ringRows][LD]
    uint32_t *boundS = reinterpret_cast<uint32_t *>(ring + (size_t)a.ringRows * LD);      // [fbCap]   ... and st
    const double INF = __builtin_inf();
    const int lane = threadIdx.x;
    const int dim = (int)a.dim;
    const uint32_t ringMask = a.ringRows - 1;

    for (uint32_t k = blockIdx.x; k < a.nPairs; k += gridDim.x) {
        const uint32_t l = k / a.nTgt, t = k % a.nTgt;
        const LaneStep s = a.steps[l];
        const int Fb = (int)(a.tgtOff[t + 1] - a.tgtOff[t]);
        if (s.m == 0 || Fb == 0)
            continue;                       // nothing new, or a target without frames: the state stays what it is
        const double *b0 = a.tgtRaw + a.tgtOff[t] * dim;
        const size_t sBase = (size_t)l * a.sumFb + a.tgtOff[t];
        const size_t pBase = s.profOff + (size_t)t * s.m;

        // hand-off row in (the barrier: the previous pair's store-back has read the row)
        __syncthreads();
        if (s.first != 0)
            for (int j = lane; j < Fb; j += 64) {
                boundD[j] = a.stateD[sBase + j];
                boundS[j] = a.stateS[sBase + j];
            }
        // every lane starts from the stored best: strict < keeps it against an equal new row, and in the reduction its
        // row number is below every new one
        double bestD = a.bestD[k];
        uint32_t bestEnd = a.bestE[k], bestSt = a.bestS[k];
        for (uint32_t c0 = 0; c0 < s.m; c0 += 64) {
            const uint32_t rl = c0 + (uint32_t)lane;
            const bool rowValid = rl < s.m;
            const uint32_t r = s.first + rl;          // the absolute row: what st and the best's end hold
            const int rowsHere = (int)min(64u, s.m - c0);
            const bool rowAbove = s.first + c0 != 0;
            double ar[DIMR];
            wave_load_frame(ar, s.rows + (size_t)(rowValid ? rl : c0) * dim, dim);
            double mineD = INF;             // D(r, j-1)
            uint32_t mineS = kNone;
            double diagD = INF;             // D(r-1, j-1)
            uint32_t diagS = kNone;
            const int tauEnd = Fb - 1 + rowsHere;     // exclusive: lane l works on column tau - l
            for (int tau = 0; tau < tauEnd; ++tau) {
                // (the refill's barrier also orders the hand-off row: the loads above and the previous chunk's writes
                // are done before tau = 0 goes on)
                if ((tau & 63) == 0)
                    wave_refill<DIMR>(ring, ringMask, b0, dim, Fb, tau);
                const int j = tau - lane;
                const double c = wave_cell_cost(ar, ring, ringMask, min(max(j, 0), Fb - 1), a.squared);
                double upD = shfl_up1(mineD);             // D(r-1, j) and its start, for lanes >= 1
                uint32_t upS = (uint32_t)shfl_up1((int)mineS);
                if (lane == 0) {
                    // the row above lane 0 is the hand-off row; its column j - 1 is what this lane read one step ago
                    // (diagD / diagS), so a bottom row in lane 0 may overwrite column j in this very step
                    upD = INF;
                    upS = kNone;
                    if (rowAbove && j < Fb) {
                        upD = boundD[j];
                        upS = boundS[j];
                    }
                }
                const double dgD = diagD;
                const uint32_t dgS = diagS;
                const bool active = rowValid && j >= 0 && j < Fb;
                if (active) {
                    double cur = c;                       // column 0: a path may start at any source frame
                    uint32_t st = r;
                    if (j > 0) {
                        cur = __dadd_rn(c, wave_min3(upD, mineD, dgD));
                        const uint32_t pred = wave_pred(upD, mineD, dgD);
                        st = pred == 0u ? dgS : pred == 1u ? upS : mineS;
                    }
                    if (lane == rowsHere - 1) {           // the chunk's bottom row
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
            if (rowValid) {
                a.profD[pBase + rl] = mineD;
                a.profS[pBase + rl] = mineS;
            }
        }
        // hand-off row out: the last chunk's bottom row, whichever lane wrote it
        __syncthreads();
        for (int j = lane; j < Fb; j += 64) {
            a.stateD[sBase + j] = boundD[j];
            a.stateS[sBase + j] = boundS[j];
        }
        SSYM_SPOT_FIRST_MIN(bestD, bestEnd, bestSt)
        if (lane == 0) {
            a.bestD[k] = bestD;
            a.bestE[k] = bestEnd;
            a.bestS[k] = bestSt;
        }
    }
}

// dtw_watch_paced_kernel's arguments: WatchArgs, with stateD / stateS holding TWO rows per (lane, target).  A struct of its
// own: dtw_watch_kernel's arguments, and with them its register figures, stay what they were.
struct WatchPacedArgs : WatchArgs {
    uint64_t rowStride;          // entries from a pair's row n - 1 to its row n - 2: nLanes * sumFb
};

// Paced watching (the file header has the order argument of the two hand-off rows).
template <int DIMR>
__global__ __launch_bounds__(64) void dtw_watch_paced_kernel(const WatchPacedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int LD = wave_ld(DIMR);
    double *bound1D = smem;                                         // [fbCap]   E of the row above the chunk: value ...
    double *bound2D = smem + a.fbCap;                               // [fbCap]   E of the row above that: value ...
    double *ring = smem + 2 * (size_t)a.fbCap;                      // [ringRows][LD]
    uint32_t *bound1S = reinterpret_cast<uint32_t *>(ring + (size_t)a.ringRows * LD);     // [fbCap]   ... and start
    uint32_t *bound2S = bound1S + a.fbCap;                          // [fbCap]   ... and start
    const double INF = __builtin_inf();
    const int lane = threadIdx.x;
    const int dim = (int)a.dim;
    const uint32_t ringMask = a.ringRows - 1;

    for (uint32_t k = blockIdx.x; k < a.nPairs; k += gridDim.x) {
        const uint32_t l = k / a.nTgt, t = k % a.nTgt;
        const LaneStep s = a.steps[l];
        const int Fb = (int)(a.tgtOff[t + 1] - a.tgtOff[t]);
        if (s.m == 0 || Fb == 0)
            continue;                       // nothing new, or a target without frames: the state stays what it is
        const double *b0 = a.tgtRaw + a.tgtOff[t] * dim;
        const size_t sBase = (size_t)l * a.sumFb + a.tgtOff[t];
        const size_t pBase = s.profOff + (size_t)t * s.m;

        // hand-off rows in, those that exist (the barrier: the previous pair's store-back has read the rows)
        __syncthreads();
        for (int j = lane; j < Fb; j += 64) {
            if (s.first >= 1) {
                bound1D[j] = a.stateD[sBase + j];
                bound1S[j] = a.stateS[sBase + j];
            }
            if (s.first >= 2) {
                bound2D[j] = a.stateD[a.rowStride + sBase + j];
                bound2S[j] = a.stateS[a.rowStride + sBase + j];
            }
        }
        // every lane starts from the stored best, as in dtw_watch_kernel
        double bestD = a.bestD[k];
        uint32_t bestEnd = a.bestE[k], bestSt = a.bestS[k];
        for (uint32_t c0 = 0; c0 < s.m; c0 += 64) {
            const uint32_t rl = c0 + (uint32_t)lane;
            const bool rowValid = rl < s.m;
            const uint32_t r = s.first + rl;          // the absolute row: what the starts and the best's end hold
            const int rowsHere = (int)min(64u, s.m - c0);
            const bool row1 = s.first + c0 >= 1;      // the row above the chunk exists ...
            const bool row2 = s.first + c0 >= 2;      // ... and the one above that
            double ar[DIMR];
            wave_load_frame(ar, s.rows + (size_t)(rowValid ? rl : c0) * dim, dim);
            double mineN = INF, mineE = INF;                        // N(r, j-1), E(r, j-1)
            uint32_t mineNS = kNone, mineES = kNone;
            double d1D = INF, d2D = INF;                            // E(r-1, j-1), E(r-2, j-1)
            uint32_t d1S = kNone, d2S = kNone;
            double in1D = INF, in2D = INF;                          // lane 0: entry tau - 1 of the two hand-off rows
            uint32_t in1S = kNone, in2S = kNone;
            const int tauEnd = Fb - 1 + rowsHere;     // exclusive: lane l works on column tau - l
            for (int tau = 0; tau < tauEnd; ++tau) {
                // (the refill's barrier also orders the hand-off rows: the loads above and the previous chunk's writes
                // are done before tau = 0 goes on)
                if ((tau & 63) == 0)
                    wave_refill<DIMR>(ring, ringMask, b0, dim, Fb, tau);
                const int j = tau - lane;
                const double c = wave_cell_cost(ar, ring, ringMask, min(max(j, 0), Fb - 1), a.squared);
                const double upD = shfl_up1(mineE);       // E(r-1, j) and its start, for lanes >= 1: the next step's d1
                const uint32_t upS = (uint32_t)shfl_up1((int)mineES);
                if (lane == 0) {
                    // its diagonals are entry tau - 1 of the hand-off rows, read one step ago; entry tau is read now,
                    // BEFORE this step's stores, which may overwrite it
                    d1D = in1D;
                    d1S = in1S;
                    d2D = in2D;
                    d2S = in2S;
                    in1D = in2D = INF;
                    in1S = in2S = kNone;
                    if (j < Fb) {
                        if (row1) {
                            in1D = bound1D[j];
                            in1S = bound1S[j];
                        }
                        if (row2) {
                            in2D = bound2D[j];
                            in2S = bound2S[j];
                        }
                    }
                }
                // E(r-2, j) for the next step: the d1 of lane l - 1, lane 0's being what it took from the hand-off row
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
                    if (rowsHere == 1) {                  // (lane 0) the row that was above becomes the second row above
                        bound2D[j] = in1D;
                        bound2S[j] = in1S;
                    }
                    if (lane == rowsHere - 1) {           // the chunk's bottom row
                        bound1D[j] = eD;
                        bound1S[j] = eS;
                    }
                    if (lane == rowsHere - 2) {           // and the row above it
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
            if (rowValid) {
                a.profD[pBase + rl] = mineE;
                a.profS[pBase + rl] = mineES;
            }
        }
        // hand-off rows out: the last chunk's two bottom rows, whichever lanes wrote them
        __syncthreads();
        for (int j = lane; j < Fb; j += 64) {
            a.stateD[sBase + j] = bound1D[j];
            a.stateS[sBase + j] = bound1S[j];
            a.stateD[a.rowStride + sBase + j] = bound2D[j];
            a.stateS[a.rowStride + sBase + j] = bound2S[j];
        }
        SSYM_SPOT_FIRST_MIN(bestD, bestEnd, bestSt)
        if (lane == 0) {
            a.bestD[k] = bestD;
            a.bestE[k] = bestEnd;
            a.bestS[k] = bestSt;
        }
    }
}

// ---- reporting ----------------------------------------------------------------------------------------------------------

constexpr int kRepPairs = 4;               // pairs per workgroup: few, so that many workgroups hide each other's latency
constexpr int kRepLd = 65;                  // LDS stride of a pair's 64-row tile: the walking lanes read distinct banks

struct ReportArgs {
    const LaneStep *steps;
    const uint64_t *tgtOff;
    uint32_t nTgt, nPairs;
    const double *profD;
    const uint32_t *profS;
    const double *maxCost;       // [nTgt] (+inf: none)
    double *pendD;               // [nPairs] the pending event (pendE = none: no event pending) ...
    uint32_t *pendS, *pendE;
    uint32_t *last;              // [nPairs] the end of the last emitted event
    uint32_t *cnt;               // [nPairs + 1]: counting pass: out, events per pair; writing pass: in, their places
    uint32_t flushLane;          // the lane whose pending events are emitted after the rows (none: 0xffffffff)
    uint64_t evBase;             // events in the log before this launch
    double *evCost;
    uint32_t *evLane, *evTgt, *evStart, *evEnd;
};

// WRITE = false: count the events the rows (and the flush) emit, mutate nothing.  WRITE = true: emit them and store the state.
template <bool WRITE>
__global__ __launch_bounds__(64) void spotter_report_kernel(const ReportArgs a)
{
    __shared__ double tD[kRepPairs * kRepLd];
    __shared__ uint32_t tS[kRepPairs * kRepLd];
    __shared__ uint64_t sBase[kRepPairs];
    __shared__ uint32_t sM[kRepPairs];
    const uint32_t lane = threadIdx.x;
    const uint64_t k64 = (uint64_t)blockIdx.x * kRepPairs + lane;
    const bool mine = lane < (uint32_t)kRepPairs && k64 < a.nPairs;
    const uint32_t k = (uint32_t)k64;
    uint32_t m = 0, first = 0, l = 0, t = 0;
    bool flush = false;
    double pendD = __builtin_inf(), limit = 0.0;
    uint32_t pendS = kNone, pendE = kNone, last = kNone;
    if (lane < (uint32_t)kRepPairs) {
        uint64_t base = 0;
        if (mine) {
            l = k / a.nTgt;
            t = k % a.nTgt;
            const LaneStep s = a.steps[l];
            if (a.tgtOff[t + 1] > a.tgtOff[t]) {      // (a target without frames has no rows and nothing pending)
                m = s.m;
                first = s.first;
                base = s.profOff + (uint64_t)t * s.m;
                flush = l == a.flushLane;
            }
            pendD = a.pendD[k];
            pendS = a.pendS[k];
            pendE = a.pendE[k];
            last = a.last[k];
            limit = a.maxCost[t];
        }
        sM[lane] = m;
        sBase[lane] = base;
    }
    __syncthreads();
    uint32_t maxM = 0;
    for (int p = 0; p < kRepPairs; ++p)
        maxM = max(maxM, sM[p]);
    uint32_t n = 0;                                   // events so far
    const uint64_t place = WRITE && mine ? a.evBase + a.cnt[k] : 0;
    auto emit = [&]() {
        if constexpr (WRITE) {
            a.evCost[place + n] = pendD;
            a.evLane[place + n] = l;
            a.evTgt[place + n] = t;
            a.evStart[place + n] = pendS;
            a.evEnd[place + n] = pendE;
        }
        ++n;
        last = pendE;
        pendE = kNone;
    };
    for (uint32_t x0 = 0; x0 < maxM; x0 += 64) {
        for (int p = 0; p < kRepPairs; ++p)
            if (x0 + lane < sM[p]) {
                tD[p * kRepLd + lane] = a.profD[sBase[p] + x0 + lane];
                tS[p * kRepLd + lane] = a.profS[sBase[p] + x0 + lane];
            }
        __syncthreads();
        if (x0 < m) {                                 // (m = 0 beyond the walking lanes)
            const uint32_t rows = min(64u, m - x0);
            // eight rows' LDS reads at a time, ahead of the rule's serial chain (entries beyond `rows` are inside the
            // tile and not looked at)
            for (uint32_t xb = 0; xb < rows; xb += 8) {
                double dv[8];
                uint32_t sv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    dv[u] = tD[lane * kRepLd + xb + u];
                    sv[u] = tS[lane * kRepLd + xb + u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (xb + u >= rows)
                        break;
                    const double d = dv[u];
                    const uint32_t s = sv[u];
                    if (pendE != kNone && s > pendE)
                        emit();
                    const bool cand = d < __builtin_inf() && d > -__builtin_inf() && d <= limit && (last == kNone || s > last);
                    if (cand && (pendE == kNone || d < pendD)) {
                        pendD = d;
                        pendS = s;
                        pendE = first + x0 + xb + u;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (flush && pendE != kNone)
        emit();
    if (mine) {
        if constexpr (WRITE) {
            a.pendD[k] = pendD;
            a.pendS[k] = pendS;
            a.pendE[k] = pendE;
            a.last[k] = last;
        } else {
            a.cnt[k] = n;
        }
    }
}

// The profile rows of the targets without frames, the workgroups taking the pairs in turn: (+inf, none).  The watch kernels skip such a
// pair, and the profile scratch is a cached block that goes to the caller's profile outputs as it stands: without this
// those rows held whatever the context ran before.  Launched only for a query set that has such a target, and only
// when a profile output is asked for (the reporting pass never reads these rows).
__global__ __launch_bounds__(64) void spotter_no_frames_kernel(const LaneStep *__restrict__ steps,
                                                               const uint64_t *__restrict__ tgtOff, uint32_t nTgt,
                                                               uint32_t nPairs, double *__restrict__ profD,
                                                               uint32_t *__restrict__ profS)
{
    for (uint32_t k = blockIdx.x; k < nPairs; k += gridDim.x) {
        const uint32_t l = k / nTgt, t = k % nTgt;
        if (tgtOff[t + 1] != tgtOff[t])
            continue;
        const LaneStep s = steps[l];
        const size_t pBase = s.profOff + (size_t)t * s.m;
        for (uint32_t rl = threadIdx.x; rl < s.m; rl += 64) {
            profD[pBase + rl] = __builtin_inf();
            profS[pBase + rl] = kNone;
        }
    }
}

// cnt[0 ... n - 1] -> its exclusive prefix sums in place, the total in cnt[n].  One workgroup: thread i sums a run of
// consecutive entries, the 1024 sums are scanned in LDS, the run is rewritten.
__global__ __launch_bounds__(1024) void spotter_scan_kernel(uint32_t *cnt, uint32_t n)
{
    __shared__ uint32_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = (uint32_t)min((uint64_t)tid * per, (uint64_t)n), hi = (uint32_t)min((uint64_t)lo + per, (uint64_t)n);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i)
        sum += cnt[i];
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = cnt[i];
        cnt[i] = run;
        run += c;
    }
    if (tid == 1023u)
        cnt[n] = part[1023];
}

struct InitArgs {
    double *bestD, *pendD;
    uint32_t *bestE, *bestS, *pendS, *pendE, *last;
};

// pairs first ... first + n - 1 back to "nothing consumed"
__global__ __launch_bounds__(256) void spotter_init_kernel(const InitArgs a, uint32_t first, uint32_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    const size_t k = (size_t)first + i;
    a.bestD[k] = a.pendD[k] = __builtin_inf();
    a.bestE[k] = a.bestS[k] = a.pendS[k] = a.pendE[k] = a.last[k] = kNone;
}

}  // namespace
}  // namespace ssym

struct ssym_spotter {
    ssym_ctx *ctx = nullptr;
    const ssym_queries *q = nullptr;
    uint32_t nLanes = 0, nTgt = 0, nPairs = 0;
    uint32_t step = SSYM_STEP_SYMMETRIC;     // what the forward launch and the state's size go by
    std::vector<uint64_t> consumed;          // frames per lane
    // device, allocated at creation
    double *stateD = nullptr;                // [nLanes][sumFb]; paced: [2][nLanes][sumFb], row n - 1 then row n - 2
    uint32_t *stateS = nullptr;
    double *pairD = nullptr;                 // [2][nPairs]: bestD, pendD
    uint32_t *pairW = nullptr;               // [5][nPairs]: bestE, bestS, pendS, pendE, last
    double *maxCost = nullptr;               // [nTgt]
    ssym::LaneStep *dSteps = nullptr;        // [nLanes]
    uint32_t *dCnt = nullptr;                // [nPairs + 1]
    // the event log: the events of the last push / follow / flush
    double *evCost = nullptr;                // [evCap]
    uint32_t *evWords = nullptr;             // [4][evCap]: lane, target, start, end
    uint64_t evCap = 0, nEvents = 0;
    std::vector<ssym::LaneStep> hSteps;
};

namespace ssym {
namespace {

InitArgs init_args(const ssym_spotter *sp)
{
    const size_t n = sp->nPairs;
    return InitArgs{sp->pairD, sp->pairD + n, sp->pairW, sp->pairW + n, sp->pairW + 2 * n, sp->pairW + 3 * n, sp->pairW + 4 * n};
}

void spotter_free(ssym_ctx *ctx, ssym_spotter *sp)
{
    for (void *p : {(void *)sp->stateD, (void *)sp->stateS, (void *)sp->pairD, (void *)sp->pairW, (void *)sp->maxCost,
                    (void *)sp->dSteps, (void *)sp->dCnt, (void *)sp->evCost, (void *)sp->evWords})
        if (p)
            dev_free(ctx, p);
    delete sp;
}

constexpr const char *kNoun = "spotter";

// the spotter as the lane feed (lane_feed.hpp) sees it: lanes never end, and without pairs a push has nothing to upload
LaneFeed feed_of(ssym_ctx *, const ssym_spotter *sp)
{
    return LaneFeed{kNoun, "out_n_events", sp->nLanes, sp->q->set.dim, sp->consumed, nullptr, sp->nPairs != 0, nullptr};
}

// fn: ssym_spotter_create (step = SSYM_STEP_SYMMETRIC) or ssym_spotter_create_step
int32_t spotter_create(ssym_ctx *ctx, const ssym_queries *q, uint32_t n_lanes, const double *max_cost, uint32_t step,
                       ssym_spotter **out, const char *fn)
{
    if (!out) {
        ctx->err = std::string(fn) + ": out is NULL";
        return SSYM_E_INVALID;
    }
    *out = nullptr;
    if (step != SSYM_STEP_SYMMETRIC && step != SSYM_STEP_PACED) {
        ctx->err = std::string(fn) + ": step must be SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED";
        return SSYM_E_INVALID;
    }
    int32_t rc = check_spot_ctx(ctx, fn);
    if (rc != SSYM_OK)
        return rc;
    if (!q || n_lanes == 0) {
        ctx->err = std::string(fn) + ": the queries handle is NULL or n_lanes is 0";
        return SSYM_E_INVALID;
    }
    const SegmentSet &tgt = q->set;
    if (max_cost)
        for (uint32_t t = 0; t < tgt.n; ++t)
            if (max_cost[t] != max_cost[t]) {
                ctx->err = std::string(fn) + ": max_cost[" + std::to_string(t) + "] is NaN";
                return SSYM_E_INVALID;
            }
    rc = check_spot_limits(ctx, fn, tgt.n ? tgt.max_frames : 0, tgt.dim,
                           step == SSYM_STEP_PACED ? kSpotterPacedMaxTargetFrames : kSpotterMaxTargetFrames, kSpotterMaxDim);
    if (rc != SSYM_OK)
        return rc;
    if ((uint64_t)n_lanes * tgt.n > 0xfffffffeull) {
        ctx->err = std::string(fn) + ": more than 2^32 - 2 (lane, target) pairs";
        return SSYM_E_UNSUPPORTED;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ssym_spotter *sp = new ssym_spotter;
    sp->ctx = ctx;
    sp->q = q;
    sp->nLanes = n_lanes;
    sp->nTgt = tgt.n;
    sp->nPairs = n_lanes * tgt.n;
    sp->step = step;
    sp->consumed.assign(n_lanes, 0);
    sp->hSteps.resize(n_lanes);
    const size_t nState = (size_t)n_lanes * tgt.total_frames * (step == SSYM_STEP_PACED ? 2 : 1), nP = sp->nPairs;
    rc = alloc_n(ctx, &sp->stateD, nState);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &sp->stateS, nState);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &sp->pairD, 2 * nP);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &sp->pairW, 5 * nP);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &sp->maxCost, (size_t)tgt.n);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &sp->dSteps, (size_t)n_lanes);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &sp->dCnt, nP + 1);
    if (rc != SSYM_OK) {
        spotter_free(ctx, sp);
        return rc;
    }
    hipStream_t st = ctx->stream;
    std::vector<double> limits(tgt.n, __builtin_inf());
    if (max_cost)
        std::copy(max_cost, max_cost + tgt.n, limits.begin());
    hipError_t e = hipSuccess;
    if (tgt.n)
        e = hipMemcpyAsync(sp->maxCost, limits.data(), sizeof(double) * tgt.n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && nP) {
        spotter_init_kernel<<<(unsigned)((nP + 255) / 256), 256, 0, st>>>(init_args(sp), 0u, (uint32_t)nP);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        ctx->err = std::string(fn) + ": " + hipGetErrorString(e);
        spotter_free(ctx, sp);
        return SSYM_E_HIP;
    }
    *out = sp;
    return SSYM_OK;
}

// room for `need` events; the events the log holds are kept
int32_t grow_log(ssym_ctx *ctx, ssym_spotter *sp, uint64_t need)
{
    if (need <= sp->evCap)
        return SSYM_OK;
    const uint64_t cap = std::max<uint64_t>(need, std::max<uint64_t>(2 * sp->evCap, 1024));
    double *nc = nullptr;
    uint32_t *nw = nullptr;
    int32_t rc = alloc_n(ctx, &nc, cap);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &nw, 4 * cap);
    if (rc != SSYM_OK) {
        if (nc)
            dev_free(ctx, nc);
        return rc;
    }
    hipStream_t st = ctx->stream;
    if (sp->nEvents) {
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(nc, sp->evCost, sizeof(double) * sp->nEvents, hipMemcpyDeviceToDevice, st));
        for (int w = 0; w < 4; ++w)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(nw + w * cap, sp->evWords + w * sp->evCap, sizeof(uint32_t) * sp->nEvents,
                                               hipMemcpyDeviceToDevice, st));
    }
    if (sp->evCost)
        dev_free(ctx, sp->evCost);       // (reuse of a cached block is ordered by the context's stream)
    if (sp->evWords)
        dev_free(ctx, sp->evWords);
    sp->evCost = nc;
    sp->evWords = nw;
    sp->evCap = cap;
    return SSYM_OK;
}

// after a push that ran as several slices: the log holds slice after slice, each ordered by (lane, target, end); a stable
// sort by (lane, target) on the host puts the whole in that order
int32_t sort_log(ssym_ctx *ctx, ssym_spotter *sp)
{
    const size_t n = sp->nEvents, cap = sp->evCap;
    hipStream_t st = ctx->stream;
    std::vector<double> cost(n), cost2(n);
    std::vector<uint32_t> w(4 * n), w2(4 * n);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(cost.data(), sp->evCost, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    for (int x = 0; x < 4; ++x)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(w.data() + x * n, sp->evWords + x * cap, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
        return w[x] != w[y] ? w[x] < w[y] : w[n + x] < w[n + y];
    });
    for (size_t i = 0; i < n; ++i) {
        cost2[i] = cost[order[i]];
        for (int x = 0; x < 4; ++x)
            w2[x * n + i] = w[x * n + order[i]];
    }
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(sp->evCost, cost2.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    for (int x = 0; x < 4; ++x)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(sp->evWords + x * cap, w2.data() + x * n, sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return SSYM_OK;
}

size_t scratch_limit()
{
    const char *k = ssym_knob("SSYM_SPOTTER_SCRATCH_BYTES");      // tests: force the slice path with a small limit
    const long long v = k ? atoll(k) : 0;
    return v > 0 ? (size_t)v : kSpotterScratchBytes;
}

// Consume m[l] frames at rows[l] for every lane (checked by the caller), then emit what lane flush_lane has pending
// (kNone: no flush).  Rows, counting pass, scan | synchronise, grow the log | writing pass, outputs | synchronise -- per
// slice of rows.
int32_t spotter_run(ssym_ctx *ctx, ssym_spotter *sp, const std::vector<const double *> &rows, const std::vector<uint64_t> &m,
                    uint32_t flush_lane, uint32_t flags, uint64_t *out_n_events, double *out_prof_d, uint32_t *out_prof_s)
{
    const SegmentSet &tgt = sp->q->set;
    const uint32_t nL = sp->nLanes, nT = sp->nTgt;
    hipStream_t st = ctx->stream;
    sp->nEvents = 0;
    ssym_timings tm{};
    tm.n_pairs = sp->nPairs;
    uint64_t maxM = 0, sumM = 0;
    uint32_t active = 0;
    for (uint32_t l = 0; l < nL; ++l) {
        maxM = std::max(maxM, m[l]);
        sumM += m[l];
        active += m[l] != 0;
    }
    if (sp->nPairs == 0 || (maxM == 0 && flush_lane == kNone)) {
        for (uint32_t l = 0; l < nL; ++l)
            sp->consumed[l] += m[l];
        *out_n_events = 0;
        ctx->timings = tm;
        return SSYM_OK;
    }
    // rows of a lane per slice: the slice's profile, 12 bytes per (pair, row), stays within the limit
    uint64_t R = std::max<uint64_t>(maxM, 1);
    const uint64_t room = scratch_limit() / (sizeof(double) + sizeof(uint32_t));
    if (sumM * nT > room)
        R = std::max<uint64_t>(1, room / ((uint64_t)nT * active));
    const uint64_t nSlices = std::max<uint64_t>(1, (maxM + R - 1) / R);
    uint64_t profRows = 0;
    for (uint32_t l = 0; l < nL; ++l)
        profRows += std::min(R, m[l]);
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;
    const hipMemcpyKind outKind = outDev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;

    Blocks bl(ctx);
    double *profD = nullptr;
    uint32_t *profS = nullptr;
    int32_t rc = bl.get(&profD, (size_t)profRows * nT);
    if (rc == SSYM_OK)
        rc = bl.get(&profS, (size_t)profRows * nT);
    if (rc != SSYM_OK)
        return rc;
    const size_t nP = sp->nPairs;
    const InitArgs ia = init_args(sp);

    WatchPacedArgs wa{};                     // (the symmetric launch takes its WatchArgs base)
    wa.steps = sp->dSteps;
    wa.tgtRaw = tgt.raw;
    wa.tgtOff = tgt.off;
    wa.dim = tgt.dim;
    wa.squared = ctx->squared;
    wa.nTgt = nT;
    wa.nPairs = sp->nPairs;
    wa.sumFb = tgt.total_frames;
    wa.stateD = sp->stateD;
    wa.stateS = sp->stateS;
    wa.bestD = ia.bestD;
    wa.bestE = ia.bestE;
    wa.bestS = ia.bestS;
    wa.profD = profD;
    wa.profS = profS;
    const WaveGeom g = wave_geom(ctx, tgt.max_frames, tgt.dim, nP);
    wa.fbCap = g.fbCap;
    wa.ringRows = g.ringRows;
    wa.rowStride = (uint64_t)nL * tgt.total_frames;
    const size_t lds = spot_lds_bytes(g, sp->step);                  // one hand-off row, or the paced pattern's two
    const unsigned repGrid = (unsigned)((nP + kRepPairs - 1) / kRepPairs);

    ReportArgs ra{};
    ra.steps = sp->dSteps;
    ra.tgtOff = tgt.off;
    ra.nTgt = nT;
    ra.nPairs = sp->nPairs;
    ra.profD = profD;
    ra.profS = profS;
    ra.maxCost = sp->maxCost;
    ra.pendD = ia.pendD;
    ra.pendS = ia.pendS;
    ra.pendE = ia.pendE;
    ra.last = ia.last;
    ra.cnt = sp->dCnt;

    bool emptyTarget = false;                // a target without frames: no kernel writes its rows of the profile
    for (uint32_t t = 0; t < nT; ++t)
        emptyTarget = emptyTarget || tgt.h_off[t + 1] == tgt.h_off[t];
    uint64_t outLane = 0;                    // where a lane's profile starts in the outputs: [lane][target][new row]
    std::vector<uint64_t> outOff(nL);
    for (uint32_t l = 0; l < nL; ++l) {
        outOff[l] = outLane;
        outLane += m[l] * nT;
    }
    for (uint64_t sl = 0; sl < nSlices; ++sl) {
        uint64_t off = 0;
        bool any = false;
        for (uint32_t l = 0; l < nL; ++l) {
            const uint64_t s0 = std::min(sl * R, m[l]), ms = std::min(R, m[l] - s0);
            LaneStep &h = sp->hSteps[l];
            h.rows = ms ? rows[l] + s0 * tgt.dim : nullptr;
            h.profOff = off;
            h.first = (uint32_t)(sp->consumed[l] + s0);
            h.m = (uint32_t)ms;
            off += ms * nT;
            any = any || ms != 0;
        }
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(sp->dSteps, sp->hSteps.data(), sizeof(LaneStep) * nL, hipMemcpyHostToDevice, st));
        SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], st));
        if (any) {
            rc = sp->step == SSYM_STEP_PACED
                     ? wave_launch(ctx, SSYM_WAVE_KERNEL(dtw_watch_paced_kernel, g.dimr), g.grid, lds, wa)
                     : wave_launch<WatchArgs>(ctx, SSYM_WAVE_KERNEL(dtw_watch_kernel, g.dimr), g.grid, lds, wa);
            if (rc != SSYM_OK)
                return rc;
        }
        SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[1], st));
        ra.flushLane = sl + 1 == nSlices ? flush_lane : kNone;
        ra.evBase = sp->nEvents;
        spotter_report_kernel<false><<<repGrid, 64, 0, st>>>(ra);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        spotter_scan_kernel<<<1, 1024, 0, st>>>(sp->dCnt, sp->nPairs);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[2], st));
        uint32_t total = 0;
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(&total, sp->dCnt + nP, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        rc = grow_log(ctx, sp, sp->nEvents + total);
        if (rc != SSYM_OK)
            return rc;
        ra.evCost = sp->evCost;
        ra.evLane = sp->evWords;
        ra.evTgt = sp->evWords + sp->evCap;
        ra.evStart = sp->evWords + 2 * sp->evCap;
        ra.evEnd = sp->evWords + 3 * sp->evCap;
        SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[3], st));
        spotter_report_kernel<true><<<repGrid, 64, 0, st>>>(ra);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[4], st));
        sp->nEvents += total;
        // the slice's profile into the outputs: one piece when the call is one slice, else per lane a strided copy
        if (any && (out_prof_d || out_prof_s)) {
            if (emptyTarget) {
                spotter_no_frames_kernel<<<(unsigned)std::min<size_t>(nP, 65536), 64, 0, st>>>(sp->dSteps, tgt.off, nT, sp->nPairs,
                                                                                              profD, profS);
                SSYM_HIP_CHECK(ctx, hipGetLastError());
            }
            if (nSlices == 1) {
                if (out_prof_d)
                    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_prof_d, profD, sizeof(double) * off, outKind, st));
                if (out_prof_s)
                    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_prof_s, profS, sizeof(uint32_t) * off, outKind, st));
            } else {
                for (uint32_t l = 0; l < nL; ++l) {
                    const LaneStep &h = sp->hSteps[l];
                    if (!h.m)
                        continue;
                    const uint64_t s0 = std::min(sl * R, m[l]);
                    if (out_prof_d)
                        SSYM_HIP_CHECK(ctx, hipMemcpy2DAsync(out_prof_d + outOff[l] + s0, sizeof(double) * m[l], profD + h.profOff,
                                                             sizeof(double) * h.m, sizeof(double) * h.m, nT, outKind, st));
                    if (out_prof_s)
                        SSYM_HIP_CHECK(ctx, hipMemcpy2DAsync(out_prof_s + outOff[l] + s0, sizeof(uint32_t) * m[l], profS + h.profOff,
                                                             sizeof(uint32_t) * h.m, sizeof(uint32_t) * h.m, nT, outKind, st));
                }
            }
        }
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        tm.main_ms += ev_ms(ctx->ev[0], ctx->ev[1]);
        tm.reduce_ms += ev_ms(ctx->ev[1], ctx->ev[2]) + ev_ms(ctx->ev[3], ctx->ev[4]);
        tm.main_launches += any ? 1 : 0;
    }
    for (uint32_t l = 0; l < nL; ++l)
        sp->consumed[l] += m[l];
    if (nSlices > 1 && sp->nEvents > 1) {
        rc = sort_log(ctx, sp);
        if (rc != SSYM_OK)
            return rc;
    }
    tm.total_ms = tm.main_ms + tm.reduce_ms;
    ctx->timings = tm;
    *out_n_events = sp->nEvents;
    return SSYM_OK;
}

// what push, follow and flush hand to the entry bodies (lane_feed.hpp) beside the feed: the run with the profile outputs of
// the call (a flush has none)
auto spotter_runner(ssym_ctx *ctx, ssym_spotter *sp, uint32_t flags, uint64_t *out_n_events, double *out_prof_d, uint32_t *out_prof_s)
{
    static_assert(kNone == kLaneNone, "a call without a flush names the same lane to the feed and to the run");
    return [=](const char *, const std::vector<const double *> &rows, const std::vector<uint64_t> &m, uint32_t flushLane) {
        return spotter_run(ctx, sp, rows, m, flushLane, flags, out_n_events, out_prof_d, out_prof_s);
    };
}

int32_t spotter_events(ssym_ctx *ctx, const ssym_spotter *sp, uint32_t *out_lane, uint32_t *out_target, double *out_cost,
                       uint32_t *out_start, uint32_t *out_end, uint32_t flags)
{
    int32_t rc = check_handle(ctx, sp, kNoun, "ssym_spotter_events");
    if (rc != SSYM_OK || sp->nEvents == 0)
        return rc;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;
    const size_t n = sp->nEvents, cap = sp->evCap;
    rc = copy_out(ctx, out_cost, sp->evCost, n, outDev);
    uint32_t *const outs[4] = {out_lane, out_target, out_start, out_end};
    for (int w = 0; w < 4 && rc == SSYM_OK; ++w)
        rc = copy_out(ctx, outs[w], sp->evWords + w * cap, n, outDev);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
}

int32_t spotter_best(ssym_ctx *ctx, const ssym_spotter *sp, double *out_cost, uint32_t *out_start, uint32_t *out_end,
                     uint32_t flags)
{
    int32_t rc = check_handle(ctx, sp, kNoun, "ssym_spotter_best");
    if (rc != SSYM_OK || sp->nPairs == 0)
        return rc;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;
    const InitArgs ia = init_args(sp);
    rc = copy_out(ctx, out_cost, (const double *)ia.bestD, sp->nPairs, outDev);
    if (rc == SSYM_OK)
        rc = copy_out(ctx, out_start, (const uint32_t *)ia.bestS, sp->nPairs, outDev);
    if (rc == SSYM_OK)
        rc = copy_out(ctx, out_end, (const uint32_t *)ia.bestE, sp->nPairs, outDev);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_spotter_create(ssym_ctx *ctx, const ssym_queries *q, uint32_t n_lanes, const double *max_cost, ssym_spotter **out)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        return spotter_create(ctx, q, n_lanes, max_cost, SSYM_STEP_SYMMETRIC, out, "ssym_spotter_create");
    });
}

int32_t ssym_spotter_create_step(ssym_ctx *ctx, const ssym_queries *q, uint32_t n_lanes, const double *max_cost,
                                 uint32_t step, ssym_spotter **out)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        return spotter_create(ctx, q, n_lanes, max_cost, step, out, "ssym_spotter_create_step");
    });
}

int32_t ssym_spotter_destroy(ssym_ctx *ctx, ssym_spotter *sp)
{
    return lane_destroy(ctx, sp, spotter_free);
}

int32_t ssym_spotter_push(ssym_ctx *ctx, ssym_spotter *sp, const double *feats, const uint64_t *frame_offsets, uint32_t flags,
                          uint64_t *out_n_events, double *out_profile_cost, uint32_t *out_profile_start)
{
    return lane_push(ctx, sp, kNoun, "ssym_spotter_push", feed_of, feats, frame_offsets, out_n_events,
                     spotter_runner(ctx, sp, flags, out_n_events, out_profile_cost, out_profile_start));
}

int32_t ssym_spotter_follow(ssym_ctx *ctx, ssym_spotter *sp, const ssym_stream *stream, uint32_t flags,
                            uint64_t *out_n_events, double *out_profile_cost, uint32_t *out_profile_start)
{
    return lane_follow(ctx, sp, kNoun, "ssym_spotter_follow", feed_of, stream, out_n_events,
                       spotter_runner(ctx, sp, flags, out_n_events, out_profile_cost, out_profile_start));
}

int32_t ssym_spotter_events(ssym_ctx *ctx, const ssym_spotter *sp, uint32_t *out_lane, uint32_t *out_target, double *out_cost,
                            uint32_t *out_start, uint32_t *out_end, uint32_t flags)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        return spotter_events(ctx, sp, out_lane, out_target, out_cost, out_start, out_end, flags);
    });
}

int32_t ssym_spotter_flush(ssym_ctx *ctx, ssym_spotter *sp, uint32_t lane, uint64_t *out_n_events)
{
    return lane_flush(ctx, sp, kNoun, "ssym_spotter_flush", feed_of, lane, out_n_events,
                      spotter_runner(ctx, sp, 0, out_n_events, nullptr, nullptr));
}

int32_t ssym_spotter_best(ssym_ctx *ctx, const ssym_spotter *sp, double *out_cost, uint32_t *out_start, uint32_t *out_end,
                          uint32_t flags)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return spotter_best(ctx, sp, out_cost, out_start, out_end, flags); });
}

int32_t ssym_spotter_counts(const ssym_spotter *sp, uint64_t *out_frames)
{
    if (!sp || !out_frames)
        return SSYM_E_INVALID;
    std::copy(sp->consumed.begin(), sp->consumed.end(), out_frames);
    return SSYM_OK;
}

int32_t ssym_spotter_reset(ssym_ctx *ctx, ssym_spotter *sp, uint32_t lane)
{
    return lane_reset(ctx, sp, kNoun, "ssym_spotter_reset", feed_of, lane, [&]() -> int32_t {
        if (sp->nTgt) {
            spotter_init_kernel<<<(sp->nTgt + 255) / 256, 256, 0, ctx->stream>>>(init_args(sp), lane * sp->nTgt, sp->nTgt);
            SSYM_HIP_CHECK(ctx, hipGetLastError());
            SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        }
        sp->consumed[lane] = 0;
        return SSYM_OK;
    });
}

}  // extern "C"
