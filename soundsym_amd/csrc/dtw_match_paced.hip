// dtw_match_paced.hip -- paced matching: for every target the dictionary segment with the least cost under the paced
// step pattern, and the matrix of those costs (DESIGN.md 2 "Paced matching", 5.21).
//
// Role on the path: ssym_match_queries minimises the symmetric DTW cost; the pair it picks may have no paced path at all
// (a source of more than twice the target's frames), so a caller that aligns under the paced pattern searches under it
// too.  Neither cost bounds the other (a paced step that skips a source frame is no symmetric step), so the f16 filter
// cannot go in front: every shape-feasible pair is evaluated exactly.
//
// Definition.  For source s (Fa frames) and target t (Fb frames), cost(s, t) is the cost of "Paced alignment"
// (dtw_align.hip, dtw_align_paced_kernel), all of it:
//   shape   : Fa = 0, Fb = 0, or Fa outside floor((Fb-1)/2) + 1 ... 2 Fb - 1  ->  +inf, decided before the recurrence
//   N(0,0) = c(0,0);  N(i,0) = +inf for i >= 1;  H(i,0) = +inf
//   E(i,j) = N(i,j); if H(i,j) < N(i,j): H(i,j)                       (strict <)
//   j >= 1:  P = E(i-1,j-1); if E(i-2,j-1) < P: E(i-2,j-1)             (strict <; outside the matrix = +inf)
//            N(i,j) = c(i,j) + P;   H(i,j) = c(i,j) + N(i,j-1)
//   cost    = E(Fa-1,Fb-1)
// in dtw_wave.hpp's arithmetic (f64, k ascending, every sub, mul, add and sqrt rounded separately, no contraction, the
// context's squared option), over the whole matrix.  Per target, ssym_match_queries' dtw rule:
//   idx[t] = argmin_s |cost(s,t) - distance[t]|   (distance NULL = 0), the first minimum, the fold starting at (0, +inf):
//   a NaN or +inf key never wins, out_cost is the winner's cost, a target nothing beats gets 0 + index_base and +inf.
//
// Mapping: a cost-only forward pass on dtw_wave.hpp's pieces.  The cell is the one text dtw_align_paced_kernel runs too
// (SSYM_PACED_PRED, SSYM_PACED_STATES), on its wavefront (d1 / d2 by DPP, two f64 hand-off rows for a source of more than 64
// frames); no codes, no slabs, no backward walk.
//   packing   a wave serves ONE target and several sources at once: consecutive shape-feasible sources of <= 64 frames
//             lie side by side in the 64 lanes (a 5 ... 40-frame dictionary: 2 - 8 pairs per wave), all reading the same
//             target ring.  A lane knows its source, its local row r and Fa, and works on column tau - r.  The lane at
//             local row 0 takes d1 = d2 = +inf and, through it, the lane at local row 1 takes d2 = +inf: never the
//             neighbour's values, which belong to another source.  tauEnd = Fb - 1 + the rows of the pack's longest
//             source.  A source of more than 64 frames runs alone, in 64-row chunks.  A pair without a paced shape costs
//             +inf without touching a frame.  A target that fits the ring stays in it for all of a block's packs.
//   fold      every lane keeps the first minimum (key, index) of the pairs that ended in it; the wave reduces them by
//             (key, index).  Grid = targets x source blocks; partial results go to [blocks][targets] scratch and
//             match_paced_fold_kernel applies the first-minimum rule across blocks in index order, so the answer depends
//             neither on the grid nor on how sources fall into packs and blocks.
//   matrix    the same kernel stores every pair's cost (ssym_pair_matrix_step).
#include "dtw_wave.hpp"

#include <algorithm>

namespace ssym {

// Limits of paced matching (soundsym_amd.h): ssym_dtw_align_step's under SSYM_STEP_PACED, so that every
// reported match can be aligned
constexpr int kMatchPacedMaxSrcFrames = 4096;
constexpr int kMatchPacedMaxTgtFrames = 2048;
constexpr int kMatchPacedMaxDim = 64;
// sources per block: at least kBlockMin (a pack needs neighbours, a resident target ring needs users), at most kBlockMax
// (the tail of a launch is one block long); in between, as many as leave kMatchPacedWavesPerCu waves per CU to balance
// the load (measured: DESIGN.md 5.21's table of block sizes)
constexpr uint32_t kMatchPacedBlockMin = 8, kMatchPacedBlockMax = 128;
constexpr uint32_t kMatchPacedWavesPerCu = 128;
// grid: targets beyond gridX are reached by a stride; blocks x gridX x 64 threads stays below 2^32
constexpr uint32_t kMatchPacedGridX = 65536, kMatchPacedGridY = 1023;

namespace {

constexpr uint32_t kNone = 0xffffffffu;

struct MatchPacedArgs {
    const double *srcRaw;
    const uint64_t *srcOff;
    uint32_t nSrc;
    const double *tgtRaw;
    const uint64_t *tgtOff;
    uint32_t nTgt;
    uint32_t dim;
    int squared;
    const double *dist;          // [nTgt], NULL = 0
    uint32_t blockSrc;           // sources per block
    uint32_t pack;               // 0: one pair per wave
    uint32_t fbCap;              // even, >= the longest target
    uint32_t ringRows;           // 64 or 128
    double *partKey;             // [blocks][nTgt]; NULL: no fold (matrix mode)
    double *partCost;            // [blocks][nTgt]
    uint32_t *partIdx;           // [blocks][nTgt]
    double *matrix;              // [nSrc][nTgt]; NULL: no matrix
};

template <int DIMR>
__global__ __launch_bounds__(64) void dtw_match_paced_kernel(const MatchPacedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double *bound1 = smem;                                          // [fbCap]   E of row c0 - 1
    double *bound2 = smem + a.fbCap;                                // [fbCap]   E of row c0 - 2
    double *ring = smem + 2 * (size_t)a.fbCap;                      // [ringRows][LD]
    const double INF = __builtin_inf();
    const int lane = threadIdx.x;
    const int dim = (int)a.dim;
    const uint32_t ringMask = a.ringRows - 1;
    const uint32_t s0 = blockIdx.y * a.blockSrc, s1 = min(a.nSrc, s0 + a.blockSrc);

    for (uint32_t t = blockIdx.x; t < a.nTgt; t += gridDim.x) {
        const int Fb = (int)(a.tgtOff[t + 1] - a.tgtOff[t]);
        const double *b0 = a.tgtRaw + a.tgtOff[t] * dim;
        const double delta = a.dist ? a.dist[t] : 0.0;
        // one source frame per target frame, steps of 0, 1 or 2 (Fb = 0: faMax < faMin, nothing fits)
        const int faMin = (Fb - 1) / 2 + 1, faMax = 2 * Fb - 1;
        // a target that fits the ring (64 frames, or 128 where the launch has a target of more than 64) enters it once and
        // stays for every pack and chunk of the block: column j sits in row j, nothing wraps
        const bool resident = Fb <= (int)a.ringRows;
        if (resident)
            for (int f0 = 0; f0 < Fb; f0 += 64)
                wave_refill<DIMR>(ring, ringMask, b0, dim, Fb, f0);

        double bestKey = INF, bestCost = INF;       // the first minimum among the pairs that ended in this lane
        uint32_t bestIdx = kNone;
        uint32_t s = s0;
        while (s < s1) {
            // the next pack: consecutive feasible sources side by side, or one long source alone
            int used = 0, rowsMax = 0;
            uint32_t myS = kNone, firstS = kNone;
            int myR = 0, myFa = 0;
            bool longSrc = false;
            while (s < s1) {
                const int Fa = (int)(a.srcOff[s + 1] - a.srcOff[s]);
                if (Fa < faMin || Fa > faMax) {           // no paced shape: +inf without touching a frame
                    if (a.matrix && lane == 0)
                        a.matrix[(size_t)s * a.nTgt + t] = INF;
                    ++s;
                    continue;
                }
                if (Fa > 64) {
                    if (used)
                        break;
                    longSrc = true;
                    myS = firstS = s;
                    myFa = rowsMax = Fa;
                    ++s;
                    break;
                }
                if (used && (!a.pack || used + Fa > 64))
                    break;
                if (lane >= used && lane < used + Fa) {
                    myS = s;
                    myR = lane - used;
                    myFa = Fa;
                }
                if (!used)
                    firstS = s;
                used += Fa;
                rowsMax = max(rowsMax, Fa);
                ++s;
            }
            if (firstS == kNone)
                break;                                     // nothing feasible was left

            // a lane without a row reads the pack's first frame, which exists
            const double *a0 = a.srcRaw + a.srcOff[myS != kNone ? myS : firstS] * dim;
            double result = INF;
            for (int c0 = 0; c0 < rowsMax; c0 += 64) {     // a pack is one chunk
                const int lr = longSrc ? lane : myR;       // the row inside the chunk: this lane works on column tau - lr
                const int r = c0 + lr;
                const bool rowValid = myS != kNone && r < myFa;
                const int rowsHere = min(64, rowsMax - c0);
                double ar[DIMR];
                wave_load_frame(ar, a0 + (size_t)(rowValid ? r : 0) * dim, dim);
                double mineN = INF, mineE = INF;                        // N(r, j-1), E(r, j-1)
                double d1 = INF, d2 = INF;                              // E(r-1, j-1), E(r-2, j-1)
                const int tauEnd = Fb - 1 + rowsHere;     // exclusive
                // (the refill's barrier also orders the hand-off rows between chunks; a resident ring has none, so:)
                if (resident)
                    __syncthreads();
                for (int tau = 0; tau < tauEnd; ++tau) {
                    if (!resident && (tau & 63) == 0)
                        wave_refill<DIMR>(ring, ringMask, b0, dim, Fb, tau);
                    const int j = tau - lr;
                    const double c = wave_cell_cost(ar, ring, ringMask, min(max(j, 0), Fb - 1), a.squared);
                    const double up = shfl_up1(mineE);        // E(r-1, j) for local rows >= 1: the next step's d1
                    if (lr == 0) {
                        d1 = d2 = INF;                        // above row 0 there is nothing: the lane before is another source's
                        if (c0 != 0 && j >= 1 && j < Fb) {
                            d1 = bound1[j - 1];
                            d2 = bound2[j - 1];
                        }
                    }
                    // E(r-2, j) for the next step: the d1 of lane l - 1 (+inf where that lane is a local row 0 of chunk 0)
                    const double nx = shfl_up1(d1);
                    const bool active = rowValid && j >= 0 && j < Fb;
                    if (active) {
                        double nD = r == 0 ? c : INF;         // column 0: the path starts at source frame 0, in state N
                        double eD = nD;
                        if (j > 0) {
                            double pD;                    // (a cost alone: nothing rides on the comparisons)
                            SSYM_PACED_PRED(pD, d1, d2, (void)0)
                            SSYM_PACED_STATES(nD, eD, c, pD, mineN, (void)0)
                        }
                        if (longSrc) {
                            if (lane == 63)
                                bound1[j] = eD;
                            if (lane == 62)
                                bound2[j] = eD;
                        }
                        if (r == myFa - 1 && j == Fb - 1)
                            result = eD;
                        mineN = nD;
                        mineE = eD;
                    }
                    d1 = up;
                    d2 = nx;
                }
            }
            // the lane of a source's last row holds its cost
            const bool holder = myS != kNone && (longSrc ? lane == ((myFa - 1) & 63) : myR == myFa - 1);
            if (holder) {
                if (a.matrix)
                    a.matrix[(size_t)myS * a.nTgt + t] = result;
                const double key = fabs(result - delta);
                if (key < bestKey) {                      // sources ascend within a lane: the first minimum; NaN never wins
                    bestKey = key;
                    bestCost = result;
                    bestIdx = myS;
                }
            }
        }
        if (a.partKey) {
            // the first minimum by (key, index) among the lanes; a lane without a candidate holds (+inf, 0xffffffff)
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double oK = __shfl_xor(bestKey, m), oC = __shfl_xor(bestCost, m);
                const uint32_t oI = (uint32_t)__shfl_xor((int)bestIdx, m);
                if (oK < bestKey || (oK == bestKey && oI < bestIdx)) {
                    bestKey = oK;
                    bestCost = oC;
                    bestIdx = oI;
                }
            }
            if (lane == 0) {
                const size_t o = (size_t)blockIdx.y * a.nTgt + t;
                a.partKey[o] = bestKey;
                a.partCost[o] = bestCost;
                a.partIdx[o] = bestIdx;
            }
        }
    }
}

// the first-minimum rule across blocks: blocks ascend in source index and each holds its lowest index among equal keys, so
// strict < keeps the lowest index (what ssym_merge_shards does among shards).  The fold starts at (0, +inf).
__global__ __launch_bounds__(128) void match_paced_fold_kernel(const double *__restrict__ partKey,
                                                               const double *__restrict__ partCost,
                                                               const uint32_t *__restrict__ partIdx, uint32_t nBlocks,
                                                               uint32_t nTgt, uint32_t indexBase,
                                                               uint32_t *__restrict__ outIdx, double *__restrict__ outCost)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nTgt)
        return;
    uint32_t minIdx = 0;
    double minKey = __builtin_inf(), cost = __builtin_inf();
    for (uint32_t b = 0; b < nBlocks; ++b) {
        const size_t o = (size_t)b * nTgt + t;
        const double k = partKey[o];
        if (k < minKey) {
            minKey = k;
            minIdx = partIdx[o];
            cost = partCost[o];
        }
    }
    outIdx[t] = minIdx + indexBase;
    if (outCost)
        outCost[t] = cost;
}

// what both calls refuse, before any device work
int32_t check_match_paced(ssym_ctx *ctx, const char *fn, const ssym_dict *dict, const ssym_queries *q)
{
    const std::string name(fn);
    if (ctx->metric != SSYM_METRIC_DTW) {
        ctx->err = name + ": the context's metric is refcos, which has no step pattern";
        return SSYM_E_UNSUPPORTED;
    }
    if (ctx->band >= 0) {
        ctx->err = name + ": the paced step pattern bounds the slope itself and takes no Sakoe-Chiba band; use a context without one";
        return SSYM_E_UNSUPPORTED;
    }
    int32_t rc = check_handles(ctx->err, fn, dict, q);
    if (rc != SSYM_OK)
        return rc;
    rc = check_sets(ctx->err, dict->set, q->set);
    if (rc != SSYM_OK) {
        ctx->err = name + ": " + ctx->err;
        return rc;
    }
    const SegmentSet &src = dict->set, &tgt = q->set;
    if (src.max_frames > (uint32_t)kMatchPacedMaxSrcFrames || tgt.max_frames > (uint32_t)kMatchPacedMaxTgtFrames ||
        src.dim > (uint32_t)kMatchPacedMaxDim) {
        ctx->err = name + ": a source has more than " + std::to_string(kMatchPacedMaxSrcFrames) + " frames, a target more than " +
                   std::to_string(kMatchPacedMaxTgtFrames) + ", or frames have more than " + std::to_string(kMatchPacedMaxDim) +
                   " values (the limits of ssym_dtw_align_step under SSYM_STEP_PACED)";
        return SSYM_E_UNSUPPORTED;
    }
    return SSYM_OK;
}

// sources per block and the grid.  The knobs (SSYM_TEST_HOOKS=1 only) are read at every launch.
void match_paced_geometry(const ssym_ctx *ctx, uint32_t N, uint32_t M, MatchPacedArgs &a, dim3 &grid)
{
    // enough waves to balance the device, blocks no shorter than kBlockMin and no longer than kBlockMax
    const uint64_t wantBlocks = std::max<uint64_t>(1, ((uint64_t)ctx->num_cus * kMatchPacedWavesPerCu + M - 1) / M);
    uint32_t blockSrc = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((N + wantBlocks - 1) / wantBlocks, kMatchPacedBlockMin),
                                                     kMatchPacedBlockMax);
    a.pack = 1;
    if (const char *k = ssym_knob("SSYM_PACED_MATCH_PACK"))
        a.pack = atoi(k) != 0;
    if (const char *k = ssym_knob("SSYM_PACED_MATCH_BLOCK"))
        blockSrc = (uint32_t)std::max(1, atoi(k));
    blockSrc = std::max(blockSrc, (N + kMatchPacedGridY - 1) / kMatchPacedGridY);
    a.blockSrc = blockSrc;
    grid = dim3(std::min(M, kMatchPacedGridX), (N + blockSrc - 1) / blockSrc);
}

int32_t launch_match_paced(ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, MatchPacedArgs &a, const dim3 &grid)
{
    const uint32_t fbCap = wave_fb_cap(tgt.max_frames), ringRows = wave_ring_rows(tgt.max_frames);
    const int dimr = wave_dimr(src.dim);
    a.srcRaw = src.raw;
    a.srcOff = src.off;
    a.nSrc = src.n;
    a.tgtRaw = tgt.raw;
    a.tgtOff = tgt.off;
    a.nTgt = tgt.n;
    a.dim = src.dim;
    a.squared = ctx->squared;
    a.fbCap = fbCap;
    a.ringRows = ringRows;
    const size_t lds = 2 * (size_t)fbCap * sizeof(double) + wave_ring_bytes(ringRows, dimr);
    void (*kern)(MatchPacedArgs) = SSYM_WAVE_KERNEL(dtw_match_paced_kernel, dimr);
    if (lds > 64 * 1024)
        SSYM_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<grid, 64, lds, ctx->stream>>>(a);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

}  // namespace

int32_t match_paced(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const double *distance, uint32_t index_base,
                    uint32_t *out_idx, double *out_cost, uint32_t flags, const char *fn)
{
    if (!ctx)
        return SSYM_E_INVALID;
    StageScope stageScope(ctx);
    int32_t rc = check_match_paced(ctx, fn, dict, q);
    if (rc != SSYM_OK)
        return rc;
    const SegmentSet &src = dict->set, &tgt = q->set;
    const uint32_t N = src.n, M = tgt.n;
    ssym_timings tm{};
    tm.n_pairs = (uint64_t)N * M;
    if (M == 0) {
        ctx->timings = tm;
        return SSYM_OK;
    }
    if (!out_idx) {
        ctx->err = std::string(fn) + ": out_idx is NULL";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    drop_pending(ctx);          // (the distances and the outputs land in scratch a begin .. finish would still need)
    hipStream_t st = ctx->stream;
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;

    MatchPacedArgs a{};
    dim3 grid;
    match_paced_geometry(ctx, N, M, a, grid);
    const size_t slots = (size_t)grid.y * M;
    rc = ensure(ctx, ctx->paced_part, slots * (2 * sizeof(double) + sizeof(uint32_t)));
    if (rc != SSYM_OK)
        return rc;
    a.partKey = (double *)ctx->paced_part.ptr;
    a.partCost = a.partKey + slots;
    a.partIdx = (uint32_t *)(a.partCost + slots);
    if (distance) {
        rc = ensure(ctx, ctx->dist, sizeof(double) * M);
        if (rc == SSYM_OK)
            rc = stage_h2d(ctx, ctx->dist.ptr, distance, sizeof(double) * M);
        if (rc != SSYM_OK)
            return rc;
        a.dist = (const double *)ctx->dist.ptr;
    }
    uint32_t *idxDev = out_idx;
    double *costDev = out_cost;
    if (!outDev) {
        rc = ensure(ctx, ctx->out_idx, sizeof(uint32_t) * M);
        if (rc == SSYM_OK)
            rc = ensure(ctx, ctx->out_cost, sizeof(double) * M);
        if (rc != SSYM_OK)
            return rc;
        idxDev = (uint32_t *)ctx->out_idx.ptr;
        costDev = out_cost ? (double *)ctx->out_cost.ptr : nullptr;
    }
    hipEvent_t *ev = ctx->ev;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    rc = launch_match_paced(ctx, src, tgt, a, grid);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    match_paced_fold_kernel<<<(M + 127) / 128, 128, 0, st>>>(a.partKey, a.partCost, a.partIdx, grid.y, M, index_base, idxDev,
                                                            costDev);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    if (!outDev) {
        rc = request_outputs(ctx, out_idx, idxDev, out_cost, costDev, M, 1);
        if (rc != SSYM_OK)
            return rc;
    }
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    stage_finish(ctx);
    tm.main_ms = ev_ms(ev[0], ev[1]);
    tm.reduce_ms = ev_ms(ev[1], ev[2]);
    tm.total_ms = ev_ms(ev[0], ev[2]);
    ctx->timings = tm;
    return SSYM_OK;
}

int32_t pair_matrix_paced(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double *out_matrix, const char *fn)
{
    if (!ctx)
        return SSYM_E_INVALID;
    int32_t rc = check_match_paced(ctx, fn, dict, q);
    if (rc != SSYM_OK)
        return rc;
    if (!out_matrix) {
        ctx->err = std::string(fn) + ": out_matrix is NULL";
        return SSYM_E_INVALID;
    }
    const SegmentSet &src = dict->set, &tgt = q->set;
    const uint32_t N = src.n, M = tgt.n;
    ssym_timings tm{};
    tm.n_pairs = (uint64_t)N * M;
    if (M == 0) {
        ctx->timings = tm;
        return SSYM_OK;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    drop_pending(ctx);          // (the matrix lands in the scratch a begin .. finish would still need)
    hipStream_t st = ctx->stream;
    rc = ensure(ctx, ctx->part, sizeof(double) * (size_t)N * M);
    if (rc != SSYM_OK)
        return rc;
    MatchPacedArgs a{};
    dim3 grid;
    match_paced_geometry(ctx, N, M, a, grid);
    a.matrix = (double *)ctx->part.ptr;
    hipEvent_t *ev = ctx->ev;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    rc = launch_match_paced(ctx, src, tgt, a, grid);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_matrix, a.matrix, sizeof(double) * (size_t)N * M, hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    tm.main_ms = tm.total_ms = ev_ms(ev[0], ev[1]);
    ctx->timings = tm;
    return SSYM_OK;
}

}  // namespace ssym
