// dtw_cover.hip -- the cover: the sequence of dictionary segments, with the target's cut points, whose paced alignment costs
// sum to the least total over every tiling of the target (DESIGN.md 2 "Cover", 5.23).
//
// Role on the path: match -> align -> warp starts from a target that is cut already, and the cut never saw the dictionary.
// Under the paced pattern every path has one cell per target frame, so every tiling of a T-frame target has T cells and
// the totals of different tilings compare.  The cover chooses boundaries and matches together; every piece goes straight
// into ssym_dtw_align_step(SSYM_STEP_PACED) and the warp calls.
//
// Definition.  c, the squared option and the arithmetic are those of "Paced alignment" (dtw_align.hip), word for word: f64,
// k ascending, every sub, mul, add and sqrt rounded separately, no contraction.  For one target X of T frames and sources
// n = 0 ... N-1 of Fa[n] frames:
//   w(n,s,L) = the cost of "Paced matching" for (source n, target X[s ... s+L-1]): +inf where the shape rule says no (Fa = 0,
//              or Fa outside floor((L-1)/2) + 1 ... 2 L - 1, decided before the recurrence), else E(Fa-1, L-1) -- a source of
//              Fa frames covers windows of ceil((Fa+1)/2) ... 2 Fa frames only
//   M(s,L)   = the first least w(n,s,L) over n ascending from (none, +inf), strict <  (NaN and +inf never win) -> src(s,L)
//   best(-1) = 0
//   best(e)  = scan L = 1 ... min(e+1, 2 Fmax) ascending from (none, +inf), strict <, over the L that have a src(e-L+1, L):
//              v = (M(e-L+1, L) + piece_penalty) + best(e-L)  -> the first least v, its (L, src, M)
//   cover    : walk back from e = T-1 while best is finite: piece (src, start = e-L+1, end = e, cost = M); e <- e-L
//   total    = best(T-1);  count = pieces;  pieces reported in ascending start
//   no cover : T = 0, or best(T-1) not finite -> count 0, total +inf
// Cover with gaps (ssym_dtw_cover_gaps) adds one candidate to each step: vg = gap_cost + best(e-1); if vg < v (strict, so a
// piece keeps a tie) best(e) = vg with the back-pointer (L = 1, SSYM_COVER_GAP, M = gap_cost).  The walk reports a gap frame
// as the piece (SSYM_COVER_GAP, e, e, gap_cost); piece_penalty is not charged on it.  gap_cost = +inf never wins: that is
// ssym_dtw_cover.  With a finite gap_cost every best(e) is finite, so every target of at least one frame has a cover.
//
// Mapping.  A column of the paced recurrence depends on the column before it alone, so ONE forward pass per (n, s) over the
// longest window, 2 Fa columns, yields w(n,s,L) for every L: after column L-1 the bottom row holds it.  And the local
// distance c(i, t) of source frame i and target frame t is shared by every start s = t - j.
//   forward   cover_forward_kernel.  A workgroup takes S consecutive starts of one target (one start per lane, S = 64
//             unless the source rows ask for fewer) and a block of consecutive sources.  Per source, strips of JC columns:
//             the c tile [Fa][S + JC - 1] of the strip is computed once into LDS by all lanes, then every lane runs its
//             columns.  A lane's E and N columns sit in LDS ([row][lane]: consecutive lanes, consecutive doubles) and are
//             updated in place with the row descending, so E(i-1, j-1) and E(i-2, j-1) are still the old column's when row
//             i reads them: a cell costs one c read, one E read, one N read and two writes, nothing crosses lanes.  The
//             whole matrix is computed, cells the start cannot reach included: a NaN there can stand in a comparison of
//             a cell that counts.  After column L-1, if the shape rule admits (Fa, L), the lane folds E(Fa-1, L-1) into
//             its own entry (L, s) of the block's table under strict <: sources ascend, so the first minimum stays.
//   fold      cover_fold_kernel folds the blocks' tables in block order under strict <, as match_paced_fold_kernel does,
//             into block 0's.  The result depends neither on the grid nor on S, JC or the block size.
//   chain     cover_chain_kernel: one wave per target, sequentially over e.  best lives in an LDS ring; the <= 2 Fmax
//             candidates of a step are spread over the lanes (L ascending within a lane, strict <) and reduced by (v, L).
//             Lane 0 then walks the back-pointers twice (count, then fill in ascending start) with plain stores.
// No kernel waits on another workgroup: stream order is the only ordering between the three.
// The coverer (dtw_coverer.hip, "Live cover") launches the forward pass and its fold through cover_forward below, on a buffer
// of its own, and runs the chain's step (dtw_cover_chain.hpp) in a resumable kernel: one body each for both callers.
#include "dtw_wave.hpp"
#include "dtw_cover_chain.hpp"

#include <algorithm>
#include <cmath>

namespace ssym {

// Limits of the cover (soundsym_amd.h)
constexpr uint32_t kCoverMaxSourceFrames = 128;
constexpr uint32_t kCoverMaxDim = 64;
// scratch: blocks x frames x 2 Fmax x 12 bytes (the M / src tables) + frames x 16 bytes (back-pointers)
constexpr uint64_t kCoverScratchBytes = 512ull << 20;
constexpr uint32_t kCoverMaxStarts = 128;                 // starts per workgroup: one lane each, two waves at most
constexpr size_t kCoverLdsBytes = 160 * 1024;             // what one workgroup may take of a CU
constexpr size_t kCoverLdsShared = 80 * 1024;             // ... and what leaves room for a second workgroup
constexpr uint32_t kCoverWorkgroupsPerCu = 4;             // source blocks are sized to leave this many workgroups per CU
constexpr uint32_t kCoverBlockMin = 8;
constexpr uint32_t kCoverRing = 512;                      // > 2 kCoverMaxSourceFrames, a power of two
constexpr uint32_t kCoverGridY = 65535, kCoverGridZ = 65535;

namespace {

constexpr uint32_t kNone = kCoverNone;

__device__ __forceinline__ uint64_t min64(uint64_t x, uint64_t y) { return x < y ? x : y; }

struct CoverArgs {
    const double *srcRaw;
    const uint64_t *srcOff;
    uint32_t nSrc;
    const double *tgtRaw;
    const uint64_t *tgtOff;
    uint32_t nTgt;
    uint32_t dim;
    int squared;
    uint32_t blockSrc;           // sources per block
    uint32_t starts;             // S: starts per workgroup, <= blockDim.x
    uint32_t strip;              // JC: columns per c tile
    uint32_t width;              // 2 Fmax: the L a table row holds
    uint64_t frames;             // target frames of the whole query set
    double *tabM;                // [blocks][width][frames]
    uint32_t *tabSrc;            // [blocks][width][frames]
};

__global__ __launch_bounds__(kCoverMaxStarts) void cover_forward_kernel(const CoverArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const double INF = __builtin_inf();
    const uint32_t S = a.starts, W = S + a.strip;
    const uint32_t tid = threadIdx.x;
    const uint32_t dim = a.dim;
    const uint32_t n0 = blockIdx.y * a.blockSrc, n1 = min(a.nSrc, n0 + a.blockSrc);
    double *tabM = a.tabM + (size_t)blockIdx.y * a.width * a.frames;
    uint32_t *tabSrc = a.tabSrc + (size_t)blockIdx.y * a.width * a.frames;

    for (uint32_t t = blockIdx.z; t < a.nTgt; t += gridDim.z) {
        const uint64_t g0 = a.tgtOff[t];
        const uint64_t T = a.tgtOff[t + 1] - g0;
        const uint64_t s0 = (uint64_t)blockIdx.x * S;
        if (s0 >= T)
            continue;
        const uint64_t s = s0 + tid;
        const bool lane = tid < S && s < T;
        const double *b0 = a.tgtRaw + g0 * dim;
        if (lane)
            for (uint32_t L = 0; L < a.width; ++L) {
                tabM[(size_t)L * a.frames + g0 + s] = INF;
                tabSrc[(size_t)L * a.frames + g0 + s] = kNone;
            }
        for (uint32_t n = n0; n < n1; ++n) {
            const uint32_t Fa = (uint32_t)(a.srcOff[n + 1] - a.srcOff[n]);
            const uint32_t lMin = Fa / 2 + 1;                            // ceil((Fa + 1) / 2): the shortest window Fa covers
            if (Fa == 0 || T - s0 < lMin)
                continue;                                                // (the tile's first start has the most room)
            const double *a0 = a.srcRaw + a.srcOff[n] * dim;
            double *E = smem, *N = smem + (size_t)Fa * S, *C = smem + 2 * (size_t)Fa * S;
            const uint32_t colsAll = (uint32_t)min64((uint64_t)2 * Fa, T - s0);
            const uint32_t cols = lane ? (uint32_t)min64((uint64_t)2 * Fa, T - s) : 0;
            for (uint32_t j0 = 0; j0 < colsAll; j0 += a.strip) {
                const uint32_t jc = min(a.strip, colsAll - j0);
                // the strip's c tile: target frames s0 + j0 + x, x < S + jc - 1, as far as the target goes
                const uint32_t nx = (uint32_t)min64((uint64_t)(S + jc - 1), T - s0 - j0);
                __syncthreads();                                         // the strip before is read
                for (uint32_t idx = tid; idx < Fa * nx; idx += blockDim.x) {
                    const uint32_t i = idx / nx, x = idx - i * nx;
                    const double *ar = a0 + (size_t)i * dim, *br = b0 + (s0 + j0 + x) * dim;
                    double acc = 0.0;
                    for (uint32_t k = 0; k < dim; ++k) {
                        const double df = __dsub_rn(ar[k], br[k]);
                        acc = __dadd_rn(acc, __dmul_rn(df, df));
                    }
                    C[(size_t)i * W + x] = a.squared ? acc : sqrt(acc);
                }
                __syncthreads();
                for (uint32_t jj = 0; jj < jc; ++jj) {
                    const uint32_t j = j0 + jj;
                    if (j >= cols)
                        break;
                    double bottom;
                    if (j == 0) {
                        // column 0: the path starts at source frame 0, in state N
                        bottom = INF;
                        for (uint32_t i = 0; i < Fa; ++i) {
                            const double v = i == 0 ? C[tid] : INF;
                            N[(size_t)i * S + tid] = v;
                            E[(size_t)i * S + tid] = v;
                            bottom = v;
                        }
                    } else {
                        double e1 = Fa >= 2 ? E[(size_t)(Fa - 2) * S + tid] : INF;          // E(i-1, j-1)
                        bottom = INF;
                        for (uint32_t i = Fa; i-- > 0;) {
                            const double e2 = i >= 2 ? E[(size_t)(i - 2) * S + tid] : INF;  // E(i-2, j-1)
                            const double c = C[(size_t)i * W + tid + jj];
                            double pD, nD, eD;            // (a cost alone: nothing rides on the comparisons)
                            SSYM_PACED_PRED(pD, e1, e2, (void)0)
                            SSYM_PACED_STATES(nD, eD, c, pD, N[(size_t)i * S + tid], (void)0)
                            N[(size_t)i * S + tid] = nD;
                            E[(size_t)i * S + tid] = eD;
                            if (i == Fa - 1)
                                bottom = eD;
                            e1 = e2;
                        }
                    }
                    // the window of j + 1 frames ends here: Fa <= 2 (j + 1) - 1 holds from lMin on, j + 1 <= 2 Fa always
                    if (j + 1 >= lMin) {
                        const size_t o = (size_t)j * a.frames + g0 + s;
                        if (bottom < tabM[o]) {          // sources ascend: the first minimum stays; NaN and +inf never win
                            tabM[o] = bottom;
                            tabSrc[o] = n;
                        }
                    }
                }
            }
            __syncthreads();                              // E, N and C move with the next source's Fa
        }
    }
}

// the first-minimum rule across blocks, into block 0's table: blocks ascend in source index and each holds its lowest index
// among equal costs, so strict < keeps the lowest index
__global__ __launch_bounds__(256) void cover_fold_kernel(double *__restrict__ tabM, uint32_t *__restrict__ tabSrc,
                                                         uint32_t nBlocks, uint64_t entries)
{
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= entries)
        return;
    double best = __builtin_inf();
    uint32_t src = kNone;
    for (uint32_t b = 0; b < nBlocks; ++b) {
        const double v = tabM[(size_t)b * entries + o];
        if (v < best) {
            best = v;
            src = tabSrc[(size_t)b * entries + o];
        }
    }
    tabM[o] = best;
    tabSrc[o] = src;
}

struct ChainArgs {
    const double *tabM;          // [width][frames]
    const uint32_t *tabSrc;
    const uint64_t *tgtOff;
    uint32_t nTgt;
    uint32_t width;
    uint64_t frames;
    double penalty;
    double gapCost;              // the price of a frame left uncovered; +inf: the plain cover
    uint32_t *bpLen, *bpSrc;     // [frames] back-pointers: the last piece of the best cover of X[0 ... e]
    double *bpCost;              // [frames]
    uint32_t *outCount;          // [nTgt]
    double *outTotal;            // [nTgt]
    uint32_t *outSrc, *outStart, *outEnd;   // [frames]
    double *outCost;             // [frames]
};

__global__ __launch_bounds__(64) void cover_chain_kernel(const ChainArgs a)
{
    __shared__ double ring[kCoverRing];                  // best(e) at (e + 1) mod kCoverRing
    const double INF = __builtin_inf();
    const uint32_t lane = threadIdx.x;
    for (uint32_t t = blockIdx.x; t < a.nTgt; t += gridDim.x) {
        const uint64_t g0 = a.tgtOff[t];
        const uint64_t T = a.tgtOff[t + 1] - g0;
        for (uint64_t f = lane; f < T; f += 64) {
            a.outSrc[g0 + f] = kNone;
            a.outStart[g0 + f] = kNone;
            a.outEnd[g0 + f] = kNone;
            a.outCost[g0 + f] = INF;
        }
        if (lane == 0)
            ring[0] = 0.0;                               // best(-1)
        __syncthreads();
        double last = INF;                               // best(T-1); T = 0: no cover
        for (uint64_t e = 0; e < T; ++e) {
            const uint32_t lMax = (uint32_t)min64((uint64_t)a.width, e + 1);
            const CoverPick pick = cover_chain_step(a.tabM, a.tabSrc, a.frames, g0 + e, lMax, a.penalty, a.gapCost, ring, kCoverRing - 1,
                                                    e, lane);
            const double bestV = pick.v, bestM = pick.m;
            const uint32_t bestL = pick.len, bestS = pick.src;
            if (lane == 0) {
                ring[(e + 1) & (kCoverRing - 1)] = bestV;
                a.bpLen[g0 + e] = bestL;
                a.bpSrc[g0 + e] = bestS;
                a.bpCost[g0 + e] = bestM;
            }
            last = bestV;
            __syncthreads();
        }
        if (lane == 0) {
            uint32_t count = 0;
            if (last < INF) {
                // a finite best(e) has a last piece (a gap frame is a piece of one frame), and what lies before it has a
                // finite best as well
                for (int64_t e = (int64_t)T - 1; e >= 0; e -= a.bpLen[g0 + e])
                    ++count;
                uint32_t k = count;
                for (int64_t e = (int64_t)T - 1; e >= 0;) {
                    const uint32_t L = a.bpLen[g0 + e];
                    --k;
                    a.outSrc[g0 + k] = a.bpSrc[g0 + e];
                    a.outStart[g0 + k] = (uint32_t)(e + 1 - L);
                    a.outEnd[g0 + k] = (uint32_t)e;
                    a.outCost[g0 + k] = a.bpCost[g0 + e];
                    e -= L;
                }
            }
            a.outCount[t] = count;
            a.outTotal[t] = count ? last : INF;
        }
        __syncthreads();                                 // the ring starts over with the next target
    }
}

}  // namespace

CoverLimits cover_limits()
{
    return CoverLimits{kCoverMaxSourceFrames, kCoverMaxDim, kCoverRing, kCoverScratchBytes};
}

// what the call refuses of a context, every message once
int32_t check_cover_ctx(ssym_ctx *ctx, const char *fn)
{
    if (ctx->metric != SSYM_METRIC_DTW) {
        ctx->err = std::string(fn) + ": the context's metric is refcos, which has no alignment to cover with";
        return SSYM_E_UNSUPPORTED;
    }
    if (ctx->band >= 0) {
        ctx->err = std::string(fn) + ": the paced step pattern bounds the slope itself and takes no Sakoe-Chiba band; use a context without one";
        return SSYM_E_UNSUPPORTED;
    }
    return SSYM_OK;
}

// ... of the prices: per piece, and per frame left uncovered
int32_t check_cover_prices(ssym_ctx *ctx, const char *fn, double piece_penalty, double gap_cost)
{
    if (!(piece_penalty >= 0.0) || std::isinf(piece_penalty)) {
        ctx->err = std::string(fn) + ": piece_penalty must be finite and not negative";
        return SSYM_E_INVALID;
    }
    if (!(gap_cost >= 0.0)) {
        ctx->err = std::string(fn) + ": gap_cost must not be negative or NaN (+inf: no gaps)";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

// ... and of a dictionary
int32_t check_cover_dict(ssym_ctx *ctx, const char *fn, const SegmentSet &src)
{
    if (src.max_frames > kCoverMaxSourceFrames || src.dim > kCoverMaxDim) {
        ctx->err = std::string(fn) + ": a dictionary segment has more than " + std::to_string(kCoverMaxSourceFrames) +
                   " frames, or frames have more than " + std::to_string(kCoverMaxDim) + " values";
        return SSYM_E_UNSUPPORTED;
    }
    return SSYM_OK;
}

namespace {

// starts per workgroup, columns per strip and LDS of a launch whose longest source has fmax frames: E and N [fmax][S]
// and the c tile [fmax][S + JC].  64 starts where they fit with a strip of at least 8 columns, halved until they do;
// the strip as long as leaves room for a second workgroup on the CU, else as long as fits.
struct CoverShape {
    uint32_t starts, strip;
    size_t lds;
};
CoverShape cover_shape(uint32_t fmax, uint32_t startsKnob, uint32_t stripKnob)
{
    const uint32_t rows = std::max(fmax, 1u);
    const size_t perCol = (size_t)rows * sizeof(double);
    uint32_t S = startsKnob ? std::min(startsKnob, kCoverMaxStarts) : 64;
    while (S > 1 && perCol * (3 * (size_t)S + 8) > kCoverLdsBytes)
        S /= 2;
    auto fit = [&](size_t budget) -> uint32_t {
        const size_t colsFit = budget / perCol;
        return colsFit > 3 * (size_t)S ? (uint32_t)std::min<size_t>(colsFit - 3 * (size_t)S, 2 * rows) : 0;
    };
    uint32_t JC = fit(kCoverLdsShared);
    if (JC < std::min(16u, 2 * rows))
        JC = fit(kCoverLdsBytes);
    if (stripKnob)
        JC = std::min(std::max(stripKnob, 1u), fit(kCoverLdsBytes));
    return CoverShape{S, JC, perCol * (3 * (size_t)S + JC)};
}

}  // namespace

// The forward pass and its fold for nTgt targets (tgtRaw, tgtOff: DEVICE; hTgtOff: the same offsets on the HOST), enqueued
// on the context's stream: the launch geometry of ssym_dtw_cover and of the coverer.  The tables of the source blocks go
// into ctx->cover_tab, block 0's holding the folded result afterwards, with room for extraF64 doubles and extraU32 words
// (the caller's back-pointers) in the same buffer.  The caller has checked that one block's tables and the extra room fit
// kCoverScratchBytes.
int32_t cover_forward(ssym_ctx *ctx, const SegmentSet &src, const double *tgtRaw, const uint64_t *tgtOff, const uint64_t *hTgtOff,
                      uint32_t nTgt, uint64_t extraF64, uint64_t extraU32, CoverTables *out)
{
    const uint32_t N = src.n, M = nTgt;
    const uint64_t F = hTgtOff[M] - hTgtOff[0];
    const uint32_t width = 2 * std::max(src.max_frames, 1u);
    const uint64_t tableBytes = F * width * (sizeof(double) + sizeof(uint32_t));      // one block's M and src
    const uint64_t backBytes = extraF64 * sizeof(double) + extraU32 * sizeof(uint32_t);
    hipStream_t st = ctx->stream;
    uint64_t maxFrames = 0;
    for (uint32_t t = 0; t < M; ++t)
        maxFrames = std::max(maxFrames, hTgtOff[t + 1] - hTgtOff[t]);

    // geometry.  The knobs (SSYM_TEST_HOOKS=1 only) are read at every launch; none changes a result.
    uint32_t startsKnob = 0, stripKnob = 0, blockKnob = 0;
    if (const char *k = ssym_knob("SSYM_COVER_STARTS"))
        startsKnob = (uint32_t)std::max(1, atoi(k));
    if (const char *k = ssym_knob("SSYM_COVER_STRIP"))
        stripKnob = (uint32_t)std::max(1, atoi(k));
    if (const char *k = ssym_knob("SSYM_COVER_BLOCK"))
        blockKnob = (uint32_t)std::max(1, atoi(k));
    const CoverShape shape = cover_shape(src.max_frames, startsKnob, stripKnob);
    const uint64_t tiles = (maxFrames + shape.starts - 1) / shape.starts;
    uint64_t tilesAll = 0;
    for (uint32_t t = 0; t < M; ++t)
        tilesAll += (hTgtOff[t + 1] - hTgtOff[t] + shape.starts - 1) / shape.starts;
    // source blocks: enough workgroups to balance the device, as many tables as the scratch holds
    const uint64_t wantBlocks = std::max<uint64_t>(1, ((uint64_t)ctx->num_cus * kCoverWorkgroupsPerCu + tilesAll) / (tilesAll + 1));
    const uint64_t roomBlocks = tableBytes ? std::max<uint64_t>(1, (kCoverScratchBytes - backBytes) / tableBytes) : 1;
    uint64_t nBlocks = std::min<uint64_t>({wantBlocks, roomBlocks, (uint64_t)kCoverGridY, (uint64_t)(N + kCoverBlockMin - 1) / kCoverBlockMin});
    uint32_t blockSrc = (uint32_t)((N + nBlocks - 1) / std::max<uint64_t>(nBlocks, 1));
    if (blockKnob)
        blockSrc = std::max<uint32_t>(blockKnob, (uint32_t)((N + std::min<uint64_t>(roomBlocks, kCoverGridY) - 1) /
                                                            std::min<uint64_t>(roomBlocks, kCoverGridY)));
    nBlocks = (N + blockSrc - 1) / blockSrc;

    const int32_t rc = ensure(ctx, ctx->cover_tab, (size_t)(nBlocks * tableBytes + backBytes) + 64);
    if (rc != SSYM_OK)
        return rc;
    const uint64_t entries = F * width;
    double *tabM = (double *)ctx->cover_tab.ptr;
    double *moreF64 = tabM + nBlocks * entries;
    uint32_t *tabSrc = (uint32_t *)(moreF64 + extraF64);
    *out = CoverTables{tabM, tabSrc, moreF64, tabSrc + nBlocks * entries, width};
    if (F) {
        CoverArgs a{};
        a.srcRaw = src.raw;
        a.srcOff = src.off;
        a.nSrc = N;
        a.tgtRaw = tgtRaw;
        a.tgtOff = tgtOff;
        a.nTgt = M;
        a.dim = src.dim;
        a.squared = ctx->squared;
        a.blockSrc = blockSrc;
        a.starts = shape.starts;
        a.strip = shape.strip;
        a.width = width;
        a.frames = F;
        a.tabM = tabM;
        a.tabSrc = tabSrc;
        if (shape.lds > 64 * 1024)
            SSYM_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)cover_forward_kernel,
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds));
        const dim3 grid((unsigned)tiles, (unsigned)nBlocks, std::min(M, kCoverGridZ));
        const unsigned threads = (shape.starts + 63) / 64 * 64;
        cover_forward_kernel<<<grid, threads, shape.lds, st>>>(a);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        if (nBlocks > 1) {
            cover_fold_kernel<<<(unsigned)((entries + 255) / 256), 256, 0, st>>>(tabM, tabSrc, (uint32_t)nBlocks, entries);
            SSYM_HIP_CHECK(ctx, hipGetLastError());
        }
    }
    return SSYM_OK;
}

namespace {

// ssym_dtw_cover (gap_cost = +inf) and ssym_dtw_cover_gaps: one body, the chain's gap candidate is the only difference
int32_t dtw_cover(ssym_ctx *ctx, const char *fn, const ssym_dict *dict, const ssym_queries *q, double piece_penalty, double gap_cost,
                  uint32_t flags, uint32_t *out_count, double *out_total, uint32_t *out_src, uint32_t *out_start,
                  uint32_t *out_end, double *out_cost)
{
    if (!ctx)
        return SSYM_E_INVALID;
    int32_t rc = check_cover_ctx(ctx, fn);
    if (rc != SSYM_OK)
        return rc;
    rc = check_handles(ctx->err, fn, dict, q);
    if (rc != SSYM_OK)
        return rc;
    rc = check_cover_prices(ctx, fn, piece_penalty, gap_cost);
    if (rc != SSYM_OK)
        return rc;
    const SegmentSet &src = dict->set, &tgt = q->set;
    const uint32_t N = src.n, M = tgt.n;
    const uint64_t F = tgt.total_frames;
    ssym_timings tm{};
    tm.n_pairs = (uint64_t)N * F;
    if (M == 0) {
        ctx->timings = tm;
        return SSYM_OK;
    }
    rc = check_sets(ctx->err, src, tgt);
    if (rc != SSYM_OK) {
        ctx->err = std::string(fn) + ": " + ctx->err;
        return rc;
    }
    if (!out_count || !out_total || (F && (!out_src || !out_start || !out_end || !out_cost))) {
        ctx->err = std::string(fn) + ": out_count, out_total, out_src, out_start, out_end and out_cost must not be NULL";
        return SSYM_E_INVALID;
    }
    rc = check_cover_dict(ctx, fn, src);
    if (rc != SSYM_OK)
        return rc;
    const uint32_t width = 2 * std::max(src.max_frames, 1u);
    const uint64_t tableBytes = F * width * (sizeof(double) + sizeof(uint32_t));      // one block's M and src
    const uint64_t backBytes = F * (sizeof(double) + 2 * sizeof(uint32_t));
    if (F > 0xffffffffull || tableBytes + backBytes > kCoverScratchBytes) {
        ctx->err = std::string(fn) + ": the tables need frames x 2 Fmax x 12 + frames x 16 bytes, more than " +
                   std::to_string(kCoverScratchBytes >> 20) + " MiB of scratch; cover fewer target frames per call";
        return SSYM_E_UNSUPPORTED;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    Blocks bl(ctx);
    // outputs: the caller's device arrays in place, or one f64 and one u32 block copied back after the chain
    StagedOut out(flags, {{out_total, M}, {out_cost, F}}, {{out_count, M}, {out_src, F}, {out_start, F}, {out_end, F}});
    rc = out.alloc(bl);
    if (rc != SSYM_OK)
        return rc;
    ChainArgs c{};
    c.outTotal = out.f64[0];
    c.outCost = out.f64[1];
    c.outCount = out.u32[0];
    c.outSrc = out.u32[1];
    c.outStart = out.u32[2];
    c.outEnd = out.u32[3];

    hipEvent_t *ev = ctx->ev;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    CoverTables tab{};
    rc = cover_forward(ctx, src, tgt.raw, tgt.off, tgt.h_off.data(), M, F, 2 * F, &tab);       // + the back-pointers
    if (rc != SSYM_OK)
        return rc;
    double *tabM = tab.tabM, *bpCost = tab.moreF64;
    uint32_t *tabSrc = tab.tabSrc, *bpLen = tab.moreU32, *bpSrc = bpLen + F;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    c.tabM = tabM;
    c.tabSrc = tabSrc;
    c.tgtOff = tgt.off;
    c.nTgt = M;
    c.width = width;
    c.frames = F;
    c.penalty = piece_penalty;
    c.gapCost = gap_cost;
    c.bpLen = bpLen;
    c.bpSrc = bpSrc;
    c.bpCost = bpCost;
    cover_chain_kernel<<<std::min<unsigned>(M, (unsigned)ctx->num_cus * 8), 64, 0, st>>>(c);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    rc = out.finish(ctx);
    if (rc != SSYM_OK)
        return rc;
    tm.main_ms = ev_ms(ev[0], ev[1]);
    tm.reduce_ms = ev_ms(ev[1], ev[2]);
    tm.total_ms = ev_ms(ev[0], ev[2]);
    tm.main_launches = 1;
    ctx->timings = tm;
    return SSYM_OK;
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_dtw_cover(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double piece_penalty, uint32_t flags,
                       uint32_t *out_count, double *out_total, uint32_t *out_src, uint32_t *out_start, uint32_t *out_end,
                       double *out_cost)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_cover(ctx, "ssym_dtw_cover", dict, q, piece_penalty, __builtin_inf(), flags, out_count, out_total, out_src,
                         out_start, out_end, out_cost);
    });
}

int32_t ssym_dtw_cover_gaps(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double piece_penalty, double gap_cost,
                            uint32_t flags, uint32_t *out_count, double *out_total, uint32_t *out_src, uint32_t *out_start,
                            uint32_t *out_end, double *out_cost)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_cover(ctx, "ssym_dtw_cover_gaps", dict, q, piece_penalty, gap_cost, flags, out_count, out_total, out_src,
                         out_start, out_end, out_cost);
    });
}
}
