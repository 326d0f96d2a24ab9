// dtw_mosaic.hip -- the mosaic: an uncut target tiled by pieces, each piece any span of any dictionary segment aligned under
// the paced pattern; the cuts, the segments, the spans and the paths are chosen together in one pass (DESIGN.md 2 "Mosaic",
// 5.25).
//
// Role on the path: spotting frees the dictionary's cut, the cover frees the target's; the mosaic frees both.  Under the
// paced pattern every tiling of a T-frame target has T cells, so the totals of different tilings compare.  Every piece
// goes straight into the warp calls with windows (ssym_reconstruct_warped_spans / _wsola_spans).
//
// Definition.  c, the squared option and the arithmetic are those of "Paced spotting" (dtw_spot.hip), word for word: f64, k
// ascending, every sub, mul, add and sqrt rounded separately, no contraction.  The dictionary's segments are laid end to
// end: g = 0 ... G-1 is a global source frame, seg(g) its segment and pos(g) its frame within it; empty segments contribute
// nothing.  Every cell has the states N and H of the paced pattern.  For one target X of T frames:
//   best(-1) = 0
//   column j = 0 ... T-1:
//     S      = piece_penalty + best(j-1)                              (the price of opening a piece at column j)
//     P(g)   = E(g-1, j-1) if pos(g) >= 1, else +inf
//              if pos(g) >= 2 and E(g-2, j-1) < P: E(g-2, j-1)         (strict <; j = 0: P = +inf)
//     open(g)= not (P(g) <= S)                                        (a tie continues the piece; a NaN P opens)
//     Q      = S if open(g) else P(g)
//     H(g,j) = c(g,j) + N(g,j-1)                                      (+inf at j = 0)
//     N(g,j) = c(g,j) + Q
//     E(g,j) = N(g,j); if H(g,j) < N(g,j): H(g,j)                     (strict <: a tie keeps N)
//     (v,arg)= the first least E(g,j) over g ascending from (+inf, none), strict <   (NaN and +inf never win)
//     vg     = gap_cost + best(j-1);  if vg < v (strict): best(j) = vg, arg(j) = GAP;  else best(j) = v, arg(j) = arg
//   total    = best(T-1);  no mosaic: T = 0, or total not finite -> count 0, total +inf
//   backward : j = T-1, at arg(j).  GAP: frame j is a gap frame, go to arg(j-1).  Otherwise the state is H if H < N there,
//              else N.  State H at (g,j): the cell before is (g, j-1) in state N.  State N at (g,j): if open(g) at column
//              j, a piece starts here, go to arg(j-1); else the cell before is (g-2, j-1) if the P rule took it, else
//              (g-1, j-1), in its E state.
//
// Mapping.  Column j needs the least value of ALL of column j-1, over every source frame, so each column ends in a
// reduction over the whole dictionary: the row wavefront of dtw_wave.hpp cannot express that.
//   forward   mosaic_forward_kernel, one workgroup per target, the column loop inside; the body of a column is
//             mosaic_column (dtw_mosaic_common.hpp), which the live mosaic's forward kernel runs as well -- the kernel keeps
//             column -1, the first frame and the total.  The source frames are spread over the threads (g = thread,
//             thread + blockDim, ...).  E and N of column j-1 sit in a ping-pong slab of global
//             scratch per workgroup (4 G doubles, L2-resident at these sizes; one code path for every G); column -1 is a
//             slab of +inf, which makes column 0 the general column.  A thread forms c(g,j) in the oracle's order from
//             its source frame in global memory and the target frame in a two-row LDS ring (mosaic_cost: dtw_wave.hpp's
//             wave_load_frame / wave_cell_cost keep ONE source frame in registers over many columns; here a thread has
//             many frames per column, and reloading the register frame per cell cost 129 spilled SGPRs and 52 spilled
//             VGPRs at 64 values per frame -- DESIGN.md 5.25).  The source frames are read from a TRANSPOSED copy
//             [dim][G] made once per call, so the 64 lanes of a load read 512 consecutive bytes and not 64 rows (a
//             quarter less time on the many-target shape, LAB.md).  The thread reads E(g-1), E(g-2) and N(g) of the old column, writes the new pair and ONE direction byte (bit 0: H < N; bits 1-2: 0 diagonal, 1 skip,
//             2 open), and keeps its first-least (value, g).  The waves reduce those by (value, g) with shuffles, write one
//             pair each to LDS, and after the column's ONE __syncthreads() every thread folds the <= 16 pairs and applies
//             the gap candidate itself: best(j) and the next S are in every thread's registers, thread 0 stores arg(j).
//             The same barrier orders the slab, the ring row and the pairs (both double-buffered by the column's parity).
//   backward  mosaic_backtrace_kernel, one workgroup per target on the forward launch's grid: thread 0 walks the bytes
//             back from arg(T-1) (mosaic_walk, dtw_mosaic_common.hpp: the backward rule over keys, the one the live
//             mosaic's commit runs; T steps at most, g clamped whatever the bytes hold) and leaves (g | start bit) or GAP
//             per column in the arg row; it then lists and counts the starts.  All threads fill the per-frame outputs from
//             that row (mosaic_frame) and pad.
//             (As the forward kernel's tail the same lines cost that kernel 49 spilled SGPRs.)
// A call whose slabs would pass the scratch cap runs fewer workgroups than targets: rounds of `grid` targets, a forward and
// a back-trace launch each, in stream order on the same slabs.
// pos(g) clipped at 2 (one byte per source frame) and the transposed frames are made once per call by mosaic_prep_kernel
// and shared by every workgroup.
// No workgroup waits on another: no spin wait, no cooperative launch; stream order is the only ordering between kernels.
#include "dtw_mosaic_common.hpp"

#include <algorithm>
#include <cmath>

namespace ssym {

namespace {

constexpr uint32_t kNone = kCoverNone;

struct MosaicArgs {
    MosaicCore k;                // k.G: source frames of the whole dictionary; k.slab: [grid][4 G + 1], E / N of the two
                                 // parities, then best(T-1)
    const double *srcRaw;
    const uint64_t *srcOff;
    uint32_t nSrc;
    const double *tgtRaw;
    const uint64_t *tgtOff;
    uint32_t nTgt;
    uint32_t t0;                 // the round's first target: workgroup b takes target t0 + b
    uint64_t maxT;               // the longest target: what a workgroup's rows hold
    uint32_t *path;              // [grid][maxT] arg(j); after the walk g | kMosaicStart, or GAP
    uint8_t *dir;                // [grid][maxT][G]
    uint32_t *outCount;          // [nTgt]; every output may be NULL
    double *outTotal;            // [nTgt]
    uint32_t *outStart, *outSrc, *outFrame;   // [frames]
    double *outCost;             // [frames]
};

__global__ __launch_bounds__(kMosaicThreads) void mosaic_forward_kernel(const MosaicArgs a)
{
    __shared__ double ring[2][kMosaicMaxDim];                // target frames j and j + 1
    __shared__ double partV[2][kMosaicMaxWaves];
    __shared__ uint32_t partG[2][kMosaicMaxWaves];
    const double INF = __builtin_inf();
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t G = a.k.G, dim = a.k.dim;
    MosaicCore k = a.k;
    k.slab += (size_t)blockIdx.x * (4 * (size_t)G + 1);
    const MosaicColumns cols{a.dir + (size_t)blockIdx.x * a.maxT * G, a.path + (size_t)blockIdx.x * a.maxT, G, ~0ull};
    const uint32_t t = a.t0 + blockIdx.x;
    if (t >= a.nTgt)
        return;
    const uint64_t f0 = a.tgtOff[t];
    const uint64_t T = a.tgtOff[t + 1] - f0;
    const double *b0 = a.tgtRaw + f0 * dim;
    // column -1: nothing to continue and nothing to repeat
    for (uint32_t g = tid; g < G; g += nthr) {
        k.slab[(size_t)2 * G + g] = INF;
        k.slab[(size_t)3 * G + g] = INF;
    }
    if (T)
        for (uint32_t e = tid; e < dim; e += nthr)
            ring[0][e] = b0[e];
    __syncthreads();

    double best = 0.0;                                       // best(j-1), the same in every thread
    for (uint64_t j = 0; j < T; ++j)
        best = mosaic_column(k, cols, j, best, ring, partV, partG, [&](double *row) {
            if (j + 1 < T)
                for (uint32_t e = tid; e < dim; e += nthr)
                    row[e] = b0[(j + 1) * dim + e];
        });
    if (tid == 0)
        k.slab[(size_t)4 * G] = T ? best : INF;
}

__global__ __launch_bounds__(kMosaicThreads) void mosaic_backtrace_kernel(const MosaicArgs a)
{
    __shared__ uint32_t shCount;
    const double INF = __builtin_inf();
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t G = a.k.G, dim = a.k.dim;
    const MosaicColumns cols{a.dir + (size_t)blockIdx.x * a.maxT * G, a.path + (size_t)blockIdx.x * a.maxT, G, ~0ull};
    const uint32_t t = a.t0 + blockIdx.x;
    if (t >= a.nTgt)
        return;
    const uint64_t f0 = a.tgtOff[t];
    const uint64_t T = a.tgtOff[t + 1] - f0;
    const double *b0 = a.tgtRaw + f0 * dim;
    const double best = a.k.slab[(size_t)blockIdx.x * (4 * (size_t)G + 1) + (size_t)4 * G];
    const bool ok = T > 0 && best < INF;
    if (tid == 0) {
        uint32_t count = 0;
        if (ok) {
            const long long top = (long long)T - 1;
            mosaic_walk(cols, mosaic_enter(cols, cols.word(top), top), top, -1);
            for (uint64_t j = 0; j < T; ++j)
                if (cols.arg[j] & kMosaicStart) {            // a piece or a gap frame starts: GAP has the bit as well
                    if (a.outStart)
                        a.outStart[f0 + count] = (uint32_t)j;
                    ++count;
                }
        }
        if (a.outCount)
            a.outCount[t] = count;
        if (a.outTotal)
            a.outTotal[t] = ok ? best : INF;
        shCount = count;
    }
    __syncthreads();
    const uint32_t count = shCount;
    for (uint64_t f = tid; f < T; f += nthr) {
        MosaicFrame o{kNone, kNone, INF};
        if (ok)
            o = mosaic_frame(cols.arg[f], a.srcRaw, a.srcOff, a.nSrc, a.k, b0 + f * dim);
        if (a.outSrc)
            a.outSrc[f0 + f] = o.src;
        if (a.outFrame)
            a.outFrame[f0 + f] = o.frame;
        if (a.outCost)
            a.outCost[f0 + f] = o.cost;
        if (a.outStart && f >= count)
            a.outStart[f0 + f] = kNone;
    }
}

// the bytes one running workgroup needs for a longest target of maxT frames: G maxT direction bytes, 32 G + 8 of state and
// the arg row
uint64_t mosaic_slab_bytes(uint64_t G, uint64_t maxT)
{
    return G * maxT + 32 * G + 8 + 4 * maxT;
}

int32_t dtw_mosaic(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double piece_penalty, double gap_cost, uint32_t flags,
                   uint32_t *out_count, double *out_total, uint32_t *out_start, uint32_t *out_src, uint32_t *out_frame,
                   double *out_frame_cost)
{
    const char *fn = "ssym_dtw_mosaic";
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
    const uint32_t M = tgt.n;
    const uint64_t F = tgt.total_frames, G = src.total_frames;
    ssym_timings tm{};
    tm.n_pairs = G * F;                                      // cells
    if (M == 0) {
        ctx->timings = tm;
        return SSYM_OK;
    }
    rc = check_sets(ctx->err, src, tgt);
    if (rc != SSYM_OK) {
        ctx->err = std::string(fn) + ": " + ctx->err;
        return rc;
    }
    if (src.dim > kMosaicMaxDim) {
        ctx->err = std::string(fn) + ": frames have more than " + std::to_string(kMosaicMaxDim) + " values";
        return SSYM_E_UNSUPPORTED;
    }
    uint64_t cap = kMosaicScratchBytes;
    if (const char *k = ssym_knob("SSYM_MOSAIC_SCRATCH_BYTES"))      // tests: force the workgroup stride, or the refusal
        cap = std::min<uint64_t>(cap, strtoull(k, nullptr, 10));
    uint64_t maxT = 0;
    for (uint32_t t = 0; t < M; ++t)
        maxT = std::max(maxT, tgt.h_off[t + 1] - tgt.h_off[t]);
    const uint64_t posBytes = ((G + 15) & ~15ull) + G * src.dim * sizeof(double);      // pos and the transposed frames
    // (G and maxT each below 2^32 keep the product below 2^64; a set beyond either cannot fit the cap)
    if (G > 0xffffffffull || maxT > 0xffffffffull || mosaic_slab_bytes(G, maxT) + posBytes > cap) {
        ctx->err = std::string(fn) + ": a target's tables need G x T + 33 G + 8 G dim + 4 T + 24 bytes (G source frames, T target frames), more than " +
                   std::to_string(cap >> 20) + " MiB of scratch; cut the target";
        return SSYM_E_UNSUPPORTED;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    Blocks bl(ctx);
    // outputs, every one nullable: the caller's device arrays in place, or one f64 and one u32 block copied back at the end
    StagedOut out(flags, {{out_total, M}, {out_frame_cost, F}}, {{out_count, M}, {out_start, F}, {out_src, F}, {out_frame, F}});
    rc = out.alloc(bl);
    if (rc != SSYM_OK)
        return rc;
    MosaicArgs a{};
    a.outTotal = out.f64[0];
    a.outCost = out.f64[1];
    a.outCount = out.u32[0];
    a.outStart = out.u32[1];
    a.outSrc = out.u32[2];
    a.outFrame = out.u32[3];

    // fewer workgroups than targets where the slabs would pass the cap: rounds of `grid` targets on the same slabs
    const uint64_t slab = mosaic_slab_bytes(G, maxT);
    const unsigned grid = (unsigned)std::min<uint64_t>({(uint64_t)M, (cap - posBytes) / std::max<uint64_t>(slab, 1), (uint64_t)ctx->num_cus * 2});
    const uint64_t stateBytes = (uint64_t)grid * (32 * G + 8), pathBytes = ((uint64_t)grid * 4 * maxT + 15) & ~15ull;
    rc = ensure(ctx, ctx->mosaic_tab, (size_t)(stateBytes + pathBytes + posBytes + (uint64_t)grid * G * maxT) + 64);
    if (rc != SSYM_OK)
        return rc;
    char *base = (char *)ctx->mosaic_tab.ptr;
    a.k.slab = (double *)base;
    a.path = (uint32_t *)(base + stateBytes);
    double *srcT = (double *)(base + stateBytes + pathBytes);
    uint8_t *posc = (uint8_t *)(srcT + G * src.dim);
    a.k.srcT = srcT;
    a.k.posc = posc;
    a.dir = (uint8_t *)srcT + posBytes;
    a.srcRaw = src.raw;
    a.srcOff = src.off;
    a.nSrc = src.n;
    a.k.G = (uint32_t)G;
    a.tgtRaw = tgt.raw;
    a.tgtOff = tgt.off;
    a.nTgt = M;
    a.k.dim = src.dim;
    a.k.squared = ctx->squared;
    a.k.penalty = piece_penalty;
    a.k.gapCost = gap_cost;
    a.maxT = maxT;

    hipEvent_t *ev = ctx->ev;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    if (G) {
        mosaic_prep_kernel<<<(unsigned)((G + 255) / 256), 256, 0, st>>>(src.off, src.n, (uint32_t)G, src.raw, src.dim, posc, srcT);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    for (uint32_t t0 = 0; t0 < M; t0 += grid) {
        a.t0 = t0;
        const unsigned blocks = std::min<unsigned>(grid, M - t0);
        mosaic_forward_kernel<<<blocks, kMosaicThreads, 0, st>>>(a);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        mosaic_backtrace_kernel<<<blocks, kMosaicThreads, 0, st>>>(a);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        ++tm.main_launches;
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    rc = out.finish(ctx);
    if (rc != SSYM_OK)
        return rc;
    tm.main_ms = ev_ms(ev[1], ev[2]);
    tm.total_ms = ev_ms(ev[0], ev[2]);
    ctx->timings = tm;
    return SSYM_OK;
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_dtw_mosaic(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double piece_penalty, double gap_cost,
                        uint32_t flags, uint32_t *out_count, double *out_total, uint32_t *out_start, uint32_t *out_src,
                        uint32_t *out_frame, double *out_frame_cost)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_mosaic(ctx, dict, q, piece_penalty, gap_cost, flags, out_count, out_total, out_start, out_src, out_frame,
                          out_frame_cost);
    });
}
}
