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
//   forward   mosaic_forward_kernel, one workgroup per target, the column loop inside.  The source frames are spread over
//             the threads (g = thread, thread + blockDim, ...).  E and N of column j-1 sit in a ping-pong slab of global
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
//             back, T steps at most, clamping g whatever the bytes hold, and leaves (g | start bit) or GAP per column in
//             the arg row; it then lists the starts.  All threads fill the per-frame outputs from that row and pad.
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

constexpr uint32_t kNone = kCoverNone, kGap = kCoverGap;

struct MosaicArgs {
    const double *srcRaw;
    const uint64_t *srcOff;
    uint32_t nSrc;
    uint32_t G;                  // source frames of the whole dictionary
    const double *tgtRaw;
    const uint64_t *tgtOff;
    uint32_t nTgt;
    uint32_t t0;                 // the round's first target: workgroup b takes target t0 + b
    uint32_t dim;
    int squared;
    double penalty, gapCost;
    uint64_t maxT;               // the longest target: what a workgroup's rows hold
    const uint8_t *posc;         // [G] min(pos(g), 2)
    const double *srcT;          // [dim][G] the source frames, transposed
    double *state;               // [grid][4 G + 1]: E / N of the two parities, then best(T-1)
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
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, nWaves = nthr >> 6;
    const uint32_t G = a.G, dim = a.dim;
    double *slab = a.state + (size_t)blockIdx.x * (4 * (size_t)G + 1);
    uint32_t *path = a.path + (size_t)blockIdx.x * a.maxT;
    uint8_t *dir = a.dir + (size_t)blockIdx.x * a.maxT * G;
    const uint32_t t = a.t0 + blockIdx.x;
    if (t >= a.nTgt)
        return;
    {
        const uint64_t f0 = a.tgtOff[t];
        const uint64_t T = a.tgtOff[t + 1] - f0;
        const double *b0 = a.tgtRaw + f0 * dim;
        // column -1: nothing to continue and nothing to repeat
        for (uint32_t g = tid; g < G; g += nthr) {
            slab[(size_t)2 * G + g] = INF;
            slab[(size_t)3 * G + g] = INF;
        }
        if (T)
            for (uint32_t e = tid; e < dim; e += nthr)
                ring[0][e] = b0[e];
        __syncthreads();

        double best = 0.0;                                   // best(j-1), the same in every thread
        for (uint64_t j = 0; j < T; ++j) {
            const uint32_t par = (uint32_t)j & 1;
            const double S = __dadd_rn(a.penalty, best);
            const double *Eo = slab + (size_t)(par ^ 1) * 2 * G, *No = Eo + G;
            double *En = slab + (size_t)par * 2 * G, *Nn = En + G;
            uint8_t *dcol = dir + j * G;
            double bv = INF;
            uint32_t bg = kNone;
            for (uint32_t g = tid; g < G; g += nthr) {
                const uint32_t pc = a.posc[g];
                const double nOld = No[g];
                double P = INF;
                uint32_t code = 0;
                if (pc >= 1)
                    P = Eo[g - 1];
                if (pc >= 2) {
                    const double e2 = Eo[g - 2];
                    if (e2 < P) {
                        P = e2;
                        code = 1;
                    }
                }
                if (!(P <= S)) {
                    P = S;
                    code = 2;
                }
                const double c = mosaic_cost(a.srcT + g, G, ring[par], dim, a.squared);
                const double nD = __dadd_rn(c, P);
                const double hD = __dadd_rn(c, nOld);
                const bool rep = hD < nD;
                const double eD = rep ? hD : nD;
                En[g] = eD;
                Nn[g] = nD;
                dcol[g] = (uint8_t)(code << 1 | (rep ? 1u : 0u));
                if (eD < bv) {                               // g ascends within a thread: the first minimum stays
                    bv = eD;
                    bg = g;
                }
            }
            if (j + 1 < T)
                for (uint32_t e = tid; e < dim; e += nthr)
                    ring[par ^ 1][e] = b0[(j + 1) * dim + e];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double oV = __shfl_xor(bv, m);
                const uint32_t oG = (uint32_t)__shfl_xor((int)bg, m);
                if (oV < bv || (oV == bv && oG < bg)) {
                    bv = oV;
                    bg = oG;
                }
            }
            if ((tid & 63) == 0) {
                partV[par][wave] = bv;
                partG[par][wave] = bg;
            }
            __syncthreads();
            double v = INF;
            uint32_t arg = kNone;
            for (uint32_t w = 0; w < nWaves; ++w) {
                const double oV = partV[par][w];
                const uint32_t oG = partG[par][w];
                if (oV < v || (oV == v && oG < arg)) {
                    v = oV;
                    arg = oG;
                }
            }
            const double vg = __dadd_rn(a.gapCost, best);
            if (vg < v) {
                v = vg;
                arg = kGap;
            }
            best = v;
            if (tid == 0)
                path[j] = arg;
        }
        if (tid == 0)
            slab[(size_t)4 * G] = T ? best : INF;
    }
}

__global__ __launch_bounds__(kMosaicThreads) void mosaic_backtrace_kernel(const MosaicArgs a)
{
    __shared__ uint32_t shCount;
    const double INF = __builtin_inf();
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t G = a.G, dim = a.dim;
    uint32_t *path = a.path + (size_t)blockIdx.x * a.maxT;
    const uint8_t *dir = a.dir + (size_t)blockIdx.x * a.maxT * G;
    const uint32_t t = a.t0 + blockIdx.x;
    if (t >= a.nTgt)
        return;
    {
        const uint64_t f0 = a.tgtOff[t];
        const uint64_t T = a.tgtOff[t + 1] - f0;
        const double *b0 = a.tgtRaw + f0 * dim;
        const double best = a.state[(size_t)blockIdx.x * (4 * (size_t)G + 1) + (size_t)4 * G];
        const bool ok = T > 0 && best < INF;
        if (tid == 0) {
            uint32_t count = 0;
            if (ok) {
                uint32_t g = path[T - 1];
                bool forceN = false;
                for (uint64_t j = T; j-- > 0;) {             // T steps, whatever the bytes hold
                    if (g >= G) {                            // GAP (anything else beyond G cannot be; it is read as one)
                        path[j] = kGap;
                        ++count;
                        forceN = false;
                        if (j)
                            g = path[j - 1];
                        continue;
                    }
                    const uint32_t d = dir[j * G + g];
                    if ((d & 1) && !forceN) {                // state H: the cell before is (g, j-1) in state N
                        path[j] = g;
                        forceN = true;
                        continue;
                    }
                    forceN = false;
                    const uint32_t code = d >> 1;
                    if (code >= 2 || j == 0) {               // a piece starts here
                        path[j] = g | kMosaicStart;
                        ++count;
                        if (j)
                            g = path[j - 1];
                    } else {
                        path[j] = g;
                        g = g > code ? g - 1 - code : 0;
                    }
                }
                if (a.outStart) {
                    uint32_t k = 0;
                    for (uint64_t j = 0; j < T; ++j)
                        if (path[j] & kMosaicStart)          // GAP has the bit as well
                            a.outStart[f0 + k++] = (uint32_t)j;
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
            uint32_t src = kNone, frame = kNone;
            double cost = INF;
            if (ok) {
                const uint32_t p = path[f];
                if (p == kGap) {
                    src = kGap;
                    cost = a.gapCost;
                } else {
                    const uint32_t g = min(p & ~kMosaicStart, G - 1);
                    src = mosaic_segment(a.srcOff, a.nSrc, g);
                    frame = (uint32_t)(g - a.srcOff[src]);
                    cost = mosaic_cost(a.srcRaw + (size_t)g * dim, 1, b0 + f * dim, dim, a.squared);
                }
            }
            if (a.outSrc)
                a.outSrc[f0 + f] = src;
            if (a.outFrame)
                a.outFrame[f0 + f] = frame;
            if (a.outCost)
                a.outCost[f0 + f] = cost;
            if (a.outStart && f >= count)
                a.outStart[f0 + f] = kNone;
        }
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
    a.state = (double *)base;
    a.path = (uint32_t *)(base + stateBytes);
    double *srcT = (double *)(base + stateBytes + pathBytes);
    uint8_t *posc = (uint8_t *)(srcT + G * src.dim);
    a.srcT = srcT;
    a.posc = posc;
    a.dir = (uint8_t *)srcT + posBytes;
    a.srcRaw = src.raw;
    a.srcOff = src.off;
    a.nSrc = src.n;
    a.G = (uint32_t)G;
    a.tgtRaw = tgt.raw;
    a.tgtOff = tgt.off;
    a.nTgt = M;
    a.dim = src.dim;
    a.squared = ctx->squared;
    a.penalty = piece_penalty;
    a.gapCost = gap_cost;
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
