// dtw_mosaicker.hip -- the live mosaic: growing targets tiled by free spans of the uncut recordings of one resident
// dictionary, every target frame reported by the push after which no longer recording could change it (DESIGN.md 2 "Live
// mosaic", 5.26).
//
// Role on the path: ssym_dtw_mosaic needs its whole target up front and keeps one direction byte per (source frame, target
// frame).  A mosaicker is its resumable form, lane by lane, as a coverer is ssym_dtw_cover's: what it emits from reset to
// flush is, frame for frame and bit for bit, what ssym_dtw_mosaic gives for the whole, and its tables hold the uncommitted
// columns alone.
//
// Definition.  c, S, P, open, Q, H, N, E, best, arg, the tie rules and the arithmetic are those of "Mosaic" (dtw_mosaic.hip),
// word for word.  For one lane, X is everything consumed so far and n its frame count.
//   resume   : the lane holds n, E(., n-1) and N(., n-1), best(n-1), the direction byte of every (g, j) and arg(j) for every
//              column j after the committed column, done (the last committed column, -1 at first) and lastFinite (the
//              largest j with a finite best(j), -1 at first).  Consuming frames n ... n+m-1 runs columns n ... n+m-1 exactly
//              as "Mosaic" does.
//   key      : a position of the backward walk at column j: (g, H), (g, N) or GAP.  A walk steps from a key at column j to
//              one at column j-1 by the "backward" rule of "Mosaic"; two walks that share a key at a column are the same
//              from there back.
//   live(n)  : S' = piece_penalty + best(n-1), as the next column will form it.  Every g with E(g, n-1) finite and <= S', in
//              the state bit 0 says (H if H < N, else N); every g whose bit 0 is set and whose N(g, n-1) is finite and
//              <= S', in state N; GAP if arg(n-1) = GAP and best(n-1) is finite.  NaN is never live.
//   commit   : c(n) = the largest column <= n-1 at which all walks of live(n) hold the same key, -1 if there is none;
//              live(n) empty: unchanged.  A push emits frames done+1 ... c(n), then done = c(n).
//   dead     : best(n-1) not finite makes every later column +inf.  A dead lane goes on counting frames but stores nothing
//              more and commits nothing more (its last commit is c(lastFinite + 1)).
//   flush    : emits the rest of the walk from arg(lastFinite) at column lastFinite; the lane has then ENDED until reset.
//   best     : total = best(n-1) (+inf for n = 0 or when not finite), covered = lastFinite + 1, committed = done + 1
// Why: a state above S' is never used by column n.  E: as the P of a successor it is > S', and that successor opens; else
// the other predecessor was taken.  N: H(g,n) = c + N(g,n-1) wins only if it is < c + Q with Q <= S', and rounding is
// monotone.  So every mosaic of every longer X passes through a live state at column n-1, and hence through the common key.
//
// Mapping.
//   create    mosaic_prep_kernel (dtw_mosaic_common.hpp) once: pos(g) and the transposed source frames stay with the object.
//   forward   mosaicker_forward_kernel, one workgroup per lane with new frames: the column body is mosaic_column
//             (dtw_mosaic_common.hpp), the one mosaic_forward_kernel runs.  E / N of column j sit in the lane's slab at
//             parity j & 1 (4 G doubles per lane), so column n-1 is where a push finds it; best(n-1) comes from the lane's
//             record.  Direction bytes, arg(j) and the target frame (the emission's frame cost needs it) go into the lane's
//             ring, column j at j mod cap.  The loop stops at the first column whose best is not finite: the slab of column
//             lastFinite stays.
//   commit    mosaicker_commit_kernel, one workgroup per lane.  The live keys of column lastFinite are collected into a
//             list; each step maps the list one column back through the ring into a second list, a key going in only if it
//             is the first to raise its flag (duplicates drop as walks merge; the flags are lowered again before the next
//             step).  It stops when one key is left (at once when the keys already agree) or at column done + 1.  Thread 0
//             then walks from that key down to done + 1, leaving g | start bit or GAP in the arg ring, and all threads fill
//             the call's frame log in ascending column with plain stores.  The keys, the step back, the walk and the frame's
//             (src, frame, cost) are dtw_mosaic_common.hpp's (mosaic_enter / mosaic_back, mosaic_walk, mosaic_frame), the ones
//             mosaic_backtrace_kernel runs on the offline tables.  A flush is the same emission from arg(lastFinite).
//   regrow    mosaicker_regrow_kernel moves the uncommitted columns when the ring doubles.
// Host: the checks, the upload and the bodies of push / follow / flush / reset are lane_feed.hpp's, and so is the frame log
// (LaneLog).  What the mosaicker shares with the coverer is lane_tiling.hpp's: the base of the handle, the dictionary check,
// the first refusals of create, best's host body, the hand-over of a grown ring, and the loop over a call's slices
// (tiling_run): forward between its first two events, commit between the last two.  A slice that is refused or fails leaves
// through that loop's epilogue.  The slice's plan with its budget refusal is here (MosaickerSlices).
// No workgroup waits on another: no spin wait; stream order is the only ordering between kernels.
#include "dtw_mosaic_common.hpp"
#include "lane_feed.hpp"
#include "lane_tiling.hpp"

#include <algorithm>
#include <cmath>

namespace ssym {

constexpr uint32_t kMosaickerMaxLanes = 65535;                   // one workgroup per lane
constexpr uint64_t kMosaickerRingBytes = 64ull << 20;            // the initial ring
constexpr uint64_t kMosaickerRingMax = 1024, kMosaickerRingMin = 16;

// a lane's record on the device
struct MosLane {
    long long n;                 // frames consumed
    long long stored;            // columns the ring has seen: n, or the first column without a finite best + 1
    long long done;              // the last committed column, -1 at first
    long long lastFinite;        // the largest j with a finite best(j), -1 at first
    unsigned long long count;    // frames the last commit or flush wrote into the log
    double best;                 // best(n-1); 0 at n = 0
    double bestFinite;           // best(lastFinite); 0 at first
};

// what one slice of a call does with a lane
struct MosStep {
    const double *rows;          // the new frames (DEVICE), m x dim
    uint64_t logAt;              // where the lane's next frame goes in the log
    uint32_t m;                  // new frames
    uint32_t flush;              // 1: emit the walk from arg(lastFinite)
};

}  // namespace ssym

// beside what every live tiling holds (lane_tiling.hpp; the words of the log, the frames of the last push / follow / flush,
// are lane, column, src, frame, start)
struct ssym_mosaicker : ssym::LaneTiling {
    ssym_mosaicker() : LaneTiling(5) {}
    uint32_t G = 0;
    uint64_t budget = 0;                     // bytes the object may own
    uint64_t fixedBytes = 0;                 // what it owns beside the ring
    std::vector<int64_t> stored;             // host mirrors of the lanes'
    std::vector<uint8_t> dead;
    // device
    double *srcT = nullptr;                  // [dim][G]
    uint8_t *posc = nullptr;                 // [G]
    double *slab = nullptr;                  // [nLanes][4 G]: E / N of the two column parities
    uint32_t *keys = nullptr;                // [nLanes][3][2 G + 2]: the commit's two key lists and its flags (all 0 between steps)
    ssym::MosLane *lanes = nullptr;          // [nLanes]
    ssym::MosStep *dSteps = nullptr;         // [nLanes]
    uint64_t cap = 0;                        // columns per lane of the ring, a power of two
    uint8_t *dir = nullptr;                  // [nLanes][cap][G], column j at j mod cap
    uint32_t *arg = nullptr;                 // [nLanes][cap]
    double *frames = nullptr;                // [nLanes][cap][dim]
};

namespace ssym {
namespace {

constexpr uint32_t kGap = kCoverGap;

__global__ __launch_bounds__(256) void mosaicker_init_kernel(MosLane *lanes, uint32_t lane0, uint32_t nLanes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nLanes)
        lanes[lane0 + i] = MosLane{0, 0, -1, -1, 0, 0.0, 0.0};
}

struct MosForwardArgs {
    const MosStep *steps;
    MosLane *lanes;
    MosaicCore k;                // k.slab: [nLanes][4 G]
    uint64_t cap;
    uint8_t *dir;
    uint32_t *arg;
    double *frames;
};

// the commit walks the same ring; its emission reads the dictionary's raw rows and fills the log
struct MosCommitArgs : MosForwardArgs {
    const double *srcRaw;
    const uint64_t *srcOff;
    uint32_t nSrc;
    uint32_t *keys;
    uint32_t *logLane, *logColumn, *logSrc, *logFrame, *logStart;
    double *logCost;
};

__global__ __launch_bounds__(kMosaicThreads) void mosaicker_forward_kernel(const MosForwardArgs a)
{
    __shared__ double ring[2][kMosaicMaxDim];                // target frames j and j + 1
    __shared__ double partV[2][kMosaicMaxWaves];
    __shared__ uint32_t partG[2][kMosaicMaxWaves];
    const double INF = __builtin_inf();
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t G = a.k.G, dim = a.k.dim, l = blockIdx.x;
    const MosStep s = a.steps[l];
    if (s.m == 0)
        return;
    const MosLane st = a.lanes[l];
    if (st.n > 0 && !(st.best < INF)) {                      // dead: the frames are counted, nothing else
        if (tid == 0)
            a.lanes[l].n = st.n + s.m;
        return;
    }
    MosaicCore k = a.k;
    k.slab += (size_t)l * 4 * G;
    const uint64_t mask = a.cap - 1;
    const MosaicColumns cols{a.dir + (size_t)l * a.cap * G, a.arg + (size_t)l * a.cap, G, mask};
    double *kept = a.frames + (size_t)l * a.cap * dim;
    const double *b0 = s.rows;
    const uint64_t n = (uint64_t)st.n;
    if (n == 0)                                              // column -1: nothing to continue and nothing to repeat
        for (uint32_t g = tid; g < G; g += nthr) {
            k.slab[(size_t)2 * G + g] = INF;
            k.slab[(size_t)3 * G + g] = INF;
        }
    for (uint32_t e = tid; e < dim; e += nthr) {
        const double v = b0[e];
        ring[n & 1][e] = v;
        kept[(n & mask) * dim + e] = v;
    }
    __syncthreads();

    double best = st.best;                                   // best(j-1), the same in every thread
    double bestFinite = st.bestFinite;
    long long lastFinite = st.lastFinite;
    uint64_t j = n;
    const uint64_t end = n + s.m;
    for (; j < end; ++j) {
        best = mosaic_column(k, cols, j, best, ring, partV, partG, [&](double *row) {
            if (j + 1 < end)
                for (uint32_t e = tid; e < dim; e += nthr) {
                    const double v = b0[(j + 1 - n) * dim + e];
                    row[e] = v;
                    kept[((j + 1) & mask) * dim + e] = v;    // the emission's frame cost needs it
                }
        });
        if (!(best < INF)) {                                 // the lane dies here (every thread sees the same best)
            ++j;
            break;
        }
        lastFinite = (long long)j;
        bestFinite = best;
    }
    if (tid == 0) {
        MosLane o = st;
        o.n = (long long)end;
        o.stored = (long long)j;
        o.lastFinite = lastFinite;
        o.best = best;
        o.bestFinite = bestFinite;
        a.lanes[l] = o;
    }
}

__global__ __launch_bounds__(kMosaicThreads) void mosaicker_commit_kernel(const MosCommitArgs a)
{
    __shared__ uint32_t shN[2];
    __shared__ long long shC;
    const uint32_t l = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const MosStep s = a.steps[l];
    if (s.m == 0 && !s.flush)
        return;
    const double INF = __builtin_inf();
    const MosLane st = a.lanes[l];
    const uint32_t G = a.k.G, dim = a.k.dim;
    const MosaicColumns cols{a.dir + (size_t)l * a.cap * G, a.arg + (size_t)l * a.cap, G, a.cap - 1};
    const double *kept = a.frames + (size_t)l * a.cap * dim;
    const size_t K = 2 * (size_t)G + 2;
    uint32_t *lists = a.keys + (size_t)l * 3 * K, *flag = lists + 2 * K;
    const long long done = st.done, top = st.lastFinite;
    auto slot = [&](uint32_t key) -> size_t { return key == kGap ? 2 * (size_t)G : key; };

    long long c = done;                                      // the last column that is final
    uint32_t tip = kGap;                                     // the key at it
    if (top > done) {
        if (s.flush) {
            c = top;
            tip = mosaic_enter(cols, cols.word(top), top).key;
        } else {
            // live(lastFinite + 1): for a lane that lives lastFinite = n - 1; for one that died the last commit there was
            if (tid == 0)
                shN[0] = shN[1] = 0;
            __syncthreads();
            const double S = __dadd_rn(a.k.penalty, st.bestFinite);
            const double *E = a.k.slab + (size_t)l * 4 * G + (size_t)((uint64_t)top & 1) * 2 * G, *N = E + G;
            for (uint32_t g = tid; g < G; g += nthr) {
                const uint32_t d = cols.byte(top, g);
                const double e = E[g];
                if (e > -INF && e <= S)
                    lists[atomicAdd(&shN[0], 1u)] = g << 1 | (d & 1u);
                if (d & 1u) {
                    const double nn = N[g];
                    if (nn > -INF && nn <= S)
                        lists[atomicAdd(&shN[0], 1u)] = g << 1;
                }
            }
            if (tid == 0 && cols.word(top) == kGap)
                lists[atomicAdd(&shN[0], 1u)] = kGap;
            __syncthreads();
            // every step maps the list one column back (column col - 1 > done: it is in the ring)
            uint32_t cur = 0;
            long long col = top;
            uint32_t cnt = shN[0];
            while (cnt > 1 && col > done + 1) {
                const uint32_t *from = lists + cur * K;
                uint32_t *to = lists + (cur ^ 1) * K;
                for (uint32_t i = tid; i < cnt; i += nthr) {
                    const uint32_t nk = mosaic_back(cols, mosaic_pos(cols, from[i], col), col).key;
                    if (atomicExch(&flag[slot(nk)], 1u) == 0u)
                        to[atomicAdd(&shN[cur ^ 1], 1u)] = nk;
                }
                __syncthreads();
                cnt = shN[cur ^ 1];
                for (uint32_t i = tid; i < cnt; i += nthr)
                    flag[slot(to[i])] = 0u;
                if (tid == 0)
                    shN[cur] = 0;
                cur ^= 1;
                --col;
                __syncthreads();
            }
            if (cnt == 1) {
                c = col;
                tip = lists[cur * K];
            }
        }
    }
    if (c < done)
        c = done;
    // every thread has its copy of the lane record before thread 0 stores the new `done`: the flush path has
    // no other barrier between the two
    __syncthreads();
    if (tid == 0) {
        mosaic_walk(cols, mosaic_pos(cols, tip, c), c, done);
        a.lanes[l].done = c;
        a.lanes[l].count = (unsigned long long)(c - done);
        shC = c;
    }
    __syncthreads();
    c = shC;
    for (long long f = done + 1 + tid; f <= c; f += nthr) {
        const uint32_t p = cols.word(f);
        const MosaicFrame o = mosaic_frame(p, a.srcRaw, a.srcOff, a.nSrc, a.k, kept + ((uint64_t)f & cols.mask) * dim);
        const uint64_t k = s.logAt + (uint64_t)(f - done - 1);
        a.logLane[k] = l;
        a.logColumn[k] = (uint32_t)f;
        a.logSrc[k] = o.src;
        a.logFrame[k] = o.frame;
        a.logStart[k] = (p & kMosaicStart) ? 1u : 0u;        // GAP has the bit as well
        a.logCost[k] = o.cost;
    }
}

// the uncommitted columns, from a ring of oldCap columns per lane into one of newCap; grid (blocks, lanes)
__global__ __launch_bounds__(256) void mosaicker_regrow_kernel(const MosLane *lanes, uint32_t G, uint32_t dim, uint64_t oldCap,
                                                               uint64_t newCap, const uint8_t *oldDir, const uint32_t *oldArg,
                                                               const double *oldFrames, uint8_t *newDir, uint32_t *newArg,
                                                               double *newFrames)
{
    const uint32_t l = blockIdx.y;
    const long long first = lanes[l].done + 1, n = lanes[l].stored;
    for (long long j = first + blockIdx.x; j < n; j += gridDim.x) {
        const size_t from = (size_t)l * oldCap + ((uint64_t)j & (oldCap - 1)), to = (size_t)l * newCap + ((uint64_t)j & (newCap - 1));
        for (uint32_t g = threadIdx.x; g < G; g += blockDim.x)
            newDir[to * G + g] = oldDir[from * G + g];
        for (uint32_t e = threadIdx.x; e < dim; e += blockDim.x)
            newFrames[to * dim + e] = oldFrames[from * dim + e];
        if (threadIdx.x == 0)
            newArg[to] = oldArg[from];
    }
}

__global__ __launch_bounds__(256) void mosaicker_best_kernel(const MosLane *lanes, uint32_t nLanes, double *total, uint32_t *covered,
                                                             uint32_t *committed)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nLanes)
        return;
    const MosLane s = lanes[l];
    if (total)
        total[l] = s.n > 0 && s.best < __builtin_inf() ? s.best : __builtin_inf();
    if (covered)
        covered[l] = (uint32_t)(s.lastFinite + 1);
    if (committed)
        committed[l] = (uint32_t)(s.done + 1);
}

void mosaicker_free(ssym_ctx *ctx, ssym_mosaicker *mk)
{
    for (void *p : {(void *)mk->srcT, (void *)mk->posc, (void *)mk->slab, (void *)mk->keys, (void *)mk->lanes, (void *)mk->dSteps,
                    (void *)mk->dir, (void *)mk->arg, (void *)mk->frames})
        if (p)
            dev_free(ctx, p);
    mk->log.free(ctx);
    delete mk;
}

constexpr const char *kNoun = "mosaicker";

// bytes of one ring column of one lane: the direction bytes, arg and the target frame
uint64_t column_bytes(uint64_t G, uint32_t dim)
{
    return G + 4 + 8 * (uint64_t)dim;
}

// the ring with `cap` columns per lane (a power of two); the uncommitted stretches move over
int32_t ring_store(ssym_ctx *ctx, ssym_mosaicker *mk, uint64_t cap)
{
    uint8_t *dir = nullptr;
    uint32_t *arg = nullptr;
    double *frames = nullptr;
    int32_t rc = alloc_n(ctx, &dir, (size_t)mk->nLanes * cap * mk->G);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &arg, (size_t)mk->nLanes * cap);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &frames, (size_t)mk->nLanes * cap * mk->dim);
    return ring_swap(
        ctx, kNoun, rc, {mk->dir, mk->arg, mk->frames}, {dir, arg, frames}, mk->cap != 0,
        [&] {
            mosaicker_regrow_kernel<<<dim3(16, mk->nLanes), 256, 0, ctx->stream>>>(mk->lanes, mk->G, mk->dim, mk->cap, cap, mk->dir,
                                                                                   mk->arg, mk->frames, dir, arg, frames);
        },
        [&] {
            mk->dir = dir;
            mk->arg = arg;
            mk->frames = frames;
            mk->cap = cap;
        });
}

uint64_t knob_u64(const char *name, uint64_t otherwise)
{
    const char *k = ssym_knob(name);
    return k ? strtoull(k, nullptr, 10) : otherwise;
}

int32_t mosaicker_create(ssym_ctx *ctx, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty, double gap_cost,
                         ssym_mosaicker **out)
{
    const char *fn = "ssym_mosaicker_create";
    int32_t rc = tiling_create_checks(ctx, fn, dict, n_lanes, piece_penalty, gap_cost, out);
    if (rc != SSYM_OK)
        return rc;
    const SegmentSet &src = dict->set;
    if (src.dim > kMosaicMaxDim) {
        ctx->err = std::string(fn) + ": frames have more than " + std::to_string(kMosaicMaxDim) + " values";
        return SSYM_E_UNSUPPORTED;
    }
    if (n_lanes > kMosaickerMaxLanes) {
        ctx->err = std::string(fn) + ": more than " + std::to_string(kMosaickerMaxLanes) + " lanes";
        return SSYM_E_UNSUPPORTED;
    }
    const uint64_t G = src.total_frames, dim = src.dim;
    const uint64_t budget = std::min(kMosaicScratchBytes, knob_u64("SSYM_MOSAICKER_SCRATCH_BYTES", kMosaicScratchBytes));
    // beside the ring: pos and the transposed frames once, per lane the E / N slab, the commit's lists and flags, the records
    const uint64_t K = 2 * G + 2;
    const uint64_t fixed = ((G + 15) & ~15ull) + 8 * G * dim + (uint64_t)n_lanes * (32 * G + 12 * K + sizeof(MosLane) + sizeof(MosStep));
    const uint64_t col = column_bytes(G, src.dim);
    if (G > 0x7fffffffull || fixed > budget || (budget - fixed) / ((uint64_t)n_lanes * col) < kMosaickerRingMin) {
        ctx->err = std::string(fn) + ": the state needs G (1 + 8 dim) + lanes x (56 G + 16 x (G + 4 + 8 dim)) bytes (G source frames) at least, more than " +
                   std::to_string(budget >> 20) + " MiB; use fewer lanes per mosaicker or a smaller dictionary";
        return SSYM_E_UNSUPPORTED;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ssym_mosaicker *mk = new ssym_mosaicker;
    mk->bind(ctx, dict, n_lanes, piece_penalty, gap_cost);
    mk->G = (uint32_t)G;
    mk->budget = budget;
    mk->fixedBytes = fixed;
    mk->stored.assign(n_lanes, 0);
    mk->dead.assign(n_lanes, 0);
    // the initial ring: the largest power of two <= 1024 columns with lanes x cap x (G + 4) <= 64 MiB, 16 at least, within
    // the budget
    uint64_t cap = kMosaickerRingMax;
    while (cap > kMosaickerRingMin && (uint64_t)n_lanes * cap * (G + 4) > kMosaickerRingBytes)
        cap >>= 1;
    if (const char *k = ssym_knob("SSYM_MOSAICKER_RING"))
        cap = pow2_at_least(std::max<uint64_t>(kMosaickerRingMin, strtoull(k, nullptr, 10)));
    while (cap > kMosaickerRingMin && (uint64_t)n_lanes * cap * col > budget - fixed)
        cap >>= 1;
    rc = alloc_n(ctx, &mk->srcT, (size_t)(G * dim));
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &mk->posc, (size_t)G);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &mk->slab, (size_t)n_lanes * 4 * G);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &mk->keys, (size_t)n_lanes * 3 * K);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &mk->lanes, (size_t)n_lanes);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &mk->dSteps, (size_t)n_lanes);
    if (rc == SSYM_OK)
        rc = ring_store(ctx, mk, cap);
    if (rc != SSYM_OK) {
        mosaicker_free(ctx, mk);
        return rc;
    }
    hipError_t e = hipMemsetAsync(mk->keys, 0, sizeof(uint32_t) * (size_t)n_lanes * 3 * K, ctx->stream);
    if (e == hipSuccess && G) {
        mosaic_prep_kernel<<<(unsigned)((G + 255) / 256), 256, 0, ctx->stream>>>(src.off, src.n, (uint32_t)G, src.raw, src.dim, mk->posc,
                                                                                 mk->srcT);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        mosaicker_init_kernel<<<(n_lanes + 255) / 256, 256, 0, ctx->stream>>>(mk->lanes, 0u, n_lanes);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->err = std::string(fn) + ": " + hipGetErrorString(e);
        mosaicker_free(ctx, mk);
        return SSYM_E_HIP;
    }
    *out = mk;
    return SSYM_OK;
}

// The mosaicker's part of a push, follow or flush (the loop is tiling_run, lane_tiling.hpp): the frames go through in slices
// of at most sliceMax per lane, and of no more than the ring can take beside what it holds.
struct MosaickerSlices {
    ssym_ctx *ctx;
    ssym_mosaicker *mk;
    uint64_t sliceMax;
    uint64_t capMax;                         // the most columns the ring may grow to within the budget
    MosCommitArgs k;                         // the slice's kernel arguments

    // columns of lane l the ring holds uncommitted
    uint64_t pending(uint32_t l) const { return (uint64_t)(mk->stored[l] - (mk->done[l] + 1)); }

    int32_t plan(const TilingCall &call, std::vector<MosStep> &steps, uint64_t *left, uint64_t *need)
    {
        const uint32_t nL = mk->nLanes;
        // the slice: what the ring takes beside the longest uncommitted stretch of a lane that still has frames
        uint64_t most = 0;
        for (uint32_t l = 0; l < nL; ++l)
            if (call.m[l] > call.at[l]) {
                *left += call.m[l] - call.at[l];
                if (!mk->dead[l])
                    most = std::max(most, pending(l));
            }
        uint64_t slice = sliceMax;
        if (*left) {
            if (most >= capMax) {
                ctx->err = std::string(call.fn) + ": the uncommitted columns of a lane fill the " + std::to_string(mk->budget >> 20) +
                           " MiB the mosaicker may own (" + std::to_string(most) + " columns of " +
                           std::to_string(column_bytes(mk->G, mk->dim)) + " bytes on " + std::to_string(nL) +
                           " lanes); flush the lane (ssym_mosaicker_flush) and reset it";
                return SSYM_E_UNSUPPORTED;
            }
            slice = std::min(slice, capMax - most);
        }
        for (uint32_t l = 0; l < nL; ++l) {
            const uint64_t ml = tiling_step(mk, call, l, slice, &steps[l]);
            if (ml && !mk->dead[l])
                *need = std::max(*need, pending(l) + ml);
        }
        return SSYM_OK;
    }

    int32_t grow(uint64_t need) { return need > mk->cap ? ring_store(ctx, mk, pow2_at_least(need)) : SSYM_OK; }

    int32_t forward(bool any)
    {
        const SegmentSet &src = mk->dict->set;
        k = MosCommitArgs{};
        k.steps = mk->dSteps;
        k.lanes = mk->lanes;
        k.k = MosaicCore{mk->G, mk->dim, ctx->squared, mk->penalty, mk->gapCost, mk->posc, mk->srcT, mk->slab};
        k.srcRaw = src.raw;
        k.srcOff = src.off;
        k.nSrc = src.n;
        k.keys = mk->keys;
        k.cap = mk->cap;
        k.dir = mk->dir;
        k.arg = mk->arg;
        k.frames = mk->frames;
        k.logLane = mk->log.word(0);
        k.logColumn = mk->log.word(1);
        k.logSrc = mk->log.word(2);
        k.logFrame = mk->log.word(3);
        k.logStart = mk->log.word(4);
        k.logCost = mk->log.cost;
        if (any) {
            mosaicker_forward_kernel<<<mk->nLanes, kMosaicThreads, 0, ctx->stream>>>(k);          // (its part of the arguments)
            SSYM_HIP_CHECK(ctx, hipGetLastError());
        }
        return SSYM_OK;
    }

    int32_t commit(bool)
    {
        mosaicker_commit_kernel<<<mk->nLanes, kMosaicThreads, 0, ctx->stream>>>(k);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        return SSYM_OK;
    }

    void fold(uint32_t l, const MosLane &lane)
    {
        mk->stored[l] = lane.stored;
        mk->dead[l] = lane.n > 0 && !(lane.best < __builtin_inf());
    }
};

// what push, follow and flush hand to the entry bodies (lane_feed.hpp): the mosaicker's feed and its run
LaneFeed mosaicker_feed(ssym_ctx *ctx, const ssym_mosaicker *mk)
{
    return feed_of(ctx, mk, kNoun, "out_n_frames");
}

auto mosaicker_run(ssym_ctx *ctx, ssym_mosaicker *mk, uint64_t *out_n_frames)
{
    return [=](const char *fn, const std::vector<const double *> &rows, const std::vector<uint64_t> &m, uint32_t flushLane) -> int32_t {
        const uint64_t sliceMax = std::max<uint64_t>(knob_u64("SSYM_MOSAICKER_SLICE", kLaneMaxFrames), 1);
        // the most columns a ring may grow to within the budget (a power of two): while it doubles, the ring it leaves (half
        // of it at most) exists beside it
        uint64_t capMax = kMosaickerRingMin;
        while ((uint64_t)mk->nLanes * (capMax * 3) * column_bytes(mk->G, mk->dim) <= mk->budget - mk->fixedBytes)
            capMax *= 2;
        MosaickerSlices o{ctx, mk, sliceMax, std::max(capMax, mk->cap), MosCommitArgs{}};
        return tiling_run(ctx, mk, o, mk->dSteps, mk->lanes, mk->G, fn, rows, m, flushLane, out_n_frames);
    };
}

int32_t mosaicker_frames(ssym_ctx *ctx, const ssym_mosaicker *mk, uint32_t *out_lane, uint32_t *out_column, uint32_t *out_src,
                         uint32_t *out_frame, double *out_cost, uint32_t *out_start, uint32_t flags)
{
    int32_t rc = check_handle(ctx, mk, kNoun, "ssym_mosaicker_frames");
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint32_t *const outs[5] = {out_lane, out_column, out_src, out_frame, out_start};
    return mk->log.copy(ctx, out_cost, outs, (flags & SSYM_OUT_DEVICE) != 0);
}

int32_t mosaicker_best(ssym_ctx *ctx, const ssym_mosaicker *mk, double *out_total, uint32_t *out_covered, uint32_t *out_committed,
                       uint32_t flags)
{
    return tiling_best(ctx, mk, kNoun, "ssym_mosaicker_best", out_total, out_covered, out_committed, flags,
                       [&](double *total, uint32_t *covered, uint32_t *committed) {
                           const uint32_t nL = mk->nLanes;
                           mosaicker_best_kernel<<<(nL + 255) / 256, 256, 0, ctx->stream>>>(mk->lanes, nL, total, covered, committed);
                       });
}

}  // namespace

// the last frame log as the resynthesiser takes it (lane_feed.hpp): lane l's first entry is column done[l] + 1 - count[l]
MosaickerLog mosaicker_log(const ssym_mosaicker *mk)
{
    return MosaickerLog{mk->ctx, mk->nLanes, &mk->log, &mk->done, mk->calls};
}

}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_mosaicker_create(ssym_ctx *ctx, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty, double gap_cost,
                              ssym_mosaicker **out)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return mosaicker_create(ctx, dict, n_lanes, piece_penalty, gap_cost, out); });
}

int32_t ssym_mosaicker_destroy(ssym_ctx *ctx, ssym_mosaicker *mk)
{
    return lane_destroy(ctx, mk, mosaicker_free);
}

int32_t ssym_mosaicker_push(ssym_ctx *ctx, ssym_mosaicker *mk, const double *feats, const uint64_t *frame_offsets, uint32_t flags,
                            uint64_t *out_n_frames)
{
    return lane_push(ctx, mk, kNoun, "ssym_mosaicker_push", mosaicker_feed, feats, frame_offsets, out_n_frames,
                     mosaicker_run(ctx, mk, out_n_frames));
}

int32_t ssym_mosaicker_follow(ssym_ctx *ctx, ssym_mosaicker *mk, const ssym_stream *stream, uint32_t flags, uint64_t *out_n_frames)
{
    return lane_follow(ctx, mk, kNoun, "ssym_mosaicker_follow", mosaicker_feed, stream, out_n_frames,
                       mosaicker_run(ctx, mk, out_n_frames));
}

int32_t ssym_mosaicker_frames(ssym_ctx *ctx, const ssym_mosaicker *mk, uint32_t *out_lane, uint32_t *out_column, uint32_t *out_src,
                              uint32_t *out_frame, double *out_cost, uint32_t *out_start, uint32_t flags)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        return mosaicker_frames(ctx, mk, out_lane, out_column, out_src, out_frame, out_cost, out_start, flags);
    });
}

int32_t ssym_mosaicker_flush(ssym_ctx *ctx, ssym_mosaicker *mk, uint32_t lane, uint64_t *out_n_frames)
{
    return lane_flush(ctx, mk, kNoun, "ssym_mosaicker_flush", mosaicker_feed, lane, out_n_frames, mosaicker_run(ctx, mk, out_n_frames));
}

int32_t ssym_mosaicker_best(ssym_ctx *ctx, const ssym_mosaicker *mk, double *out_total, uint32_t *out_covered,
                            uint32_t *out_committed, uint32_t flags)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return mosaicker_best(ctx, mk, out_total, out_covered, out_committed, flags); });
}

int32_t ssym_mosaicker_counts(const ssym_mosaicker *mk, uint64_t *out_frames, uint64_t *out_capacity)
{
    if (!mk)
        return SSYM_E_INVALID;
    if (out_frames)
        std::copy(mk->consumed.begin(), mk->consumed.end(), out_frames);
    if (out_capacity)
        *out_capacity = mk->cap;
    return SSYM_OK;
}

int32_t ssym_mosaicker_reset(ssym_ctx *ctx, ssym_mosaicker *mk, uint32_t lane)
{
    return lane_reset(ctx, mk, kNoun, "ssym_mosaicker_reset", mosaicker_feed, lane, [&]() -> int32_t {
        mosaicker_init_kernel<<<1, 256, 0, ctx->stream>>>(mk->lanes, lane, 1u);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        mk->consumed[lane] = 0;
        mk->done[lane] = -1;
        mk->stored[lane] = 0;
        mk->ended[lane] = mk->dead[lane] = 0;
        return SSYM_OK;
    });
}

}  // extern "C"
