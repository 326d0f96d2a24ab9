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
//   forward   mosaicker_forward_kernel, one workgroup per lane with new frames, the column loop of mosaic_forward_kernel:
//             the same operations in the same order.  E / N of column j sit in the lane's slab at parity j & 1 (4 G doubles
//             per lane), so column n-1 is where a push finds it; best(n-1) comes from the lane's record.  Direction bytes,
//             arg(j) and the target frame (the emission's frame cost needs it) go into the lane's ring, column j at
//             j mod cap.  The loop stops at the first column whose best is not finite: the slab of column lastFinite stays.
//   commit    mosaicker_commit_kernel, one workgroup per lane.  The live keys of column lastFinite are collected into a
//             list; each step maps the list one column back through the ring into a second list, a key going in only if it
//             is the first to raise its flag (duplicates drop as walks merge; the flags are lowered again before the next
//             step).  It stops when one key is left (at once when the keys already agree) or at column done + 1.  Thread 0
//             then walks from that key down to done + 1 as mosaic_backtrace_kernel's thread 0 does, leaving g | start bit
//             or GAP in the arg ring, and all threads fill the call's frame log in ascending column with plain stores.
//             A flush is the same emission from arg(lastFinite).
//   regrow    mosaicker_regrow_kernel moves the uncommitted columns when the ring doubles.
// No workgroup waits on another: no spin wait; stream order is the only ordering between kernels.
#include "dtw_mosaic_common.hpp"
#include "lane_feed.hpp"

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

struct ssym_mosaicker {
    ssym_ctx *ctx = nullptr;
    const ssym_dict *dict = nullptr;
    uint32_t nLanes = 0, dim = 0, G = 0;
    uint32_t dictN = 0;                      // the dictionary as it was at creation
    uint64_t dictFrames = 0;
    double penalty = 0.0, gapCost = 0.0;     // gapCost +inf: no gaps
    uint64_t budget = 0;                     // bytes the object may own
    uint64_t fixedBytes = 0;                 // what it owns beside the ring
    // host mirrors of the lanes
    std::vector<uint64_t> consumed;
    std::vector<int64_t> done, stored;
    std::vector<uint8_t> ended, dead;
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
    // the frame log: the frames of the last push / follow / flush, lane l's from logOff[l] on
    double *logCost = nullptr;               // [logCap]
    uint32_t *logWords = nullptr;            // [5][logCap]: lane, column, src, frame, start
    uint64_t logCap = 0;
    std::vector<uint64_t> logOff, logCount;
};

namespace ssym {
namespace {

constexpr uint32_t kNone = kCoverNone, kGap = kCoverGap;

__global__ __launch_bounds__(256) void mosaicker_init_kernel(MosLane *lanes, uint32_t lane0, uint32_t nLanes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nLanes)
        lanes[lane0 + i] = MosLane{0, 0, -1, -1, 0, 0.0, 0.0};
}

struct MosForwardArgs {
    const MosStep *steps;
    MosLane *lanes;
    uint32_t G, dim;
    int squared;
    double penalty, gapCost;
    const uint8_t *posc;
    const double *srcT;
    double *slab;
    uint64_t cap;
    uint8_t *dir;
    uint32_t *arg;
    double *frames;
};

__global__ __launch_bounds__(kMosaicThreads) void mosaicker_forward_kernel(const MosForwardArgs a)
{
    __shared__ double ring[2][kMosaicMaxDim];                // target frames j and j + 1
    __shared__ double partV[2][kMosaicMaxWaves];
    __shared__ uint32_t partG[2][kMosaicMaxWaves];
    const double INF = __builtin_inf();
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, nWaves = nthr >> 6;
    const uint32_t G = a.G, dim = a.dim, l = blockIdx.x;
    const MosStep s = a.steps[l];
    if (s.m == 0)
        return;
    const MosLane st = a.lanes[l];
    if (st.n > 0 && !(st.best < INF)) {                      // dead: the frames are counted, nothing else
        if (tid == 0)
            a.lanes[l].n = st.n + s.m;
        return;
    }
    double *slab = a.slab + (size_t)l * 4 * G;
    const uint64_t mask = a.cap - 1;
    uint32_t *path = a.arg + (size_t)l * a.cap;
    uint8_t *dir = a.dir + (size_t)l * a.cap * G;
    double *kept = a.frames + (size_t)l * a.cap * dim;
    const double *b0 = s.rows;
    const uint64_t n = (uint64_t)st.n;
    if (n == 0)                                              // column -1: nothing to continue and nothing to repeat
        for (uint32_t g = tid; g < G; g += nthr) {
            slab[(size_t)2 * G + g] = INF;
            slab[(size_t)3 * G + g] = INF;
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
        const uint32_t par = (uint32_t)j & 1;
        const double S = __dadd_rn(a.penalty, best);
        const double *Eo = slab + (size_t)(par ^ 1) * 2 * G, *No = Eo + G;
        double *En = slab + (size_t)par * 2 * G, *Nn = En + G;
        uint8_t *dcol = dir + (j & mask) * G;
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
            if (eD < bv) {                                   // g ascends within a thread: the first minimum stays
                bv = eD;
                bg = g;
            }
        }
        if (j + 1 < end)
            for (uint32_t e = tid; e < dim; e += nthr) {
                const double v = b0[(j + 1 - n) * dim + e];
                ring[par ^ 1][e] = v;
                kept[((j + 1) & mask) * dim + e] = v;
            }
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
            path[j & mask] = arg;
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

struct MosCommitArgs {
    const MosStep *steps;
    MosLane *lanes;
    uint32_t G, dim;
    int squared;
    double penalty, gapCost;
    const double *srcRaw;
    const uint64_t *srcOff;
    uint32_t nSrc;
    const double *slab;
    uint32_t *keys;
    uint64_t cap;
    const uint8_t *dir;
    uint32_t *arg;
    const double *frames;
    uint32_t *logLane, *logColumn, *logSrc, *logFrame, *logStart;
    double *logCost;
};

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
    const uint32_t G = a.G, dim = a.dim;
    const uint64_t mask = a.cap - 1;
    const uint8_t *dir = a.dir + (size_t)l * a.cap * G;
    uint32_t *path = a.arg + (size_t)l * a.cap;
    const double *kept = a.frames + (size_t)l * a.cap * dim;
    const size_t K = 2 * (size_t)G + 2;
    uint32_t *lists = a.keys + (size_t)l * 3 * K, *flag = lists + 2 * K;
    const long long done = st.done, top = st.lastFinite;
    // a key: g << 1 | (1: state H), or GAP.  Whatever the ring holds, a key's g stays below G.
    auto key_e = [&](uint32_t g, long long j) -> uint32_t {
        return g >= G ? kGap : g << 1 | (dir[((uint64_t)j & mask) * G + g] & 1u);
    };
    // the key at column j - 1 of the walk that holds `key` at column j (j - 1 > done: its column is in the ring)
    auto back = [&](uint32_t key, long long j) -> uint32_t {
        if (key == kGap)
            return key_e(path[(uint64_t)(j - 1) & mask], j - 1);
        const uint32_t g = key >> 1;
        if (key & 1)
            return g << 1;
        const uint32_t code = dir[((uint64_t)j & mask) * G + g] >> 1;
        if (code >= 2)
            return key_e(path[(uint64_t)(j - 1) & mask], j - 1);
        return key_e(g > code ? g - 1 - code : 0, j - 1);
    };
    auto slot = [&](uint32_t key) -> size_t { return key == kGap ? 2 * (size_t)G : key; };

    long long c = done;                                      // the last column that is final
    uint32_t tip = kGap;                                     // the key at it
    if (top > done) {
        if (s.flush) {
            c = top;
            tip = key_e(path[(uint64_t)top & mask], top);
        } else {
            // live(lastFinite + 1): for a lane that lives lastFinite = n - 1; for one that died the last commit there was
            if (tid == 0)
                shN[0] = shN[1] = 0;
            __syncthreads();
            const double S = __dadd_rn(a.penalty, st.bestFinite);
            const double *E = a.slab + (size_t)l * 4 * G + (size_t)((uint64_t)top & 1) * 2 * G, *N = E + G;
            const uint8_t *dcol = dir + ((uint64_t)top & mask) * G;
            for (uint32_t g = tid; g < G; g += nthr) {
                const uint32_t d = dcol[g];
                const double e = E[g];
                if (e > -INF && e <= S)
                    lists[atomicAdd(&shN[0], 1u)] = g << 1 | (d & 1u);
                if (d & 1u) {
                    const double nn = N[g];
                    if (nn > -INF && nn <= S)
                        lists[atomicAdd(&shN[0], 1u)] = g << 1;
                }
            }
            if (tid == 0 && path[(uint64_t)top & mask] == kGap)
                lists[atomicAdd(&shN[0], 1u)] = kGap;
            __syncthreads();
            uint32_t cur = 0;
            long long col = top;
            uint32_t cnt = shN[0];
            while (cnt > 1 && col > done + 1) {
                const uint32_t *from = lists + cur * K;
                uint32_t *to = lists + (cur ^ 1) * K;
                for (uint32_t i = tid; i < cnt; i += nthr) {
                    const uint32_t nk = back(from[i], col);
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
        uint32_t key = tip;
        for (long long col = c; col > done; --col) {
            uint32_t word = kGap;
            if (key != kGap) {
                const uint32_t g = key >> 1;
                const bool start = !(key & 1) && ((dir[((uint64_t)col & mask) * G + g] >> 1) >= 2 || col == 0);
                word = g | (start ? kMosaicStart : 0u);
            }
            const uint32_t next = col - 1 > done ? back(key, col) : kGap;
            path[(uint64_t)col & mask] = word;
            key = next;
        }
        a.lanes[l].done = c;
        a.lanes[l].count = (unsigned long long)(c - done);
        shC = c;
    }
    __syncthreads();
    c = shC;
    for (long long f = done + 1 + tid; f <= c; f += nthr) {
        const uint32_t p = path[(uint64_t)f & mask];
        uint32_t src = kGap, frame = kNone;
        double cost = a.gapCost;
        if (p != kGap) {
            const uint32_t g = min(p & ~kMosaicStart, G - 1);
            src = mosaic_segment(a.srcOff, a.nSrc, g);
            frame = (uint32_t)(g - a.srcOff[src]);
            cost = mosaic_cost(a.srcRaw + (size_t)g * dim, 1, kept + ((uint64_t)f & mask) * dim, dim, a.squared);
        }
        const uint64_t k = s.logAt + (uint64_t)(f - done - 1);
        a.logLane[k] = l;
        a.logColumn[k] = (uint32_t)f;
        a.logSrc[k] = src;
        a.logFrame[k] = frame;
        a.logStart[k] = (p & kMosaicStart) ? 1u : 0u;        // GAP has the bit as well
        a.logCost[k] = cost;
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
                    (void *)mk->dir, (void *)mk->arg, (void *)mk->frames, (void *)mk->logCost, (void *)mk->logWords})
        if (p)
            dev_free(ctx, p);
    delete mk;
}

constexpr const char *kNoun = "mosaicker";

// what a call that reads the dictionary refuses
int32_t check_dict(ssym_ctx *ctx, const ssym_mosaicker *mk, const char *fn)
{
    if (mk->dict->set.n != mk->dictN || mk->dict->set.total_frames != mk->dictFrames) {
        ctx->err = std::string(fn) + ": the dictionary was appended to after the mosaicker was created; create a new mosaicker";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

// the mosaicker as the lane feed (lane_feed.hpp) sees it: a flushed lane has ended, and push and follow read the dictionary
LaneFeed feed_of(ssym_ctx *ctx, const ssym_mosaicker *mk)
{
    return LaneFeed{kNoun, "out_n_frames", mk->nLanes, mk->dim, mk->consumed, &mk->ended, true,
                    [ctx, mk](const char *fn) { return check_dict(ctx, mk, fn); }};
}

uint64_t pow2_at_least(uint64_t x)
{
    uint64_t p = 1;
    while (p < x)
        p <<= 1;
    return p;
}

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
    if (rc != SSYM_OK) {
        for (void *p : {(void *)dir, (void *)arg, (void *)frames})
            if (p)
                dev_free(ctx, p);
        return rc;
    }
    if (mk->cap) {
        mosaicker_regrow_kernel<<<dim3(16, mk->nLanes), 256, 0, ctx->stream>>>(mk->lanes, mk->G, mk->dim, mk->cap, cap, mk->dir, mk->arg,
                                                                               mk->frames, dir, arg, frames);
        const hipError_t e = hipGetLastError();
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);         // the old ring is freed below
        if (e != hipSuccess || e2 != hipSuccess) {
            ctx->err = std::string("mosaicker: ") + hipGetErrorString(e != hipSuccess ? e : e2);
            for (void *p : {(void *)dir, (void *)arg, (void *)frames})
                dev_free(ctx, p);
            return SSYM_E_HIP;
        }
        for (void *p : {(void *)mk->dir, (void *)mk->arg, (void *)mk->frames})
            dev_free(ctx, p);
    }
    mk->dir = dir;
    mk->arg = arg;
    mk->frames = frames;
    mk->cap = cap;
    return SSYM_OK;
}

// room for `need` frames in the log; what it held is dropped (a call's log starts empty)
int32_t log_room(ssym_ctx *ctx, ssym_mosaicker *mk, uint64_t need)
{
    if (need <= mk->logCap)
        return SSYM_OK;
    const uint64_t cap = pow2_at_least(std::max<uint64_t>(need, 256));
    double *cost = nullptr;
    uint32_t *words = nullptr;
    int32_t rc = alloc_n(ctx, &cost, (size_t)cap);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &words, 5 * (size_t)cap);
    if (rc != SSYM_OK) {
        if (cost)
            dev_free(ctx, cost);
        return rc;
    }
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (void *p : {(void *)mk->logCost, (void *)mk->logWords})
        if (p)
            dev_free(ctx, p);
    mk->logCost = cost;
    mk->logWords = words;
    mk->logCap = cap;
    return SSYM_OK;
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
    if (!out) {
        ctx->err = std::string(fn) + ": out is NULL";
        return SSYM_E_INVALID;
    }
    *out = nullptr;
    int32_t rc = check_cover_ctx(ctx, fn);
    if (rc != SSYM_OK)
        return rc;
    if (!dict || n_lanes == 0) {
        ctx->err = std::string(fn) + ": the dictionary handle is NULL or n_lanes is 0";
        return SSYM_E_INVALID;
    }
    rc = check_cover_prices(ctx, fn, piece_penalty, gap_cost);
    if (rc != SSYM_OK)
        return rc;
    const SegmentSet &src = dict->set;
    if (src.n == 0) {
        ctx->err = std::string(fn) + ": empty dictionary";
        return SSYM_E_EMPTY_DICT;
    }
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
    mk->ctx = ctx;
    mk->dict = dict;
    mk->nLanes = n_lanes;
    mk->dim = src.dim;
    mk->G = (uint32_t)G;
    mk->dictN = src.n;
    mk->dictFrames = src.total_frames;
    mk->penalty = piece_penalty;
    mk->gapCost = gap_cost;
    mk->budget = budget;
    mk->fixedBytes = fixed;
    mk->consumed.assign(n_lanes, 0);
    mk->done.assign(n_lanes, -1);
    mk->stored.assign(n_lanes, 0);
    mk->ended.assign(n_lanes, 0);
    mk->dead.assign(n_lanes, 0);
    mk->logOff.assign((size_t)n_lanes + 1, 0);
    mk->logCount.assign(n_lanes, 0);
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

// The body of push, follow and flush.  rows[l]: lane l's m[l] new frames (DEVICE); flushLane: the lane to flush, or kCoverNone.
// The frames go through in slices of at most `slice` per lane, with a commit after each; the host reads the lanes' records
// back after every slice, which is also the call's synchronisation.
int32_t mosaicker_run(ssym_ctx *ctx, ssym_mosaicker *mk, const char *fn, const std::vector<const double *> &rows,
                      const std::vector<uint64_t> &m, uint32_t flushLane, uint64_t *out_n_frames)
{
    const uint32_t nL = mk->nLanes, dim = mk->dim;
    const SegmentSet &src = mk->dict->set;
    hipStream_t st = ctx->stream;
    ssym_timings tm{};
    const uint64_t sliceMax = std::max<uint64_t>(knob_u64("SSYM_MOSAICKER_SLICE", kLaneMaxFrames), 1);
    // the most columns a ring may grow to within the budget (a power of two): while it doubles, the ring it leaves (half of
    // it at most) exists beside it
    uint64_t capMax = kMosaickerRingMin;
    while ((uint64_t)nL * (capMax * 3) * column_bytes(mk->G, dim) <= mk->budget - mk->fixedBytes)
        capMax *= 2;
    capMax = std::max(capMax, mk->cap);
    // the log: a lane emits no more frames than it has beyond done
    uint64_t room = 0, total = 0;
    for (uint32_t l = 0; l < nL; ++l) {
        mk->logOff[l] = room;
        mk->logCount[l] = 0;
        if (m[l] || l == flushLane)
            room += mk->consumed[l] + m[l] - (uint64_t)(mk->done[l] + 1);
        total += m[l];
    }
    mk->logOff[nL] = room;
    tm.n_pairs = (uint64_t)mk->G * total;                     // cells
    int32_t rc = log_room(ctx, mk, room);
    if (rc != SSYM_OK)
        return rc;
    std::vector<uint64_t> at(nL, 0);
    std::vector<MosStep> steps(nL);
    std::vector<MosLane> state(nL);
    hipEvent_t *ev = ctx->ev;
    const bool flush = flushLane != kCoverNone;
    int32_t result = SSYM_OK;
    for (;;) {
        // the slice: what the ring takes beside the longest uncommitted stretch of a lane that still has frames
        uint64_t left = 0, pending = 0;
        for (uint32_t l = 0; l < nL; ++l)
            if (m[l] > at[l]) {
                left += m[l] - at[l];
                if (!mk->dead[l])
                    pending = std::max(pending, (uint64_t)(mk->stored[l] - (mk->done[l] + 1)));
            }
        if (left == 0 && !flush)
            break;
        uint64_t slice = sliceMax;
        if (left) {
            if (pending >= capMax) {
                ctx->err = std::string(fn) + ": the uncommitted columns of a lane fill the " + std::to_string(mk->budget >> 20) +
                           " MiB the mosaicker may own (" + std::to_string(pending) + " columns of " +
                           std::to_string(column_bytes(mk->G, dim)) + " bytes on " + std::to_string(nL) +
                           " lanes); flush the lane (ssym_mosaicker_flush) and reset it";
                result = SSYM_E_UNSUPPORTED;
                break;
            }
            slice = std::min(slice, capMax - pending);
        }
        uint64_t need = 0;
        for (uint32_t l = 0; l < nL; ++l) {
            const uint64_t ml = std::min(slice, m[l] - at[l]);
            MosStep &s = steps[l];
            s.rows = ml ? rows[l] + at[l] * dim : nullptr;
            s.logAt = mk->logOff[l] + mk->logCount[l];
            s.m = (uint32_t)ml;
            s.flush = flush && l == flushLane;
            if (ml && !mk->dead[l])
                need = std::max(need, (uint64_t)(mk->stored[l] - (mk->done[l] + 1)) + ml);
        }
        // the slice's device work; a failure leaves through the epilogue below, which reports what earlier slices logged
        rc = [&]() -> int32_t {
            if (need > mk->cap) {
                const int32_t grown = ring_store(ctx, mk, pow2_at_least(need));
                if (grown != SSYM_OK)
                    return grown;
            }
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(mk->dSteps, steps.data(), sizeof(MosStep) * nL, hipMemcpyHostToDevice, st));
            SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
            if (left) {
                MosForwardArgs f{};
                f.steps = mk->dSteps;
                f.lanes = mk->lanes;
                f.G = mk->G;
                f.dim = dim;
                f.squared = ctx->squared;
                f.penalty = mk->penalty;
                f.gapCost = mk->gapCost;
                f.posc = mk->posc;
                f.srcT = mk->srcT;
                f.slab = mk->slab;
                f.cap = mk->cap;
                f.dir = mk->dir;
                f.arg = mk->arg;
                f.frames = mk->frames;
                mosaicker_forward_kernel<<<nL, kMosaicThreads, 0, st>>>(f);
                SSYM_HIP_CHECK(ctx, hipGetLastError());
            }
            SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
            MosCommitArgs k{};
            k.steps = mk->dSteps;
            k.lanes = mk->lanes;
            k.G = mk->G;
            k.dim = dim;
            k.squared = ctx->squared;
            k.penalty = mk->penalty;
            k.gapCost = mk->gapCost;
            k.srcRaw = src.raw;
            k.srcOff = src.off;
            k.nSrc = src.n;
            k.slab = mk->slab;
            k.keys = mk->keys;
            k.cap = mk->cap;
            k.dir = mk->dir;
            k.arg = mk->arg;
            k.frames = mk->frames;
            k.logLane = mk->logWords;
            k.logColumn = mk->logWords + mk->logCap;
            k.logSrc = mk->logWords + 2 * mk->logCap;
            k.logFrame = mk->logWords + 3 * mk->logCap;
            k.logStart = mk->logWords + 4 * mk->logCap;
            k.logCost = mk->logCost;
            mosaicker_commit_kernel<<<nL, kMosaicThreads, 0, st>>>(k);
            SSYM_HIP_CHECK(ctx, hipGetLastError());
            SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(state.data(), mk->lanes, sizeof(MosLane) * nL, hipMemcpyDeviceToHost, st));
            SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
            return SSYM_OK;
        }();
        if (rc != SSYM_OK) {
            result = rc;
            break;
        }
        for (uint32_t l = 0; l < nL; ++l) {
            if (steps[l].m == 0 && !steps[l].flush)
                continue;
            mk->consumed[l] = (uint64_t)state[l].n;
            mk->done[l] = state[l].done;
            mk->stored[l] = state[l].stored;
            mk->dead[l] = state[l].n > 0 && !(state[l].best < __builtin_inf());
            mk->logCount[l] += state[l].count;
            at[l] += steps[l].m;
        }
        tm.main_ms += ev_ms(ev[0], ev[1]);
        tm.reduce_ms += ev_ms(ev[1], ev[2]);
        tm.total_ms += ev_ms(ev[0], ev[2]);
        tm.main_launches += left ? 1 : 0;
        if (flush)
            break;
    }
    if (flush && result == SSYM_OK)
        mk->ended[flushLane] = 1;
    uint64_t frames = 0;
    for (uint32_t l = 0; l < nL; ++l)
        frames += mk->logCount[l];
    *out_n_frames = frames;
    ctx->timings = tm;
    return result;
}

int32_t mosaicker_push(ssym_ctx *ctx, ssym_mosaicker *mk, const double *feats, const uint64_t *frame_offsets, uint32_t flags,
                       uint64_t *out_n_frames)
{
    const char *fn = "ssym_mosaicker_push";
    Blocks bl(ctx);
    std::vector<const double *> rows;
    std::vector<uint64_t> m;
    int32_t rc = check_handle(ctx, mk, kNoun, fn);
    if (rc == SSYM_OK)
        rc = feed_of(ctx, mk).push(ctx, fn, feats, frame_offsets, out_n_frames, bl, rows, m);
    if (rc != SSYM_OK)
        return rc;
    return mosaicker_run(ctx, mk, fn, rows, m, kCoverNone, out_n_frames);
}

int32_t mosaicker_follow(ssym_ctx *ctx, ssym_mosaicker *mk, const ssym_stream *stream, uint32_t flags, uint64_t *out_n_frames)
{
    const char *fn = "ssym_mosaicker_follow";
    std::vector<const double *> rows;
    std::vector<uint64_t> m;
    int32_t rc = check_handle(ctx, mk, kNoun, fn);
    if (rc == SSYM_OK)
        rc = feed_of(ctx, mk).follow(ctx, fn, stream, out_n_frames, rows, m);
    if (rc != SSYM_OK)
        return rc;
    return mosaicker_run(ctx, mk, fn, rows, m, kCoverNone, out_n_frames);
}

int32_t mosaicker_flush(ssym_ctx *ctx, ssym_mosaicker *mk, uint32_t lane, uint64_t *out_n_frames)
{
    const char *fn = "ssym_mosaicker_flush";
    int32_t rc = check_handle(ctx, mk, kNoun, fn);
    if (rc == SSYM_OK)
        rc = feed_of(ctx, mk).lane(ctx, fn, lane, true, out_n_frames);
    if (rc != SSYM_OK)
        return rc;
    const std::vector<const double *> rows(mk->nLanes, nullptr);
    const std::vector<uint64_t> m(mk->nLanes, 0);
    return mosaicker_run(ctx, mk, fn, rows, m, lane, out_n_frames);
}

int32_t mosaicker_reset(ssym_ctx *ctx, ssym_mosaicker *mk, uint32_t lane)
{
    const char *fn = "ssym_mosaicker_reset";
    int32_t rc = check_handle(ctx, mk, kNoun, fn);
    if (rc == SSYM_OK)
        rc = feed_of(ctx, mk).lane(ctx, fn, lane, false, nullptr);
    if (rc != SSYM_OK)
        return rc;
    mosaicker_init_kernel<<<1, 256, 0, ctx->stream>>>(mk->lanes, lane, 1u);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    mk->consumed[lane] = 0;
    mk->done[lane] = -1;
    mk->stored[lane] = 0;
    mk->ended[lane] = mk->dead[lane] = 0;
    return SSYM_OK;
}

int32_t mosaicker_frames(ssym_ctx *ctx, const ssym_mosaicker *mk, uint32_t *out_lane, uint32_t *out_column, uint32_t *out_src,
                         uint32_t *out_frame, double *out_cost, uint32_t *out_start, uint32_t flags)
{
    int32_t rc = check_handle(ctx, mk, kNoun, "ssym_mosaicker_frames");
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;
    const size_t cap = mk->logCap;
    uint32_t *const outs[5] = {out_lane, out_column, out_src, out_frame, out_start};
    size_t to = 0;
    bool any = false;
    for (uint32_t l = 0; l < mk->nLanes; ++l) {          // the lanes' stretches of the log, one behind the other
        const size_t from = mk->logOff[l], n = mk->logCount[l];
        if (n == 0)
            continue;
        any = true;
        rc = copy_out(ctx, out_cost ? out_cost + to : nullptr, (const double *)mk->logCost + from, n, outDev);
        for (int w = 0; w < 5 && rc == SSYM_OK; ++w)
            rc = copy_out(ctx, outs[w] ? outs[w] + to : nullptr, (const uint32_t *)mk->logWords + w * cap + from, n, outDev);
        if (rc != SSYM_OK)
            return rc;
        to += n;
    }
    if (any)
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
}

int32_t mosaicker_best(ssym_ctx *ctx, const ssym_mosaicker *mk, double *out_total, uint32_t *out_covered, uint32_t *out_committed,
                       uint32_t flags)
{
    int32_t rc = check_handle(ctx, mk, kNoun, "ssym_mosaicker_best");
    if (rc != SSYM_OK)
        return rc;
    if (!out_total && !out_covered && !out_committed)
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t nL = mk->nLanes;
    const unsigned grid = (nL + 255) / 256;
    if (flags & SSYM_OUT_DEVICE) {
        mosaicker_best_kernel<<<grid, 256, 0, ctx->stream>>>(mk->lanes, nL, out_total, out_covered, out_committed);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return SSYM_OK;
    }
    Blocks bl(ctx);
    double *dTotal = nullptr;
    uint32_t *dWords = nullptr;
    rc = bl.get(&dTotal, (size_t)nL);
    if (rc == SSYM_OK)
        rc = bl.get(&dWords, 2 * (size_t)nL);
    if (rc != SSYM_OK)
        return rc;
    mosaicker_best_kernel<<<grid, 256, 0, ctx->stream>>>(mk->lanes, nL, dTotal, dWords, dWords + nL);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    rc = copy_out(ctx, out_total, (const double *)dTotal, nL, false);
    if (rc == SSYM_OK)
        rc = copy_out(ctx, out_covered, (const uint32_t *)dWords, nL, false);
    if (rc == SSYM_OK)
        rc = copy_out(ctx, out_committed, (const uint32_t *)dWords + nL, nL, false);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
}

}  // namespace
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
    if (!mk)
        return SSYM_OK;
    if (!ctx || mk->ctx != ctx)
        return SSYM_E_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    mosaicker_free(ctx, mk);
    return SSYM_OK;
}

int32_t ssym_mosaicker_push(ssym_ctx *ctx, ssym_mosaicker *mk, const double *feats, const uint64_t *frame_offsets, uint32_t flags,
                            uint64_t *out_n_frames)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return mosaicker_push(ctx, mk, feats, frame_offsets, flags, out_n_frames); });
}

int32_t ssym_mosaicker_follow(ssym_ctx *ctx, ssym_mosaicker *mk, const ssym_stream *stream, uint32_t flags, uint64_t *out_n_frames)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return mosaicker_follow(ctx, mk, stream, flags, out_n_frames); });
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
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return mosaicker_flush(ctx, mk, lane, out_n_frames); });
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
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return mosaicker_reset(ctx, mk, lane); });
}

}  // extern "C"
