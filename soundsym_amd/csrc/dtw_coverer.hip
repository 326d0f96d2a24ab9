// dtw_coverer.hip -- the live cover: growing targets tiled by the segments of one resident dictionary, every piece reported
// by the push after which no longer recording could change it (DESIGN.md 2 "Live cover", 5.24).
//
// Role on the path: ssym_dtw_cover needs its whole target up front.  A coverer is its resumable form, lane by lane, as a
// spotter is ssym_dtw_spot's: the frames arrive in pushes (or are followed in a stream's resident analysis), and what the
// coverer emits is, piece for piece and bit for bit, a prefix of what ssym_dtw_cover gives for the whole.
//
// Definition.  c, w, M, src, best, the tie rules and the arithmetic are those of "Cover" (dtw_cover.hip), word for word.
// For one lane, X is everything consumed so far, n its frame count, W = 2 max(Fmax, 1) with Fmax the dictionary's longest
// segment at creation.
//   resume   : the lane holds n, its last W-1 frames, best(e) for the last W ends (the chain kernel's ring), the back-pointers
//              (L, src, M) of every frame after the committed end, done (the last committed end, -1 at first) and lastFinite
//              (the largest e with a finite best(e), -1 at first: best(-1) = 0).
//              Consuming frames n ... n+m-1 computes M(s,L) for every window that ends in them (s >= n-W+1) and best(e) and
//              the back-pointers for e = n ... n+m-1, exactly as "Cover" does.
//   horizon  : H(n) = { e : max(-1, n-W) <= e <= n-1, best(e) finite }   (-1 belongs to it while n < W)
//   walk(e)  : the pieces the back-pointers give from e down to -1, in ascending start   (walk(-1) is empty)
//   commit   : C(n) = the longest common prefix of walk(e) over e in H(n); H(n) empty: nothing new.
//              A push emits the pieces of C(n) not emitted before, and done = the end of the last of them.
//   flush    : emits the pieces of walk(lastFinite) not emitted before.  The lane has then ENDED: it consumes nothing more
//              until ssym_coverer_reset (push with frames for it: SSYM_E_INVALID; follow skips it).
//   best     : total = best(n-1) (+inf for n = 0 or when not finite), covered = lastFinite + 1, committed = done + 1
// Every piece has at most W frames, so a piece that ends at n or later starts after n-W: whatever a longer recording brings
// continues one of the walks of H(n), and what those walks share is final.
//
// Mapping.
//   gather    coverer_gather_kernel builds the call's frame buffer [lane][tail | new] from the lanes' stored tails and the new
//             frames (uploaded once by push, read in the stream's store by follow); coverer_tail_kernel then stores the new
//             tails.  A lane without new frames has no frames in the buffer.
//   forward   cover_forward (dtw_cover.hip): cover_forward_kernel and cover_fold_kernel on the buffer, one "target" per lane,
//             with the geometry of ssym_dtw_cover.  Starts in the tail are recomputed from column 0: keeping E / N per
//             (source, start) would cost N x W x Fa x 16 bytes per lane.
//   chain     coverer_chain_kernel: one wave per lane.  The ring is loaded into LDS, cover_chain_step (dtw_cover_chain.hpp,
//             the body cover_chain_kernel runs) gives best(e) and the back-pointer of every new end, lane 0 writes them into
//             the lane's ring store of back-pointers, and the ring goes back to memory.
//   commit    coverer_commit_kernel: one wave per lane.  The up to W ends of H(n) are spread over the wave's lanes; a lane
//             first brings its own ends to their common ancestor, then every lane steps back while it is above the wave-wide
//             minimum, until all positions are equal.  Lane 0 counts the pieces from there down to done and writes them into
//             the call's piece log in ascending start, with plain stores.  A flush is the same emission from lastFinite.
// No kernel waits on another workgroup, none spins: stream order is the only ordering between them.
// Host: the checks, the upload and the bodies of push / follow / flush / reset are lane_feed.hpp's, and so is the piece log
// (LaneLog).  What the coverer shares with the mosaicker is lane_tiling.hpp's: the base of the handle, the dictionary check,
// the first refusals of create, best's host body, the hand-over of a grown back-pointer store, and the loop over a call's
// slices (tiling_run): gather and forward between its first two events, chain and commit between the last two.  A slice
// that fails leaves through that loop's epilogue.  The slice's plan, frame buffer and bufOff are here (CovererSlices).
//
// Gaps (ssym_coverer_create_gaps).  The chain's step takes the gap candidate of "Cover with gaps": a frame left uncovered is a
// piece of one frame with the source SSYM_COVER_GAP and the cost gap_cost.  1 <= W, so the horizon argument holds as it
// stands, and commit, flush and emission walk gap frames like any other piece.  With a finite gap_cost every best(e) is
// finite: lastFinite = n - 1, H(n) is never empty, and a NaN or +-inf frame is a gap frame the lane goes on past.
#include "dtw_wave.hpp"
#include "dtw_cover_chain.hpp"
#include "lane_feed.hpp"
#include "lane_tiling.hpp"

#include <algorithm>

namespace ssym {

// (the frames a lane may consume: lane_feed.hpp's kLaneMaxFrames -- a lane's ends and cut points are reported as u32)
constexpr uint32_t kCovererMaxLanes = 65535;                      // one grid row per lane
constexpr uint64_t kCovererBackMin = 1024;                       // frames of the back-pointer store, a power of two

// a lane's state on the device
struct CovLane {
    long long n;                 // frames consumed
    long long done;              // the last committed end, -1 at first
    long long lastFinite;        // the largest e with a finite best(e), -1 at first
    unsigned long long count;    // pieces the last commit or flush wrote into the log
};

// what one slice of a call does with a lane
struct CovStep {
    const double *rows;          // the new frames (DEVICE), m x dim
    uint64_t logAt;              // where the lane's next piece goes in the log
    uint32_t m;                  // new frames
    uint32_t tail;               // min(n, W - 1): frames of the stored tail in front of them
    uint32_t flush;              // 1: emit walk(lastFinite)
    uint32_t pad;
};

}  // namespace ssym

// beside what every live tiling holds (lane_tiling.hpp; gapCost is +inf from ssym_coverer_create, and the words of the log,
// the pieces of the last push / follow / flush, are lane, src, start, end)
struct ssym_coverer : ssym::LaneTiling {
    ssym_coverer() : LaneTiling(4) {}
    uint32_t width = 0, ring = 0;
    uint64_t sliceMax = 0;                   // frames per lane and slice the scratch allows
    std::vector<int64_t> lastFinite;         // host mirror of the lanes'
    // device
    double *tail = nullptr;                  // [nLanes][W - 1][dim]: the last min(n, W - 1) frames, oldest first
    double *ringD = nullptr;                 // [nLanes][ring]: best(e) at (e + 1) mod ring
    ssym::CovLane *lanes = nullptr;          // [nLanes]
    ssym::CovStep *dSteps = nullptr;         // [nLanes]
    uint64_t *dBufOff = nullptr;             // [nLanes + 1]
    uint64_t backCap = 0;                    // frames per lane of the back-pointer store
    double *bpCost = nullptr;                // [nLanes][backCap], frame e at e mod backCap
    uint32_t *bpLen = nullptr, *bpSrc = nullptr;
};

namespace ssym {
namespace {

__global__ __launch_bounds__(256) void coverer_init_kernel(CovLane *lanes, double *ringD, uint32_t ring, uint32_t lane0, uint32_t nLanes)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nLanes * ring)
        return;
    const uint32_t l = lane0 + (uint32_t)(i / ring), x = (uint32_t)(i % ring);
    ringD[(size_t)l * ring + x] = x == 0 ? 0.0 : __builtin_inf();        // best(-1) = 0
    if (x == 0)
        lanes[l] = CovLane{0, -1, -1, 0};
}

// buf[bufOff[l] ...] = the lane's stored tail, then its new frames; grid (blocks, lanes)
__global__ __launch_bounds__(256) void coverer_gather_kernel(const CovStep *steps, const uint64_t *bufOff, const double *tail,
                                                             double *buf, uint32_t dim, uint32_t tailFrames)
{
    const uint32_t l = blockIdx.y;
    const CovStep s = steps[l];
    if (s.m == 0)
        return;
    const uint64_t nTail = (uint64_t)s.tail * dim, nAll = nTail + (uint64_t)s.m * dim;
    const double *t0 = tail + (size_t)l * tailFrames * dim;
    double *b0 = buf + bufOff[l] * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nAll; i += (uint64_t)gridDim.x * blockDim.x)
        b0[i] = i < nTail ? t0[i] : s.rows[i - nTail];
}

// the lane's new tail: the last min(tail + m, W - 1) frames of its part of the buffer
__global__ __launch_bounds__(256) void coverer_tail_kernel(const CovStep *steps, const uint64_t *bufOff, double *tail,
                                                           const double *buf, uint32_t dim, uint32_t tailFrames)
{
    const uint32_t l = blockIdx.y;
    const CovStep s = steps[l];
    if (s.m == 0)
        return;
    const uint64_t have = (uint64_t)s.tail + s.m;
    const uint64_t keep = have < tailFrames ? have : tailFrames;
    const double *b0 = buf + (bufOff[l] + have - keep) * dim;
    double *t0 = tail + (size_t)l * tailFrames * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < keep * dim; i += (uint64_t)gridDim.x * blockDim.x)
        t0[i] = b0[i];
}

struct CovChainArgs {
    const double *tabM;          // [width][frames]: the folded tables of the buffer
    const uint32_t *tabSrc;
    const uint64_t *bufOff;
    const CovStep *steps;
    CovLane *lanes;
    double *ringD;
    uint32_t ring, width;
    uint64_t frames;
    double penalty;
    double gapCost;              // the price of a frame left uncovered; +inf: the plain cover
    uint64_t backCap;
    uint32_t *bpLen, *bpSrc;
    double *bpCost;
};

// one wave per lane: best(e) and the back-pointers of the new ends
__global__ __launch_bounds__(64) void coverer_chain_kernel(const CovChainArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double ringL[];       // a.ring doubles
    const uint32_t l = blockIdx.x, lane = threadIdx.x;
    const CovStep s = a.steps[l];
    if (s.m == 0)
        return;
    double *ringG = a.ringD + (size_t)l * a.ring;
    for (uint32_t i = lane; i < a.ring; i += 64)
        ringL[i] = ringG[i];
    __syncthreads();
    const uint64_t n = (uint64_t)a.lanes[l].n;
    long long lastFinite = a.lanes[l].lastFinite;
    const uint64_t col0 = a.bufOff[l] + s.tail;
    const size_t b0 = (size_t)l * a.backCap;
    for (uint32_t k = 0; k < s.m; ++k) {
        const uint64_t e = n + k;
        // a window of L frames that ends at e starts at e + 1 - L >= 0, and in the buffer at tail + k + 1 - L >= 0: with
        // tail = min(n, W - 1) the first says both
        const uint32_t lMax = (uint32_t)(e + 1 < a.width ? e + 1 : a.width);
        const CoverPick pick = cover_chain_step(a.tabM, a.tabSrc, a.frames, col0 + k, lMax, a.penalty, a.gapCost, ringL, a.ring - 1,
                                                    e, lane);
        if (lane == 0) {
            ringL[(e + 1) & (a.ring - 1)] = pick.v;
            const size_t o = b0 + (e & (a.backCap - 1));
            a.bpLen[o] = pick.len;
            a.bpSrc[o] = pick.src;
            a.bpCost[o] = pick.m;
        }
        if (pick.v < __builtin_inf())
            lastFinite = (long long)e;
        __syncthreads();
    }
    for (uint32_t i = lane; i < a.ring; i += 64)
        ringG[i] = ringL[i];
    if (lane == 0) {
        a.lanes[l].n = (long long)(n + s.m);
        a.lanes[l].lastFinite = lastFinite;
    }
}

struct CovCommitArgs {
    const CovStep *steps;
    CovLane *lanes;
    const double *ringD;
    uint32_t ring, width;
    uint64_t backCap;
    const uint32_t *bpLen, *bpSrc;
    const double *bpCost;
    uint32_t *logLane, *logSrc, *logStart, *logEnd;
    double *logCost;
};

__device__ __forceinline__ long long wave_min(long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const long long o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

// one wave per lane: C(n) (or walk(lastFinite) for a flush), and the pieces beyond done into the log
__global__ __launch_bounds__(64) void coverer_commit_kernel(const CovCommitArgs a)
{
    const uint32_t l = blockIdx.x, lane = threadIdx.x;
    const CovStep s = a.steps[l];
    if (s.m == 0 && !s.flush)
        return;
    const long long NOPOS = 0x7fffffffffffffffll;
    const double INF = __builtin_inf();
    const CovLane st = a.lanes[l];
    const long long n = st.n, done = st.done;
    const double *ring = a.ringD + (size_t)l * a.ring;
    const uint32_t *len = a.bpLen + (size_t)l * a.backCap;
    const uint64_t mask = a.backCap - 1;
    // one piece back.  A position above done has its back-pointer in the store, and a finite end's piece has 1 ... W
    // frames; anything else (it cannot be, but a walk must end whatever the memory holds) drops the walk to done
    auto back = [&](long long p) -> long long {
        const uint32_t L = p > done ? len[(uint64_t)p & mask] : 0;
        return L - 1 < a.width ? p - (long long)L : done;
    };
    long long c;                                         // the end of the last piece that is final
    if (s.flush) {
        c = st.lastFinite;
    } else {
        // the ends of H(n), this wave lane's brought to their common ancestor.  A position above done has its back-pointer
        // in the store; every end of H(n) descends from done, so no walk passes below it (a walk that would is held there)
        const long long lo = n - (long long)a.width < -1 ? -1 : n - (long long)a.width;
        long long my = NOPOS;
        for (long long e = lo + lane; e <= n - 1; e += 64) {
            if (!(ring[(uint64_t)(e + 1) & (a.ring - 1)] < INF))
                continue;
            long long q = e;
            if (my == NOPOS)
                my = q;
            while (my != q) {
                if (my > q)
                    my = my > done ? back(my) : q;
                else
                    q = q > done ? back(q) : my;
            }
        }
        // every lane steps back while it is above the wave-wide minimum
        for (;;) {
            const long long mn = wave_min(my);
            const long long mx = -wave_min(my == NOPOS ? NOPOS : -my);     // over the lanes that hold an end
            if (mn == NOPOS || mn == mx) {
                c = mn == NOPOS ? done : mn;             // H(n) empty: nothing new
                break;
            }
            if (my != NOPOS && my > mn)
                my = my > done ? back(my) : mn;
        }
    }
    if (c < done)
        c = done;
    if (lane == 0) {
        unsigned long long count = 0;
        for (long long p = c; p > done; p = back(p))
            ++count;
        const uint32_t *src = a.bpSrc + (size_t)l * a.backCap;
        const double *cost = a.bpCost + (size_t)l * a.backCap;
        uint64_t k = s.logAt + count;
        for (long long p = c; p > done;) {
            const uint32_t L = len[(uint64_t)p & mask];
            --k;
            a.logLane[k] = l;
            a.logSrc[k] = src[(uint64_t)p & mask];
            a.logStart[k] = (uint32_t)(p + 1 - (long long)L);
            a.logEnd[k] = (uint32_t)p;
            a.logCost[k] = cost[(uint64_t)p & mask];
            p = back(p);
        }
        a.lanes[l].done = c;
        a.lanes[l].count = count;
    }
}

// the back-pointers of the uncommitted stretch, from a store of oldCap frames per lane into one of newCap
__global__ __launch_bounds__(256) void coverer_regrow_kernel(const CovLane *lanes, uint64_t oldCap, uint64_t newCap,
                                                             const uint32_t *oldLen, const uint32_t *oldSrc, const double *oldCost,
                                                             uint32_t *newLen, uint32_t *newSrc, double *newCost)
{
    const uint32_t l = blockIdx.y;
    const long long first = lanes[l].done + 1, n = lanes[l].n;
    for (long long e = first + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const size_t from = (size_t)l * oldCap + ((uint64_t)e & (oldCap - 1)), to = (size_t)l * newCap + ((uint64_t)e & (newCap - 1));
        newLen[to] = oldLen[from];
        newSrc[to] = oldSrc[from];
        newCost[to] = oldCost[from];
    }
}

__global__ __launch_bounds__(256) void coverer_best_kernel(const CovLane *lanes, const double *ringD, uint32_t ring, uint32_t nLanes,
                                                           double *total, uint32_t *covered, uint32_t *committed)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nLanes)
        return;
    const CovLane s = lanes[l];
    const double v = ringD[(size_t)l * ring + ((uint64_t)s.n & (ring - 1))];          // best(n - 1)
    if (total)
        total[l] = s.n > 0 && v < __builtin_inf() ? v : __builtin_inf();
    if (covered)
        covered[l] = (uint32_t)(s.lastFinite + 1);
    if (committed)
        committed[l] = (uint32_t)(s.done + 1);
}

void coverer_free(ssym_ctx *ctx, ssym_coverer *cv)
{
    for (void *p : {(void *)cv->tail, (void *)cv->ringD, (void *)cv->lanes, (void *)cv->dSteps, (void *)cv->dBufOff,
                    (void *)cv->bpCost, (void *)cv->bpLen, (void *)cv->bpSrc})
        if (p)
            dev_free(ctx, p);
    cv->log.free(ctx);
    delete cv;
}

constexpr const char *kNoun = "coverer";

// the back-pointer store with room for `frames` per lane (a power of two); the uncommitted stretches move over
int32_t back_store(ssym_ctx *ctx, ssym_coverer *cv, uint64_t frames)
{
    const uint64_t cap = pow2_at_least(frames);
    const size_t count = (size_t)cv->nLanes * cap;
    double *cost = nullptr;
    uint32_t *len = nullptr, *src = nullptr;
    int32_t rc = alloc_n(ctx, &cost, count);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &len, count);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &src, count);
    return ring_swap(
        ctx, kNoun, rc, {cv->bpCost, cv->bpLen, cv->bpSrc}, {cost, len, src}, cv->backCap != 0,
        [&] {
            coverer_regrow_kernel<<<dim3(4, cv->nLanes), 256, 0, ctx->stream>>>(cv->lanes, cv->backCap, cap, cv->bpLen, cv->bpSrc,
                                                                                 cv->bpCost, len, src, cost);
        },
        [&] {
            cv->bpCost = cost;
            cv->bpLen = len;
            cv->bpSrc = src;
            cv->backCap = cap;
        });
}

// ssym_coverer_create (gap_cost = +inf) and ssym_coverer_create_gaps: the chain's gap candidate is the only difference
int32_t coverer_create(ssym_ctx *ctx, const char *fn, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty, double gap_cost,
                       ssym_coverer **out)
{
    int32_t rc = tiling_create_checks(ctx, fn, dict, n_lanes, piece_penalty, gap_cost, out);
    if (rc != SSYM_OK)
        return rc;
    const SegmentSet &src = dict->set;
    rc = check_cover_dict(ctx, fn, src);
    if (rc != SSYM_OK)
        return rc;
    const CoverLimits lim = cover_limits();
    const uint32_t W = 2 * std::max(src.max_frames, 1u);
    // the tables of one slice: lanes x (W - 1 + frames) x W x 12 bytes for one source block
    const uint64_t perFrame = (uint64_t)n_lanes * W * (sizeof(double) + sizeof(uint32_t));
    if (lim.scratch_bytes / perFrame < W) {
        ctx->err = std::string(fn) + ": the tables of a one-frame push need lanes x 2 Fmax x 2 Fmax x 12 bytes, more than " +
                   std::to_string(lim.scratch_bytes >> 20) + " MiB of scratch; use fewer lanes per coverer";
        return SSYM_E_UNSUPPORTED;
    }
    if (n_lanes > kCovererMaxLanes) {
        ctx->err = std::string(fn) + ": more than " + std::to_string(kCovererMaxLanes) + " lanes";
        return SSYM_E_UNSUPPORTED;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ssym_coverer *cv = new ssym_coverer;
    cv->bind(ctx, dict, n_lanes, piece_penalty, gap_cost);
    cv->width = W;
    cv->ring = lim.ring;
    cv->sliceMax = std::min<uint64_t>(lim.scratch_bytes / perFrame - (W - 1), kLaneMaxFrames);
    cv->lastFinite.assign(n_lanes, -1);
    rc = alloc_n(ctx, &cv->tail, (size_t)n_lanes * (W - 1) * src.dim);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &cv->ringD, (size_t)n_lanes * cv->ring);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &cv->lanes, (size_t)n_lanes);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &cv->dSteps, (size_t)n_lanes);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &cv->dBufOff, (size_t)n_lanes + 1);
    uint64_t back = kCovererBackMin;
    if (const char *k = ssym_knob("SSYM_COVERER_BACK"))
        back = (uint64_t)std::max(1, atoi(k));
    if (rc == SSYM_OK)
        rc = back_store(ctx, cv, back);
    if (rc != SSYM_OK) {
        coverer_free(ctx, cv);
        return rc;
    }
    const uint64_t cells = (uint64_t)n_lanes * cv->ring;
    coverer_init_kernel<<<(unsigned)((cells + 255) / 256), 256, 0, ctx->stream>>>(cv->lanes, cv->ringD, cv->ring, 0u, n_lanes);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->err = std::string(fn) + ": " + hipGetErrorString(e);
        coverer_free(ctx, cv);
        return SSYM_E_HIP;
    }
    *out = cv;
    return SSYM_OK;
}

// The coverer's part of a push, follow or flush (the loop is tiling_run, lane_tiling.hpp): the frames go through in slices of
// at most `slice` per lane, and a slice's frame buffer has [tail | new] of every lane with new frames, lane l's at bufOff[l]
// (it goes up with the steps).  The buffer is allocated with the first slice's room, behind the log's.
struct CovererSlices {
    ssym_ctx *ctx;
    ssym_coverer *cv;
    uint64_t slice;
    Blocks &bl;
    uint64_t bufFrames;                      // what the largest slice of the call needs
    double *buf;
    std::vector<uint64_t> bufOff;            // [nLanes + 1], in frames
    CoverTables tab;                         // the forward pass's tables of the slice

    int32_t plan(const TilingCall &call, std::vector<CovStep> &steps, uint64_t *left, uint64_t *need)
    {
        const uint32_t nL = cv->nLanes, W = cv->width;
        uint64_t frames = 0;
        for (uint32_t l = 0; l < nL; ++l) {
            CovStep &s = steps[l];
            const uint64_t ml = tiling_step(cv, call, l, slice, &s), n = cv->consumed[l];
            s.tail = (uint32_t)std::min<uint64_t>(n, W - 1);
            s.pad = 0;
            bufOff[l] = frames;
            frames += ml ? s.tail + ml : 0;
            if (ml)
                *need = std::max(*need, n - (uint64_t)(cv->done[l] + 1) + ml);
            *left += ml;
        }
        bufOff[nL] = frames;
        return SSYM_OK;
    }

    int32_t grow(uint64_t need)
    {
        if (!buf && bufFrames) {
            const int32_t rc = bl.get(&buf, (size_t)bufFrames * cv->dim);
            if (rc != SSYM_OK)
                return rc;
        }
        return need > cv->backCap ? back_store(ctx, cv, need) : SSYM_OK;
    }

    // gather, the new tails, and the tables of the buffer
    int32_t forward(bool any)
    {
        const uint32_t nL = cv->nLanes, dim = cv->dim, W = cv->width;
        hipStream_t st = ctx->stream;
        tab = CoverTables{};
        if (any) {
            const unsigned gx = (unsigned)std::min<uint64_t>(((uint64_t)(W - 1 + slice) * dim + 255) / 256, 64);
            coverer_gather_kernel<<<dim3(gx, nL), 256, 0, st>>>(cv->dSteps, cv->dBufOff, cv->tail, buf, dim, W - 1);
            SSYM_HIP_CHECK(ctx, hipGetLastError());
            coverer_tail_kernel<<<dim3(std::min(gx, 8u), nL), 256, 0, st>>>(cv->dSteps, cv->dBufOff, cv->tail, buf, dim, W - 1);
            SSYM_HIP_CHECK(ctx, hipGetLastError());
            return cover_forward(ctx, cv->dict->set, buf, cv->dBufOff, bufOff.data(), nL, 0, 0, &tab);
        }
        return SSYM_OK;
    }

    // the chain over the new ends, then the commit (or the flush's emission)
    int32_t commit(bool any)
    {
        const uint32_t nL = cv->nLanes, W = cv->width;
        hipStream_t st = ctx->stream;
        if (any) {
            CovChainArgs c{};
            c.tabM = tab.tabM;
            c.tabSrc = tab.tabSrc;
            c.bufOff = cv->dBufOff;
            c.steps = cv->dSteps;
            c.lanes = cv->lanes;
            c.ringD = cv->ringD;
            c.ring = cv->ring;
            c.width = W;
            c.frames = bufOff[nL];
            c.penalty = cv->penalty;
            c.gapCost = cv->gapCost;
            c.backCap = cv->backCap;
            c.bpLen = cv->bpLen;
            c.bpSrc = cv->bpSrc;
            c.bpCost = cv->bpCost;
            coverer_chain_kernel<<<nL, 64, sizeof(double) * cv->ring, st>>>(c);
            SSYM_HIP_CHECK(ctx, hipGetLastError());
        }
        CovCommitArgs k{};
        k.steps = cv->dSteps;
        k.lanes = cv->lanes;
        k.ringD = cv->ringD;
        k.ring = cv->ring;
        k.width = W;
        k.backCap = cv->backCap;
        k.bpLen = cv->bpLen;
        k.bpSrc = cv->bpSrc;
        k.bpCost = cv->bpCost;
        k.logLane = cv->log.word(0);
        k.logSrc = cv->log.word(1);
        k.logStart = cv->log.word(2);
        k.logEnd = cv->log.word(3);
        k.logCost = cv->log.cost;
        coverer_commit_kernel<<<nL, 64, 0, st>>>(k);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        return SSYM_OK;
    }

    void fold(uint32_t l, const CovLane &lane) { cv->lastFinite[l] = lane.lastFinite; }
};

// what push, follow and flush hand to the entry bodies (lane_feed.hpp): the coverer's feed and its run
LaneFeed coverer_feed(ssym_ctx *ctx, const ssym_coverer *cv)
{
    return feed_of(ctx, cv, kNoun, "out_n_pieces");
}

auto coverer_run(ssym_ctx *ctx, ssym_coverer *cv, uint64_t *out_n_pieces)
{
    return [=](const char *fn, const std::vector<const double *> &rows, const std::vector<uint64_t> &m, uint32_t flushLane) -> int32_t {
        const uint32_t nL = cv->nLanes, W = cv->width;
        uint64_t slice = cv->sliceMax;
        if (const char *k = ssym_knob("SSYM_COVERER_SLICE"))
            slice = std::min<uint64_t>(slice, (uint64_t)std::max(1, atoi(k)));
        // the frame buffer of a slice: per lane with new frames, its tail and at most `slice` of them
        uint64_t bufFrames = 0;
        for (uint32_t l = 0; l < nL; ++l)
            if (m[l])
                bufFrames += (W - 1) + std::min(slice, m[l]);
        Blocks bl(ctx);
        CovererSlices o{ctx, cv, slice, bl, bufFrames, nullptr, std::vector<uint64_t>((size_t)nL + 1), CoverTables{}};
        return tiling_run(ctx, cv, o, cv->dSteps, cv->lanes, cv->dict->set.n, fn, rows, m, flushLane, out_n_pieces,
                          Upload{cv->dBufOff, o.bufOff.data(), sizeof(uint64_t) * (nL + 1)});
    };
}

int32_t coverer_pieces(ssym_ctx *ctx, const ssym_coverer *cv, uint32_t *out_lane, uint32_t *out_src, uint32_t *out_start,
                       uint32_t *out_end, double *out_cost, uint32_t flags)
{
    int32_t rc = check_handle(ctx, cv, kNoun, "ssym_coverer_pieces");
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint32_t *const outs[4] = {out_lane, out_src, out_start, out_end};
    return cv->log.copy(ctx, out_cost, outs, (flags & SSYM_OUT_DEVICE) != 0);
}

int32_t coverer_best(ssym_ctx *ctx, const ssym_coverer *cv, double *out_total, uint32_t *out_covered, uint32_t *out_committed,
                     uint32_t flags)
{
    return tiling_best(ctx, cv, kNoun, "ssym_coverer_best", out_total, out_covered, out_committed, flags,
                       [&](double *total, uint32_t *covered, uint32_t *committed) {
                           const uint32_t nL = cv->nLanes;
                           coverer_best_kernel<<<(nL + 255) / 256, 256, 0, ctx->stream>>>(cv->lanes, cv->ringD, cv->ring, nL, total,
                                                                                           covered, committed);
                       });
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_coverer_create(ssym_ctx *ctx, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty, ssym_coverer **out)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        return coverer_create(ctx, "ssym_coverer_create", dict, n_lanes, piece_penalty, __builtin_inf(), out);
    });
}

int32_t ssym_coverer_create_gaps(ssym_ctx *ctx, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty, double gap_cost,
                                 ssym_coverer **out)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        return coverer_create(ctx, "ssym_coverer_create_gaps", dict, n_lanes, piece_penalty, gap_cost, out);
    });
}

int32_t ssym_coverer_destroy(ssym_ctx *ctx, ssym_coverer *cv)
{
    return lane_destroy(ctx, cv, coverer_free);
}

int32_t ssym_coverer_push(ssym_ctx *ctx, ssym_coverer *cv, const double *feats, const uint64_t *frame_offsets, uint32_t flags,
                          uint64_t *out_n_pieces)
{
    return lane_push(ctx, cv, kNoun, "ssym_coverer_push", coverer_feed, feats, frame_offsets, out_n_pieces,
                     coverer_run(ctx, cv, out_n_pieces));
}

int32_t ssym_coverer_follow(ssym_ctx *ctx, ssym_coverer *cv, const ssym_stream *stream, uint32_t flags, uint64_t *out_n_pieces)
{
    return lane_follow(ctx, cv, kNoun, "ssym_coverer_follow", coverer_feed, stream, out_n_pieces, coverer_run(ctx, cv, out_n_pieces));
}

int32_t ssym_coverer_pieces(ssym_ctx *ctx, const ssym_coverer *cv, uint32_t *out_lane, uint32_t *out_src, uint32_t *out_start,
                            uint32_t *out_end, double *out_cost, uint32_t flags)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        return coverer_pieces(ctx, cv, out_lane, out_src, out_start, out_end, out_cost, flags);
    });
}

int32_t ssym_coverer_flush(ssym_ctx *ctx, ssym_coverer *cv, uint32_t lane, uint64_t *out_n_pieces)
{
    return lane_flush(ctx, cv, kNoun, "ssym_coverer_flush", coverer_feed, lane, out_n_pieces, coverer_run(ctx, cv, out_n_pieces));
}

int32_t ssym_coverer_best(ssym_ctx *ctx, const ssym_coverer *cv, double *out_total, uint32_t *out_covered,
                          uint32_t *out_committed, uint32_t flags)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return coverer_best(ctx, cv, out_total, out_covered, out_committed, flags); });
}

int32_t ssym_coverer_counts(const ssym_coverer *cv, uint64_t *out_frames, uint64_t *out_capacity)
{
    if (!cv)
        return SSYM_E_INVALID;
    if (out_frames)
        std::copy(cv->consumed.begin(), cv->consumed.end(), out_frames);
    if (out_capacity)
        *out_capacity = cv->backCap;
    return SSYM_OK;
}

int32_t ssym_coverer_reset(ssym_ctx *ctx, ssym_coverer *cv, uint32_t lane)
{
    return lane_reset(ctx, cv, kNoun, "ssym_coverer_reset", coverer_feed, lane, [&]() -> int32_t {
        coverer_init_kernel<<<(cv->ring + 255) / 256, 256, 0, ctx->stream>>>(cv->lanes, cv->ringD, cv->ring, lane, 1u);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        cv->consumed[lane] = 0;
        cv->done[lane] = cv->lastFinite[lane] = -1;
        cv->ended[lane] = 0;
        return SSYM_OK;
    });
}

}  // extern "C"
