// match.hip -- the search behind ssym_match_queries / _topk / _batch and the two-phase calls: which route a call takes
// (pick_route) and one function per route.  Host code only; every kernel lives with its launch_* function.
#include "ssym_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace ssym;

#define SSYM_MATCH_TRY(expr)                   \
    do {                                       \
        const int32_t rc__ = (expr);           \
        if (rc__ != SSYM_OK)                   \
            return rc__;                       \
    } while (0)

// the tail behind the refcos search's results (refcos_mfma.hip, refcos_pack_tail): header words of its lists + timestamps
constexpr size_t kTailBytes = 4 * sizeof(uint32_t) + 3 * sizeof(unsigned long long);

// per-target values between slot order (inside) and the caller's target order (outside)
__global__ void slots_to_targets_kernel(const double *__restrict__ bySlot, const uint32_t *__restrict__ perm,
                                        uint32_t n, double *__restrict__ byTarget)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        byTarget[perm[i]] = bySlot[i];
}
__global__ void targets_to_slots_kernel(const double *__restrict__ byTarget, const uint32_t *__restrict__ perm,
                                        uint32_t n, double *__restrict__ bySlot)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        bySlot[i] = byTarget[perm[i]];
}
extern "C" __global__ void fill_f64_kernel(double *p, double v, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        p[i] = v;
}

// ---- helpers shared with comm.hip -------------------------------------------------------------------
namespace ssym {

int32_t check_match_args(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q)
{
    if (!ctx)
        return SSYM_E_INVALID;
    if (!dict || !q) {
        ctx->err = "dictionary or queries handle is NULL";
        return SSYM_E_INVALID;
    }
    if (dict->set.n == 0) {
        // the reference indexes sounds[0] of an empty Vec and panics (src/sound.rs:369)
        ctx->err = "empty dictionary";
        return SSYM_E_EMPTY_DICT;
    }
    if (dict->set.dim != q->set.dim) {
        ctx->err = "dim mismatch between dictionary and targets";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

int32_t request_outputs(ssym_ctx *ctx, uint32_t *out_idx, const uint32_t *idxDev, double *out_cost, const double *costDev,
                        uint32_t M, uint32_t k_top)
{
    int32_t rc = stage_d2h(ctx, out_idx, idxDev, sizeof(uint32_t) * (size_t)M * k_top);
    if (rc == SSYM_OK && out_cost)
        rc = stage_d2h(ctx, out_cost, costDev, sizeof(double) * (size_t)M * k_top);
    return rc;
}

void count_exact_giveups(ssym_ctx *ctx, const uint32_t *gave, ssym_timings &tm)
{
    for (int i = 0; i < 8; ++i)
        if ((ctx->pipe_mask >> i & 1u) && gave[i])
            ++tm.exact_redone;
    ctx->pipe_mask = 0;
}

void account_filter_cells(ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, ssym_timings &tm)
{
    if (!tm.pruned && ctx->band < 0)
        tm.n_filter_cells = ctx->launched_cells * 64ull;      // from the launches' geometry (dtw_filter.hip)
    if (tm.pruned) {
        tm.n_filter_cells = ctx->pruned_cells * 64ull;
        if (ctx->band < 0) {
            const double full = (double)src.n_pad * tgt.n_pad * src.frames_pad * std::max<uint32_t>(tgt.max_frames, 1);
            ctx->prune_swept = (float)std::min(1.0, (double)tm.n_filter_cells / full);
        }
    }
}

// few short queries against a small dictionary: the exact kernel on every pair is one launch of a few
// thousand waves, the filter path a chain of ~20 launches (1 query x 1024 entries of 5...40 frames:
// 81 us against 227 us per call; from 16 queries on the filter path is the shorter one).
// (from frame counts, not sets: ssym_match_batch asks BEFORE it packs the targets, to leave out what only the filter needs)
bool few_pairs(uint64_t N, uint64_t M, uint64_t maxSrcFrames, uint64_t maxTgtFrames)
{
    return N * M <= 8192 && maxSrcFrames + maxTgtFrames <= 128;
}

}  // namespace ssym

// ---- which route a call takes -----------------------------------------------------------------------
namespace {

enum class Route { RefcosFilter, RefcosTile, DtwFilter, DtwAllPairs };

// The plain first-minimum search goes through the f64 matrix pipe (refcos_mfma.hip): every pair's dot as a
// GEMM, a rigorous interval per key, and the reference's own arithmetic only on the few pairs that can
// hold a target's minimum (top-k: one of its k smallest keys) -- same bits out.  Small problems keep the exact
// tile kernel on every pair; so does a call whose candidate list overflowed.
// (a sharded step only enqueues: its candidate list's header travels in the gathered status like the dtw
//  lists', and the attempt every rank repeats after an overflow -- so_cap set -- takes the exact tile kernel)
// Top-k goes that way up to k = 64: the waves' own thresholds (the k-th smallest bound of 64 rows each) only decide
// what is LISTED; the threshold that selects the candidates is the k-th smallest bound over all of a target's listed
// pairs (refcos_mfma.hip, refcos_topk_*).  4096 x 4096 x 128f x 12d, k = 2 / 4 / 8 / 16 / 64: 0.41 / 0.47 / 0.63 / 0.93 /
// 2.9 ms against 3.2 / 3.1 / 3.3 / 3.9 / 7.0 ms on the exact tile kernel (tools/refcos_topk_timing.py).
bool refcos_filter_applies(const ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, uint32_t k_top)
{
    const char *kmaxKnob = ssym_knob("SSYM_REFCOS_TOPK_MAX");                       // (measurements: where the filters stop paying)
    const uint32_t kFilterMax = kmaxKnob ? (uint32_t)std::max(1, atoi(kmaxKnob)) : 64u;
    return !(ctx->stream_only && (ctx->so_cap || k_top > 1)) && k_top <= kFilterMax && refcos_mfma_supported(ctx, src, tgt);
}

// frames wider than the filter's 42 values (filter_lower_bound_only): the filter scores the first 42 and bounds the
// cost from below; that supports the whole call, and the two-phase calls without per-target distances
// (sharded runs on wide frames exchange bounds in cost space: no per-target distances there)
bool dtw_filter_applies(const ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, uint32_t flags, bool hasDist,
                        Phase phase)
{
    if (flags & SSYM_DTW_FORCE_EXACT)      // (ssym_match_finish too: after a filtered begin it ignores the bounds)
        return false;
    if ((flags & kFlagFewTargets) && few_pairs(src.n, tgt.n, src.max_frames, tgt.max_frames))
        return false;
    return filter_supported(ctx, src, tgt) && (!filter_lower_bound_only(ctx, src, tgt) || phase == Phase::Whole || !hasDist);
}

Route pick_route(const ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, uint32_t k_top, uint32_t flags,
                 bool hasDist, Phase phase)
{
    if (ctx->metric == SSYM_METRIC_REFCOS)
        return refcos_filter_applies(ctx, src, tgt, k_top) ? Route::RefcosFilter : Route::RefcosTile;
    return dtw_filter_applies(ctx, src, tgt, flags, hasDist, phase) ? Route::DtwFilter : Route::DtwAllPairs;
}

// the ranks of a sharded run may score a candidate per target and agree on its cost before the filter (ssym_match_candidates)
bool prune_applies(const ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt)
{
    return !filter_lower_bound_only(ctx, src, tgt) && pick_route(ctx, src, tgt, 1, 0u, false, Phase::Begin) == Route::DtwFilter;
}

// ---- one call ---------------------------------------------------------------------------------------
struct MatchCall {
    ssym_ctx *ctx;
    const SegmentSet &src, &tgt;
    uint32_t k_top, index_base;
    uint32_t *out_idx;                   // the caller's destinations: host memory, or (outDev) what idxDev / costDev are
    double *out_cost;
    bool outDev;
    const double *distDev = nullptr;     // per-target distance (morph_to, src/sound.rs:440-446), NULL: none
    uint32_t *idxDev = nullptr;          // where the kernels leave the results
    double *costDev = nullptr;
    uint32_t *hdrTail = nullptr;         // refcos with host outputs: the tail (kTailBytes) behind the results' device block
    bool outputsStaged = false;          // host outputs already copied and synchronised
    bool stamped = false;                // refcos filter: the phase times came from device timestamps, not from events
    ssym_timings tm{};

    size_t costBytes() const { return sizeof(double) * (size_t)tgt.n * k_top; }
    size_t idxBytes() const { return (sizeof(uint32_t) * (size_t)tgt.n * k_top + 7) & ~(size_t)7; }      // (the tail's stamps: 8-byte aligned)
    int32_t request_outputs() { return ssym::request_outputs(ctx, out_idx, idxDev, out_cost, costDev, tgt.n, k_top); }
};

int32_t upload_distances(MatchCall &c, const double *distance, Phase phase)
{
    ssym_ctx *ctx = c.ctx;
    if (phase == Phase::Finish) {
        c.distDev = ctx->pending.has_dist ? (const double *)ctx->dist.ptr : nullptr;   // uploaded by begin
    } else if (distance) {
        SSYM_MATCH_TRY(ensure(ctx, ctx->dist, sizeof(double) * c.tgt.n));
        SSYM_MATCH_TRY(stage_h2d(ctx, ctx->dist.ptr, distance, sizeof(double) * c.tgt.n));
        c.distDev = (const double *)ctx->dist.ptr;
    }
    return SSYM_OK;
}

// device outputs: the caller's pointers; host outputs: the context's blocks.  refcos with host outputs: values, indices
// and four header words of the search's lists in ONE device block, so that one copy brings back everything the call
// synchronises for (a search of 0.23 ms notices four)
int32_t place_outputs(MatchCall &c)
{
    ssym_ctx *ctx = c.ctx;
    c.idxDev = c.out_idx;
    c.costDev = c.out_cost;
    if (c.outDev)
        return SSYM_OK;
    if (ctx->metric == SSYM_METRIC_REFCOS) {
        SSYM_MATCH_TRY(ensure(ctx, ctx->out_cost, c.costBytes() + c.idxBytes() + kTailBytes));
        c.costDev = (double *)ctx->out_cost.ptr;
        c.idxDev = (uint32_t *)((char *)ctx->out_cost.ptr + c.costBytes());
        c.hdrTail = (uint32_t *)((char *)c.idxDev + c.idxBytes());
        return SSYM_OK;
    }
    SSYM_MATCH_TRY(ensure(ctx, ctx->out_idx, c.idxBytes()));
    SSYM_MATCH_TRY(ensure(ctx, ctx->out_cost, c.costBytes()));
    c.idxDev = (uint32_t *)ctx->out_idx.ptr;
    c.costDev = (double *)ctx->out_cost.ptr;
    return SSYM_OK;
}

// ---- refcos -----------------------------------------------------------------------------------------
enum class RefcosEnd { Done, TryF64, TakeTile };

// One attempt of the search through a filter: the integer one (q8) where both sets have its records; should ITS list
// overflow -- values so close that 23 bits of fixed point cannot tell them apart -- the f64 filter gets the search
// (TryF64) before the exact tile kernel does (TakeTile; a sharded step repeats with the tile kernel at once: one agreed
// repeat per step).
int32_t refcos_filter(MatchCall &c, bool q8, RefcosEnd *end)
{
    ssym_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    const size_t costBytes = c.costBytes(), idxBytes = c.idxBytes();
    *end = RefcosEnd::Done;
    // Timing without events: an event record between two kernels costs ~7 us of gap on the stream, three of them a
    // tenth of a search of 0.2 ms; the search's first kernel, the first one after the main kernel and the last one
    // read the device's wall clock instead (a sharded step keeps the events: comm.hip reads them).
    unsigned long long *stampsDev = nullptr;
    if (!ctx->stream_only && ctx->wall_clock_khz > 0) {
        SSYM_MATCH_TRY(ensure(ctx, ctx->stamps, 128));
        stampsDev = (unsigned long long *)ctx->stamps.ptr;
    }
    const uint32_t *h1dev = nullptr, *h2dev = nullptr;
    uint32_t h1[2] = {0, 0}, h2[2] = {0, 0};
    if (!stampsDev)
        SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    // (where the tail goes: behind the host outputs' device block, or -- device outputs -- behind the timestamps)
    char *packed = (!ctx->stream_only && !c.outDev && c.hdrTail) ? stage_take(ctx, costBytes + idxBytes + kTailBytes) : nullptr;
    uint32_t *tailDev = packed ? c.hdrTail : (stampsDev ? (uint32_t *)(stampsDev + 4) : nullptr);
    int32_t rc = launch_refcos_match_mfma(ctx, c.src, c.tgt, c.distDev, c.index_base, c.idxDev, c.costDev, &h1dev, &h2dev,
                                          c.k_top, q8, stampsDev, tailDev);
    if (rc == SSYM_E_NOMEM && !ctx->stream_only) {
        // the filters' lists did not fit (a top-k list of a large grid is a few GB): the exact tile kernel needs
        // N x M x 8 bytes only and was the path of these calls before the filters took them
        ctx->err.clear();
        *end = RefcosEnd::TakeTile;
        return SSYM_OK;
    }
    if (rc != SSYM_OK)
        return rc;
    c.tm.refcos_filter = q8 ? 2 : 1;
    c.tm.main_launches = 1;
    if (!stampsDev)
        SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    if (ctx->stream_only) {              // enqueued: ssym_match_sharded reads the headers after the step's one synchronisation
        ctx->so_hdr1 = h1dev;
        ctx->so_hdr2 = h2dev;
        ctx->so_refcos = true;
        ctx->so_filter = false;
        c.tm.used_filter = 1;
        return SSYM_OK;                  // (device outputs: the sharded step's send block)
    }
    // host outputs: results, headers and timestamps come back in one copy and under one synchronisation; should
    // the list have overflowed the results are dropped and the next attempt's staged instead
    const size_t pendingBefore = ctx->pending_d2h.size();
    unsigned long long tailHost[(kTailBytes + 7) / 8] = {0};
    const unsigned char *tailAt = nullptr;
    if (packed) {
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(packed, c.costDev, costBytes + idxBytes + kTailBytes, hipMemcpyDeviceToHost, st));
        if (c.out_cost)
            ctx->pending_d2h.push_back({c.out_cost, packed, costBytes});
        ctx->pending_d2h.push_back({c.out_idx, packed + costBytes, sizeof(uint32_t) * (size_t)c.tgt.n * c.k_top});
        c.outputsStaged = true;
        tailAt = (const unsigned char *)packed + costBytes + idxBytes;
    } else {
        if (stampsDev) {                 // device outputs (or no staging window): the tail alone comes back
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(tailHost, tailDev, kTailBytes, hipMemcpyDeviceToHost, st));
            tailAt = (const unsigned char *)tailHost;
        } else {
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(h1, h1dev, sizeof(h1), hipMemcpyDeviceToHost, st));
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(h2, h2dev, sizeof(h2), hipMemcpyDeviceToHost, st));
        }
        if (!c.outDev) {
            SSYM_MATCH_TRY(c.request_outputs());
            c.outputsStaged = true;
        }
    }
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (tailAt) {
        const uint32_t *t = (const uint32_t *)tailAt;
        h1[0] = t[0]; h1[1] = t[1]; h2[0] = t[2]; h2[1] = t[3];
    }
    if (h1[1]) {                         // more near-ties than the list holds
        ctx->pending_d2h.resize(pendingBefore);
        c.outputsStaged = false;
        c.tm.refcos_filter = 0;
        *end = q8 ? RefcosEnd::TryF64 : RefcosEnd::TakeTile;
        return SSYM_OK;
    }
    c.tm.used_filter = 1;
    c.tm.n_refined = h2[0];
    if (stampsDev) {
        unsigned long long ts[3];
        memcpy(ts, tailAt + 4 * sizeof(uint32_t), sizeof(ts));
        c.tm.main_ms = (float)((double)(ts[1] - ts[0]) / ctx->wall_clock_khz);         // main kernel (+ its init)
        c.tm.reduce_ms = (float)((double)(ts[2] - ts[1]) / ctx->wall_clock_khz);       // selection, exact keys, fold
        c.tm.total_ms = c.tm.main_ms + c.tm.reduce_ms;
        c.stamped = true;
    }
    return SSYM_OK;
}

// the exact tile kernel on every pair, then the fold
int32_t refcos_tile(MatchCall &c)
{
    ssym_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    const uint32_t N = c.src.n, M = c.tgt.n;
    SSYM_MATCH_TRY(ensure(ctx, ctx->cmat, sizeof(double) * (size_t)N * M));
    double *sims = (double *)ctx->cmat.ptr;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    SSYM_MATCH_TRY(launch_refcos_sims(ctx, c.src, c.tgt, sims));
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    SSYM_MATCH_TRY(launch_refcos_argmin(ctx, N, M, sims, c.distDev, c.index_base, c.k_top, c.idxDev, c.costDev));
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    c.tm.main_launches = 1;          // event times are read after the call's one synchronisation (match)
    if (ctx->stream_only)            // enqueued (device outputs): no lists for ssym_match_sharded to look at
        ctx->so_filter = ctx->so_refcos = false;
    return SSYM_OK;
}

// ---- dtw, filter route ------------------------------------------------------------------------------
// early abandoning applies to the plain first-minimum search: of one unsharded call, or of a begin whose candidates were
// scored by ssym_match_candidates and their costs reduced over the ranks (prune_cost_dev); finish does what begin did
bool early_abandoning_applies(const MatchCall &c, uint32_t flags, Phase phase, const double *prune_cost_dev)
{
    if (phase == Phase::Finish)
        return c.ctx->pending.pruned;
    if (!(flags & SSYM_DTW_PRUNE) || c.k_top != 1 || c.distDev)
        return false;
    return phase == Phase::Whole || (prune_cost_dev != nullptr && prune_applies(c.ctx, c.src, c.tgt));
}

// The front: candidates and thresholds of early abandoning, the filter, the per-target bounds (-> ctx->tmin).
int32_t dtw_filter_front(MatchCall &c, bool wide, bool prune, Phase phase, const double *prune_cost_dev)
{
    ssym_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    float *cmat = (float *)ctx->cmat.ptr;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    const float *abandon = nullptr;
    unsigned long long *colCtr = nullptr;
    if (prune) {
        if (phase == Phase::Whole)
            SSYM_MATCH_TRY(launch_dtw_prune_candidates(ctx, c.src, c.tgt));
        SSYM_MATCH_TRY(launch_dtw_prune_thresholds(ctx, c.src, c.tgt, prune_cost_dev, &abandon));
        colCtr = (unsigned long long *)((char *)ctx->abandon.ptr + ctx->abandon.bytes) - 1;
        SSYM_MATCH_TRY(zero_words(ctx, colCtr, sizeof(*colCtr)));
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[6], st));
    SSYM_MATCH_TRY(launch_dtw_filter(ctx, c.src, c.tgt, cmat, abandon, colCtr, prune ? prune_cand_slots(ctx, c.tgt) : nullptr));
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    if (prune && ctx->stream_only) {     // through the pinned window: a pageable destination would block the host
        SSYM_MATCH_TRY(stage_d2h(ctx, &ctx->pruned_cells, colCtr, sizeof(*colCtr)));
    } else if (prune) {
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(&ctx->pruned_cells, colCtr, sizeof(*colCtr), hipMemcpyDeviceToHost, st));
    }
    const double *known = prune ? (const double *)ctx->prune_cost.ptr : nullptr;
    return wide ? launch_dtw_bounds_partial(ctx, c.src, c.tgt, cmat, known, c.k_top, c.distDev)
                : launch_dtw_bounds(ctx, c.src, c.tgt, cmat, c.distDev, c.k_top, known);
}

// one attempt of the back with room for `cap` pairs: select -> certify -> select2 -> exact -> fold
int32_t dtw_filter_back_enqueue(MatchCall &c, bool wide, bool prune, uint64_t cap)
{
    ssym_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    const float *cmat = (const float *)ctx->cmat.ptr;
    const uint32_t M = c.tgt.n;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    SSYM_MATCH_TRY(launch_dtw_select(ctx, c.src, c.tgt, cmat, c.distDev, (uint32_t)cap));          // stage 1
    const uint32_t *hdr1 = (const uint32_t *)ctx->cand.ptr;
    SSYM_MATCH_TRY(ensure(ctx, ctx->cand_xmin, sizeof(float) * cap));
    SSYM_MATCH_TRY(launch_certify(ctx, c.src, c.tgt, hdr1, (const uint2 *)(hdr1 + 2), (uint32_t)cap,
                                  (float *)ctx->cand_xmin.ptr));                                   // certificates
    const uint32_t *knownSrc =
        prune ? (const uint32_t *)((const uint2 *)((const uint32_t *)ctx->prune_pairs.ptr + 2) + M) : nullptr;
    SSYM_MATCH_TRY(launch_dtw_select2(ctx, c.src, c.tgt, cmat, (const float *)ctx->cand_xmin.ptr, c.distDev, (uint32_t)cap,
                                      c.k_top, wide, knownSrc));                                   // stage 2
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
    SSYM_MATCH_TRY(ensure(ctx, ctx->cand_cost, sizeof(double) * (cap + M)));
    const uint32_t *hdr2 = (const uint32_t *)ctx->cand2.ptr;
    SSYM_MATCH_TRY(launch_dtw_exact(ctx, c.src, c.tgt, (const uint2 *)(hdr2 + 2), hdr2, (uint32_t)cap, (double *)ctx->cand_cost.ptr));
    if (prune) {
        SSYM_MATCH_TRY(launch_prune_append_known(ctx, M));
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
    SSYM_MATCH_TRY(launch_dtw_final(ctx, c.src, c.tgt, c.distDev, (uint32_t)(cap + (prune ? M : 0)), c.index_base, c.k_top, c.idxDev,
                          c.costDev));
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[5], st));
    return SSYM_OK;
}

// The back: selection, re-scoring and the fold from the bounds in ctx->tmin, repeated once with the room list 1 asked for.
int32_t dtw_filter_back(MatchCall &c, bool wide, bool prune, Phase phase)
{
    ssym_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    const uint32_t N = c.src.n, M = c.tgt.n;
    ssym_timings &tm = c.tm;
    // list 1 (worst-case margin) is a few pairs per target when near-duplicates exist and
    // ~10^2 when they do not; on overflow stage 1 reports the size it wanted, the later
    // stages see the flag and do nothing, and the selection is redone with that room
    // (exactness never depends on the capacity)
    uint64_t cap = std::max<uint64_t>((256ull + 16ull * (c.k_top - 1)) * M, 65536);
    if (ctx->stream_only && ctx->so_cap)
        cap = ctx->so_cap;               // the size a previous attempt of this step asked for
    cap = std::min<uint64_t>(cap, (uint64_t)N * M);
    float sel_ms = 0.f, ref_ms = 0.f, red_ms = 0.f;
    for (int attempt = 0; attempt < 2; ++attempt) {
        SSYM_MATCH_TRY(dtw_filter_back_enqueue(c, wide, prune, cap));
        const uint32_t *hdr1 = (const uint32_t *)ctx->cand.ptr, *hdr2 = (const uint32_t *)ctx->cand2.ptr;
        if (ctx->stream_only) {          // enqueued, one attempt: ssym_match_sharded looks at the headers later
            ctx->so_hdr1 = hdr1;
            ctx->so_hdr2 = hdr2;
            ctx->so_cap = cap;
            ctx->so_filter = true;
            return SSYM_OK;
        }
        // ONE synchronisation per attempt: the lists' header words land in the pinned window (a copy into
        // pageable memory is a host round trip of its own: three of them and a second synchronisation for the
        // results were 60-80 us of a call), and the host results are requested in front of it -- an
        // overflowing list 1 (rare) drops them and asks again after the repeat
        uint32_t words[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t *hw = ctx->api_depth > 0 ? (uint32_t *)stage_take(ctx, sizeof(words)) : nullptr;
        if (hw)
            memset(hw, 0, sizeof(words));
        else
            hw = words;
        uint32_t *h1 = hw, *h2 = hw + 2, *gave = hw + 4;
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(h1, hdr1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(h2, hdr2, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (ctx->pipe_mask)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(gave, ctx->pipe_flag.ptr, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        const size_t pendingBefore = ctx->pending_d2h.size();
        const bool stagedHere = !c.outDev && ctx->api_depth > 0;
        if (stagedHere) {
            // (a result too large for the window goes straight to the caller's memory: still behind this
            //  synchronisation, and harmlessly overwritten by a repeat)
            SSYM_MATCH_TRY(c.request_outputs());
        }
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        count_exact_giveups(ctx, gave, tm);
        const bool lastAttempt = attempt == 1 || cap == (uint64_t)N * M;
        if (stagedHere && h1[1] && !lastAttempt)
            ctx->pending_d2h.resize(pendingBefore);      // the repeat's results are the ones to hand over
        else if (stagedHere)
            c.outputsStaged = true;
        if (attempt == 0 && phase != Phase::Finish)
            sel_ms += ev_ms(ev[1], ev[2]);      // the per-target threshold (bounds) belongs to selection
        sel_ms += ev_ms(ev[2], ev[3]);
        ref_ms += ev_ms(ev[3], ev[4]);
        red_ms += ev_ms(ev[4], ev[5]);
        tm.n_refined = h2[0];
        if (!h1[1])
            break;
        if (lastAttempt) {
            ctx->err = "dtw: candidate list overflow";
            return SSYM_E_NOMEM;
        }
        cap = h1[0];
        if (cap >= 0xffffffffull) {
            ctx->err = "dtw: too many near-tied candidates for one batch";
            return SSYM_E_UNSUPPORTED;
        }
    }
    tm.main_ms = phase == Phase::Finish ? ctx->pending.main_ms : ev_ms(ev[6], ev[1]);
    account_filter_cells(ctx, c.src, c.tgt, tm);
    if (tm.pruned)
        tm.prune_ms = phase == Phase::Finish ? 0.f : ev_ms(ev[0], ev[6]);
    tm.select_ms = sel_ms;
    tm.refine_ms = ref_ms;
    tm.reduce_ms = red_ms;
    tm.total_ms = ev_ms(ev[0], ev[5]) + (phase == Phase::Finish ? ctx->pending.main_ms : 0.f);
    return SSYM_OK;
}

// Whole: front, then back.  Begin (ssym_match_begin): the front, and the per-target threshold goes out to bounds_dev.
// Finish (ssym_match_finish): the threshold comes back from bounds_dev (after the ranks' all-reduce), then the back.
int32_t dtw_filter(MatchCall &c, uint32_t flags, Phase phase, double *bounds_dev, const double *prune_cost_dev)
{
    ssym_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    const uint32_t M = c.tgt.n;
    c.tm.used_filter = 1;
    SSYM_MATCH_TRY(ensure(ctx, ctx->cmat, sizeof(float) * (size_t)c.src.n_pad * c.tgt.n_pad));
    const bool wide = filter_lower_bound_only(ctx, c.src, c.tgt);
    const bool prune = early_abandoning_applies(c, flags, phase, prune_cost_dev);
    if (phase != Phase::Finish) {
        SSYM_MATCH_TRY(dtw_filter_front(c, wide, prune, phase, prune_cost_dev));
    }
    c.tm.pruned = prune ? 1 : 0;
    c.tm.main_launches = ctx->filter_launches;     // one per class of source lengths (dtw_filter.hip)
    if (phase == Phase::Begin) {
        // hand the threshold out: non-negative doubles (or +inf), bit for bit what stage 1 uses
        slots_to_targets_kernel<<<(M + 255) / 256, 256, 0, st>>>((const double *)ctx->tmin.ptr, c.tgt.perm, M, bounds_dev);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        ctx->pending.pruned = prune;
        if (ctx->stream_only)            // enqueued: ssym_match_sharded reads the times after the step's one synchronisation
            return SSYM_OK;
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        ctx->pending.main_ms = ev_ms(ctx->ev[6], ctx->ev[1]);
        c.tm.main_ms = ctx->pending.main_ms;
        return SSYM_OK;
    }
    if (phase == Phase::Finish) {
        targets_to_slots_kernel<<<(M + 255) / 256, 256, 0, st>>>(bounds_dev, c.tgt.perm, M, (double *)ctx->tmin.ptr);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], st));
    }
    return dtw_filter_back(c, wide, prune, phase);
}

// ---- dtw, the exact kernel on every pair ------------------------------------------------------------
int32_t dtw_all_pairs(MatchCall &c)
{
    ssym_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    const uint32_t N = c.src.n, M = c.tgt.n;
    SSYM_MATCH_TRY(ensure(ctx, ctx->cmat, sizeof(double) * (size_t)N * M));
    double *costs = (double *)ctx->cmat.ptr;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    SSYM_MATCH_TRY(launch_dtw_exact(ctx, c.src, c.tgt, nullptr, nullptr, 0, costs));
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    SSYM_MATCH_TRY(launch_dtw_final_allpairs(ctx, N, M, costs, c.distDev, c.index_base, c.k_top, c.idxDev, c.costDev));
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    if (ctx->stream_only) {              // enqueued: no lists for ssym_match_sharded to look at
        ctx->so_filter = false;
        return SSYM_OK;
    }
    uint32_t gave[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ctx->pipe_mask)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(gave, ctx->pipe_flag.ptr, sizeof(gave), hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    count_exact_giveups(ctx, gave, c.tm);
    c.tm.refine_ms = ev_ms(ev[0], ev[1]);
    c.tm.reduce_ms = ev_ms(ev[1], ev[2]);
    c.tm.total_ms = ev_ms(ev[0], ev[2]);
    c.tm.n_refined = (uint64_t)N * M;
    return SSYM_OK;
}

}  // namespace

// ---- the entry points of the search -----------------------------------------------------------------
namespace ssym {

// k_top = 1: ssym_match_queries (outputs [M]); k_top > 1: ssym_match_topk (outputs [M][k_top]).
int32_t match(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const double *distance, uint32_t index_base,
              uint32_t k_top, uint32_t *out_idx, double *out_cost, uint32_t flags, Phase phase, double *bounds_dev,
              const double *prune_cost_dev)
{
    StageScope stageScope(ctx);
    SSYM_MATCH_TRY(check_match_args(ctx, dict, q));
    MatchCall c{ctx, dict->set, q->set, k_top, index_base, out_idx, out_cost, (flags & SSYM_OUT_DEVICE) != 0};
    const uint32_t M = c.tgt.n;
    c.tm.n_pairs = (uint64_t)c.src.n * M;
    if (M == 0) {
        ctx->timings = c.tm;
        return SSYM_OK;
    }
    if (!out_idx && phase != Phase::Begin) {
        ctx->err = "out_idx is NULL";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (phase != Phase::Finish)
        ctx->pipe_mask = 0;            // give-up counters of the exact kernel's pipelined variant: this call's start here
    if (phase == Phase::Whole) {
        // any other call that uses the context's scratch ends a begin .. finish in progress (finish then reports
        // "without begin") and drops the candidates of ssym_match_candidates: their buffers are shared
        drop_pending(ctx);
        if (ctx->prune_default && M >= 64)      // (a handful of targets: the extra launches cost more than they save)
            flags |= SSYM_DTW_PRUNE;
    }
    SSYM_MATCH_TRY(upload_distances(c, distance, phase));
    SSYM_MATCH_TRY(place_outputs(c));

    int32_t rc = SSYM_OK;
    RefcosEnd end = RefcosEnd::Done;
    switch (pick_route(ctx, c.src, c.tgt, k_top, flags, c.distDev != nullptr, phase)) {
    case Route::RefcosFilter:
        rc = refcos_filter(c, refcos_q8_ready(ctx, c.src, c.tgt), &end);
        if (rc == SSYM_OK && end == RefcosEnd::TryF64)
            rc = refcos_filter(c, false, &end);
        if (rc != SSYM_OK || end == RefcosEnd::Done)
            break;
        [[fallthrough]];
    case Route::RefcosTile:
        rc = refcos_tile(c);
        break;
    case Route::DtwFilter:
        rc = dtw_filter(c, flags, phase, bounds_dev, prune_cost_dev);
        break;
    case Route::DtwAllPairs:
        rc = dtw_all_pairs(c);
        break;
    }
    if (rc != SSYM_OK)
        return rc;
    if (phase == Phase::Begin || ctx->stream_only) {      // nothing to hand over: the bounds went to bounds_dev / a sharded
        ctx->timings = c.tm;                              // step has device outputs and synchronises itself (comm.hip)
        return SSYM_OK;
    }
    if (!c.outDev && !c.outputsStaged)
        SSYM_MATCH_TRY(c.request_outputs());
    const bool refcos = ctx->metric == SSYM_METRIC_REFCOS;
    if ((!c.outDev || refcos) && !c.outputsStaged)      // (staged: already synchronised by the route)
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    stage_finish(ctx);
    if (refcos && !c.stamped) {
        c.tm.main_ms = ev_ms(ctx->ev[0], ctx->ev[1]);
        c.tm.reduce_ms = ev_ms(ctx->ev[1], ctx->ev[2]);
        c.tm.total_ms = ev_ms(ctx->ev[0], ctx->ev[2]);
    }
    ctx->timings = c.tm;
    return SSYM_OK;
}

// Two-phase match for source-sharded runs (see the header).  Where the filter does not apply the candidates' costs /
// the bounds are filled with +inf; the all-reduce then changes nothing.
int32_t match_candidates_impl(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double *cost_dev)
{
    SSYM_MATCH_TRY(check_match_args(ctx, dict, q));
    if (!cost_dev) {
        ctx->err = "ssym_match_candidates: cost_dev is NULL";
        return SSYM_E_INVALID;
    }
    ssym_ctx::Pending &pd = ctx->pending;
    pd = ssym_ctx::Pending{};
    const uint32_t M = q->set.n;
    if (M == 0)
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (prune_applies(ctx, dict->set, q->set)) {
        SSYM_MATCH_TRY(launch_dtw_prune_candidates(ctx, dict->set, q->set));
        slots_to_targets_kernel<<<(M + 255) / 256, 256, 0, ctx->stream>>>((const double *)ctx->prune_cost.ptr,
                                                                          q->set.perm, M, cost_dev);
        pd.cand = true;
        pd.dict = dict;
        pd.q = q;
    } else {
        fill_f64_kernel<<<(M + 255) / 256, 256, 0, ctx->stream>>>(cost_dev, (double)INFINITY, M);
    }
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    if (!ctx->stream_only)
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
}

int32_t match_begin_impl(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const double *distance,
                         uint32_t index_base, double *bounds_dev, const double *prune_cost_dev)
{
    SSYM_MATCH_TRY(check_match_args(ctx, dict, q));
    if (!bounds_dev) {
        ctx->err = "ssym_match_begin: bounds_dev is NULL";
        return SSYM_E_INVALID;
    }
    ssym_ctx::Pending &pd = ctx->pending;
    // the reduced candidate costs are only usable when THIS context scored its candidates for the same sets
    // (finish appends them); otherwise the call is a plain begin
    if (prune_cost_dev && !(pd.cand && pd.dict == dict && pd.q == q && !distance))
        prune_cost_dev = nullptr;
    pd = ssym_ctx::Pending{};
    pd.dict = dict;
    pd.q = q;
    pd.index_base = index_base;
    pd.has_dist = distance != nullptr;
    const uint32_t M = q->set.n;
    if (distance)
        pd.dist_host.assign(distance, distance + M);
    const uint32_t flags = prune_cost_dev ? SSYM_DTW_PRUNE : 0u;
    pd.filter = M > 0 && pick_route(ctx, dict->set, q->set, 1, flags, distance != nullptr, Phase::Begin) == Route::DtwFilter;
    if (pd.filter) {
        SSYM_MATCH_TRY(match(ctx, dict, q, distance, index_base, 1, nullptr, nullptr, flags, Phase::Begin, bounds_dev, prune_cost_dev));
    } else if (M > 0) {
        SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        fill_f64_kernel<<<(M + 255) / 256, 256, 0, ctx->stream>>>(bounds_dev, (double)INFINITY, M);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        if (!ctx->stream_only)
            SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    pd.valid = true;
    return SSYM_OK;
}

// where begin ran the filter, finish runs the route's back (with SSYM_DTW_FORCE_EXACT: the exact kernel on every pair,
// the bounds ignored); where it did not, finish is the whole match
int32_t match_finish_impl(ssym_ctx *ctx, const double *bounds_dev, uint32_t *out_idx, double *out_cost, uint32_t flags)
{
    ssym_ctx::Pending &pd = ctx->pending;
    if (!pd.valid) {
        ctx->err = "ssym_match_finish without ssym_match_begin";
        return SSYM_E_INVALID;
    }
    pd.valid = false;
    if (!bounds_dev) {
        ctx->err = "ssym_match_finish: bounds_dev is NULL";
        return SSYM_E_INVALID;
    }
    const double *dist = pd.has_dist ? pd.dist_host.data() : nullptr;
    return match(ctx, pd.dict, pd.q, dist, pd.index_base, 1, out_idx, out_cost, flags, pd.filter ? Phase::Finish : Phase::Whole,
                 const_cast<double *>(bounds_dev));
}

}  // namespace ssym
