// capi.hip -- the C ABI of include/soundsym_amd.h: handle lifetime, argument checks and the extern "C" wrappers
// (the search behind the match calls: match.hip).
#include "ssym_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

using namespace ssym;

static thread_local std::string g_create_err;

static int32_t make_set(ssym_ctx *ctx, SegmentSet &set, const void *feats, bool on_device,
                        const uint64_t *off, uint32_t n, uint32_t dim, bool is_source)
{
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int32_t rc = pack_segments(ctx, set, feats, on_device, off, n, dim, is_source);
    if (rc != SSYM_OK)
        free_segments(ctx, set);
    return rc;
}

// ssym_dict_create* / ssym_queries_create*: a new handle (T: ssym_dict or ssym_queries) with the segments packed
template <class T>
static int32_t create_set_handle(ssym_ctx *ctx, const void *feats, bool on_device, const uint64_t *frame_offsets,
                                 uint32_t n, uint32_t dim, bool is_source, T **out)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx || !out)
        return SSYM_E_INVALID;
    *out = nullptr;
    T *h = new (std::nothrow) T();
    if (!h)
        return SSYM_E_NOMEM;
    int32_t rc = make_set(ctx, h->set, feats, on_device, frame_offsets, n, dim, is_source);
    if (rc != SSYM_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return SSYM_OK;
    });
}

extern "C" {

int32_t ssym_abi_version(void) { return SSYM_ABI_VERSION; }

const char *ssym_last_error(const ssym_ctx *ctx)
{
    return ctx ? ctx->err.c_str() : g_create_err.c_str();
}

int32_t ssym_ctx_create(const ssym_config *cfg, ssym_ctx **out)
{
    return guarded((ssym_ctx *)nullptr, [&]() -> int32_t {
    if (!cfg || !out || cfg->struct_size != sizeof(ssym_config)) {
        g_create_err = "ssym_ctx_create: bad config (NULL or struct_size mismatch)";
        return SSYM_E_INVALID;
    }
    *out = nullptr;
    if ((cfg->metric != SSYM_METRIC_REFCOS && cfg->metric != SSYM_METRIC_DTW) ||
        (cfg->dtype != SSYM_DTYPE_F64 && cfg->dtype != SSYM_DTYPE_F32) || cfg->band < -1) {
        g_create_err = "ssym_ctx_create: bad metric / dtype / band";
        return SSYM_E_INVALID;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_err = std::string("ssym_ctx_create: no HIP device (") +
                       (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                       "); this library has no CPU path";
        return SSYM_E_NO_DEVICE;
    }
    if (cfg->device < 0 || cfg->device >= ndev) {
        g_create_err = "ssym_ctx_create: device ordinal out of range";
        return SSYM_E_INVALID;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) {
        g_create_err = "ssym_ctx_create: hipGetDeviceProperties failed";
        return SSYM_E_HIP;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_err = std::string("ssym_ctx_create: device is ") + prop.gcnArchName +
                       ", kernels are built for gfx950 only";
        return SSYM_E_NO_DEVICE;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) {
        g_create_err = "ssym_ctx_create: hipSetDevice failed";
        return SSYM_E_HIP;
    }
    ssym_ctx *ctx = new (std::nothrow) ssym_ctx();
    if (!ctx) {
        g_create_err = "out of memory";
        return SSYM_E_NOMEM;
    }
    ctx->device = cfg->device;
    ctx->metric = cfg->metric;
    ctx->dtype = cfg->dtype;
    ctx->band = cfg->band;
    ctx->squared = cfg->dtw_squared ? 1 : 0;
    ctx->prune_default = cfg->dtw_prune != 0;
    ctx->num_cus = prop.multiProcessorCount;
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) == hipSuccess && khz > 0)
            ctx->wall_clock_khz = (double)khz;
    }
    if (cfg->stream) {
        ctx->stream = (hipStream_t)cfg->stream;
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            g_create_err = "hipStreamCreate failed";
            delete ctx;
            return SSYM_E_HIP;
        }
        ctx->owns_stream = true;
    }
    for (auto &ev : ctx->ev) {
        if (hipEventCreate(&ev) != hipSuccess) {
            g_create_err = "hipEventCreate failed";
            delete ctx;
            return SSYM_E_HIP;
        }
    }
    *out = ctx;
    return SSYM_OK;
    });
}

int32_t ssym_ctx_destroy(ssym_ctx *ctx)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    DeviceBuf *bufs[] = {&ctx->handoff, &ctx->cmat, &ctx->tmin, &ctx->cand, &ctx->cand2, &ctx->cand_xmin,
                         &ctx->cand_cost, &ctx->best, &ctx->selmask, &ctx->selcnt, &ctx->topk,
                         &ctx->abandon, &ctx->prune_pairs, &ctx->prune_cost, &ctx->one_ticket, &ctx->dist, &ctx->part, &ctx->paced_part, &ctx->cover_tab, &ctx->mosaic_tab, &ctx->out_idx, &ctx->out_cost,
                         &ctx->pipe_flag, &ctx->tmin2, &ctx->zeros, &ctx->stamps};
    for (DeviceBuf *b : bufs)
        if (b->ptr)
            (void)hipFree(b->ptr);
    release_deferred(ctx);
    dev_cache_release(ctx);
    if (ctx->stage)
        (void)hipHostFree(ctx->stage);
    for (auto &ev : ctx->ev)
        if (ev)
            (void)hipEventDestroy(ev);
    if (ctx->owns_stream)
        (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return SSYM_OK;
    });
}

int32_t ssym_ctx_synchronize(ssym_ctx *ctx)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
    });
}

int32_t ssym_get_timings(const ssym_ctx *ctx, ssym_timings *out)
{
    if (!ctx || !out)
        return SSYM_E_INVALID;
    *out = ctx->timings;
    return SSYM_OK;
}

// ---- dictionary / queries -----------------------------------------------------------------------
int32_t ssym_dict_create(ssym_ctx *ctx, const void *feats, const uint64_t *frame_offsets,
                         uint32_t n_segments, uint32_t dim, ssym_dict **out)
{
    return create_set_handle(ctx, feats, false, frame_offsets, n_segments, dim, true, out);
}

int32_t ssym_dict_create_device(ssym_ctx *ctx, const void *feats_dev, const uint64_t *frame_offsets,
                                uint32_t n_segments, uint32_t dim, ssym_dict **out)
{
    return create_set_handle(ctx, feats_dev, true, frame_offsets, n_segments, dim, true, out);
}

int32_t ssym_dict_append(ssym_ctx *ctx, ssym_dict *dict, const void *feats,
                         const uint64_t *frame_offsets, uint32_t n_segments)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx || !dict)
        return SSYM_E_INVALID;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return append_segments(ctx, dict->set, feats, frame_offsets, n_segments);
    });
}

int32_t ssym_dict_size(const ssym_dict *dict, uint32_t *out_n_segments)
{
    if (!dict || !out_n_segments)
        return SSYM_E_INVALID;
    *out_n_segments = dict->set.n;
    return SSYM_OK;
}

int32_t ssym_dict_destroy(ssym_ctx *ctx, ssym_dict *dict)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!dict)
        return SSYM_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    free_segments(ctx, dict->set);
    if (dict->selfsim.ptr)
        (void)hipFree(dict->selfsim.ptr);
    delete dict;
    return SSYM_OK;
    });
}

int32_t ssym_queries_create(ssym_ctx *ctx, const void *feats, const uint64_t *frame_offsets,
                            uint32_t n_targets, uint32_t dim, ssym_queries **out)
{
    return create_set_handle(ctx, feats, false, frame_offsets, n_targets, dim, false, out);
}

int32_t ssym_queries_create_device(ssym_ctx *ctx, const void *feats_dev, const uint64_t *frame_offsets,
                                   uint32_t n_targets, uint32_t dim, ssym_queries **out)
{
    return create_set_handle(ctx, feats_dev, true, frame_offsets, n_targets, dim, false, out);
}

int32_t ssym_queries_destroy(ssym_ctx *ctx, ssym_queries *q)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!q)
        return SSYM_OK;
    if (ctx)
        (void)hipSetDevice(ctx->device);
    free_segments(ctx, q->set);      // blocks go back to the context's cache; reuse is stream-ordered
    delete q;
    return SSYM_OK;
    });
}

}  // extern "C"

// filter costs live in record-slot coordinates; the caller sees segments in its own order
__global__ void f32_to_f64_matrix_kernel(const float *__restrict__ in, uint32_t rows, uint32_t cols,
                                         uint32_t ld, const uint32_t *__restrict__ permRow,
                                         const uint32_t *__restrict__ permCol, double *__restrict__ out)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = blockIdx.y;
    if (c < cols && r < rows)
        out[(size_t)permRow[r] * cols + permCol[c]] = (double)in[(size_t)r * ld + c];
}

extern "C" {

int32_t ssym_match_queries(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q,
                           const double *distance, uint32_t index_base, uint32_t *out_idx,
                           double *out_cost, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
    return match(ctx, dict, q, distance, index_base, 1, out_idx, out_cost, flags);
    });
}

// the call above with the step pattern as an argument: SSYM_STEP_SYMMETRIC is the call above itself
int32_t ssym_match_queries_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const double *distance,
                                uint32_t index_base, uint32_t step, uint32_t *out_idx, double *out_cost, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (step == SSYM_STEP_SYMMETRIC)
        return match(ctx, dict, q, distance, index_base, 1, out_idx, out_cost, flags);
    if (step != SSYM_STEP_PACED) {
        ctx->err = "ssym_match_queries_step: step must be SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED";
        return SSYM_E_INVALID;
    }
    return match_paced(ctx, dict, q, distance, index_base, out_idx, out_cost, flags, "ssym_match_queries_step");
    });
}

int32_t ssym_match_topk(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const double *distance,
                        uint32_t k, uint32_t index_base, uint32_t *out_idx, double *out_cost, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (k == 0 || k > SSYM_TOPK_MAX) {
        ctx->err = "ssym_match_topk: k must be in 1..SSYM_TOPK_MAX";
        return SSYM_E_INVALID;
    }
    return match(ctx, dict, q, distance, index_base, k, out_idx, out_cost, flags);
    });
}

int32_t ssym_match_candidates(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double *cost_dev)
{
    return guarded(ctx, [&]() -> int32_t {
    return match_candidates_impl(ctx, dict, q, cost_dev);
    });
}

int32_t ssym_match_begin(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const double *distance,
                         uint32_t index_base, double *bounds_dev)
{
    return guarded(ctx, [&]() -> int32_t {
    return match_begin_impl(ctx, dict, q, distance, index_base, bounds_dev, nullptr);
    });
}

int32_t ssym_match_begin_pruned(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, uint32_t index_base,
                                const double *cost_dev, double *bounds_dev)
{
    return guarded(ctx, [&]() -> int32_t {
    if (ctx && !cost_dev) {
        ctx->err = "ssym_match_begin_pruned: cost_dev is NULL";
        return SSYM_E_INVALID;
    }
    return match_begin_impl(ctx, dict, q, nullptr, index_base, bounds_dev, cost_dev);
    });
}

int32_t ssym_match_finish(ssym_ctx *ctx, const double *bounds_dev, uint32_t *out_idx, double *out_cost,
                          uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    return match_finish_impl(ctx, bounds_dev, out_idx, out_cost, flags);
    });
}

int32_t ssym_match_batch(ssym_ctx *ctx, const ssym_dict *dict, const void *tgt_feats,
                         const uint64_t *tgt_frame_offsets, uint32_t n_targets, const double *distance,
                         uint32_t *out_idx, double *out_cost)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (!dict) {
        ctx->err = "dictionary handle is NULL";
        return SSYM_E_INVALID;
    }
    if (dict->set.n == 0) {
        ctx->err = "empty dictionary";
        return SSYM_E_EMPTY_DICT;
    }
    StageScope stageScope(ctx);       // one staging window for the pack and the match
    // refcos, up to 64 short queries -- or dtw, up to 4 short queries against short entries: the whole call in ONE launch
    // (refcos_match_one_kernel / dtw_match_few_kernel); queries, offsets and distances go into the pinned window,
    // which the kernel reads and answers into directly
    const bool fewRefcos = out_idx && tgt_feats && refcos_few_supported(ctx, dict->set, tgt_frame_offsets, n_targets);
    const bool fewDtw = out_idx && tgt_feats && dtw_few_supported(ctx, dict->set, tgt_frame_offsets, n_targets);
    if (fewRefcos || fewDtw) {
        const size_t esz = ctx->dtype == SSYM_DTYPE_F32 ? sizeof(float) : sizeof(double);
        const uint64_t f0 = tgt_frame_offsets[0], f1 = tgt_frame_offsets[n_targets];
        const size_t qBytes = (size_t)(f1 - f0) * dict->set.dim * esz;
        char *qP = stage_take(ctx, qBytes ? qBytes : 8);
        uint64_t *offP = (uint64_t *)stage_take(ctx, sizeof(uint64_t) * (n_targets + 1));
        double *distP = distance ? (double *)stage_take(ctx, sizeof(double) * n_targets) : nullptr;
        double *valP = (double *)stage_take(ctx, sizeof(double) * n_targets);
        uint32_t *idxP = (uint32_t *)stage_take(ctx, sizeof(uint32_t) * n_targets);
        if (qP && offP && valP && idxP && (distP || !distance)) {
            SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
            drop_pending(ctx);
            if (qBytes)
                memcpy(qP, (const char *)tgt_feats + (size_t)f0 * dict->set.dim * esz, qBytes);
            for (uint32_t i = 0; i <= n_targets; ++i)
                offP[i] = tgt_frame_offsets[i] - f0;
            if (distP)
                memcpy(distP, distance, sizeof(double) * n_targets);
            hipEvent_t *ev = ctx->ev;
            // refcos: the kernel reads the device's wall clock into the pinned window itself (two event records cost 2.5 us
            // of a 32 us call); dtw keeps the events
            unsigned long long *tsP = (fewRefcos && ctx->wall_clock_khz > 0) ? (unsigned long long *)stage_take(ctx, 8 * ((size_t)n_targets + 1)) : nullptr;
            const bool noEv = tsP != nullptr;
            if (tsP)
                memset(tsP, 0, 8 * ((size_t)n_targets + 1));
            if (!noEv)
                SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], ctx->stream));
            int32_t rcf = fewRefcos ? launch_refcos_match_few(ctx, dict->set, qP, offP, n_targets, distP, 1.0, valP, idxP, tsP)
                                    : launch_dtw_match_few(ctx, dict->set, qP, offP, n_targets, distP, valP, idxP);
            if (rcf != SSYM_OK)
                return rcf;
            if (!noEv)
                SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], ctx->stream));
            SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            memcpy(out_idx, idxP, sizeof(uint32_t) * n_targets);
            if (out_cost)
                memcpy(out_cost, valP, sizeof(double) * n_targets);
            ssym_timings tm{};
            tm.n_pairs = (uint64_t)dict->set.n * n_targets;
            if (noEv) {
                unsigned long long tEnd = tsP[0];
                for (uint32_t i = 0; i < n_targets; ++i)
                    tEnd = std::max(tEnd, tsP[1 + i]);
                tm.main_ms = tm.total_ms = (float)((double)(tEnd - tsP[0]) / ctx->wall_clock_khz);
            } else {
                tm.main_ms = tm.total_ms = ev_ms(ev[0], ev[1]);
            }
            tm.main_launches = 1;
            ctx->timings = tm;
            return SSYM_OK;
        }
    }
    ssym_queries *q = nullptr;
    hipEvent_t e0 = ctx->ev[8], e1 = ctx->ev[9];      // (the match below records ev[0..6] itself)
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    SSYM_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
    ctx->defer_sync = true;        // this call synchronises once, at the end of the match
    // a handful of short dtw queries go to the exact kernel on every pair (match.hip, kFlagFewTargets): their
    // pack can leave out everything only the filter needs
    const bool fewTargets = n_targets <= 4;
    uint64_t maxQ = 0;
    if (tgt_frame_offsets)
        for (uint32_t i = 0; i < n_targets; ++i)
            maxQ = std::max<uint64_t>(maxQ, tgt_frame_offsets[i + 1] - tgt_frame_offsets[i]);
    ctx->pack_light = ctx->metric == SSYM_METRIC_DTW && fewTargets && few_pairs(dict->set.n, n_targets, dict->set.max_frames, maxQ);
    int32_t rc = ssym_queries_create(ctx, tgt_feats, tgt_frame_offsets, n_targets, dict->set.dim, &q);
    ctx->pack_light = false;
    ctx->defer_sync = false;
    if (rc != SSYM_OK) {
        (void)hipStreamSynchronize(ctx->stream);      // the caller's buffers may go after an error too
        return rc;
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
    // a handful of queries at a time is the reference's own call pattern (match_sound per target,
    // src/sound.rs:453-454): what counts then is the length of the launch chain, see few_pairs
    rc = match(ctx, dict, q, distance, 0, 1, out_idx, out_cost, fewTargets ? kFlagFewTargets : 0u);
    if (rc == SSYM_OK)
        ctx->timings.pack_ms = ev_ms(e0, e1);
    else
        (void)hipStreamSynchronize(ctx->stream);
    ssym_queries_destroy(ctx, q);
    return rc;
    });
}

int32_t ssym_match_one(ssym_ctx *ctx, const ssym_dict *dict, const void *feats, uint64_t n_frames,
                       double distance, uint32_t *out_idx, double *out_cost)
{
    return guarded(ctx, [&]() -> int32_t {
    const uint64_t off[2] = {0, n_frames};
    return ssym_match_batch(ctx, dict, feats, off, 1, &distance, out_idx, out_cost);
    });
}

/* from_distances (src/sound.rs:405-417) on the device; see chain.hip. */
int32_t ssym_chain(ssym_ctx *ctx, ssym_dict *dict, const void *start_feats, uint64_t start_frames,
                   const double *distances, uint32_t n_steps, uint32_t *out_idx, double *out_cost)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (!dict) {
        ctx->err = "dictionary handle is NULL";
        return SSYM_E_INVALID;
    }
    if (n_steps == 0)
        return SSYM_OK;
    if (!distances || !out_idx || (!start_feats && start_frames)) {
        ctx->err = "ssym_chain: NULL argument";
        return SSYM_E_INVALID;
    }
    const SegmentSet &src = dict->set;
    const uint32_t N = src.n;
    if (N == 0) {
        ctx->err = "empty dictionary";          // the reference panics at the first step (:369)
        return SSYM_E_EMPTY_DICT;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    drop_pending(ctx);          // (the chain uses the scratch a begin .. finish would still need)
    hipStream_t st = ctx->stream;
    const bool refcos = ctx->metric == SSYM_METRIC_REFCOS;
    const double init = refcos ? 2.0 : (double)INFINITY;

    // device outputs + the current index
    int32_t rc = ensure(ctx, ctx->out_idx, sizeof(uint32_t) * ((size_t)n_steps + 1));
    if (rc != SSYM_OK)
        return rc;
    rc = ensure(ctx, ctx->out_cost, sizeof(double) * n_steps);
    if (rc != SSYM_OK)
        return rc;
    uint32_t *idxDev = (uint32_t *)ctx->out_idx.ptr;
    uint32_t *cur = idxDev + n_steps;
    double *costDev = (double *)ctx->out_cost.ptr;

    // step 0: the start sound against the whole dictionary (N values)
    const uint64_t off[2] = {0, start_frames};
    ssym_queries *q = nullptr;
    rc = ssym_queries_create(ctx, start_feats, off, 1, src.dim, &q);
    if (rc != SSYM_OK)
        return rc;
    rc = ensure(ctx, ctx->cmat, sizeof(double) * N);
    if (rc == SSYM_OK)
        rc = refcos ? launch_refcos_sims(ctx, src, q->set, (double *)ctx->cmat.ptr)
                    : launch_dtw_exact(ctx, src, q->set, nullptr, nullptr, 0, (double *)ctx->cmat.ptr);
    if (rc == SSYM_OK)
        rc = launch_chain_argmin(ctx, (const double *)ctx->cmat.ptr, 0, nullptr, N, distances[0], init, !refcos,
                                 0, cur, idxDev, costDev);
    if (rc != SSYM_OK) {
        ssym_queries_destroy(ctx, q);
        return rc;
    }

    if (n_steps > 1 && refcos) {
        // later queries are dictionary entries: rows of the self-similarity matrix
        if (dict->selfsim_n != N) {
            rc = ensure(ctx, dict->selfsim, sizeof(double) * (size_t)N * N);
            if (rc == SSYM_OK)
                rc = launch_refcos_sims(ctx, src, src, (double *)dict->selfsim.ptr);
            if (rc != SSYM_OK) {
                ssym_queries_destroy(ctx, q);
                return rc;
            }
            dict->selfsim_n = N;
        }
        for (uint32_t i = 1; i < n_steps && rc == SSYM_OK; ++i)
            rc = launch_chain_argmin(ctx, (const double *)dict->selfsim.ptr, N, cur, N, distances[i], init, false, i,
                                     cur, idxDev, costDev);
    } else if (n_steps > 1) {
        rc = ensure(ctx, ctx->cand, sizeof(uint32_t) * 2 + sizeof(uint2) * (size_t)N);
        if (rc == SSYM_OK)
            rc = ensure(ctx, ctx->cand_cost, sizeof(double) * N);
        uint32_t *hdr = (uint32_t *)ctx->cand.ptr;
        for (uint32_t i = 1; i < n_steps && rc == SSYM_OK; ++i) {
            rc = launch_chain_pairs(ctx, cur, N, (uint2 *)(hdr + 2), hdr);
            if (rc == SSYM_OK)
                rc = launch_dtw_exact(ctx, src, src, (const uint2 *)(hdr + 2), hdr, N, (double *)ctx->cand_cost.ptr);
            if (rc == SSYM_OK)
                rc = launch_chain_argmin(ctx, (const double *)ctx->cand_cost.ptr, 0, nullptr, N, distances[i], init,
                                         true, i, cur, idxDev, costDev);
        }
    }
    if (rc == SSYM_OK) {
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_idx, idxDev, sizeof(uint32_t) * n_steps, hipMemcpyDeviceToHost, st));
        if (out_cost)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_cost, costDev, sizeof(double) * n_steps, hipMemcpyDeviceToHost,
                                               st));
    }
    hipError_t e = hipStreamSynchronize(st);
    ssym_queries_destroy(ctx, q);
    if (rc == SSYM_OK && e != hipSuccess) {
        ctx->err = std::string("ssym_chain: ") + hipGetErrorString(e);
        return SSYM_E_HIP;
    }
    return rc;
    });
}

}  // extern "C"

static int32_t pair_matrix(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, int32_t exact, double *out_matrix)
{
    int32_t rc = check_match_args(ctx, dict, q);
    if (rc != SSYM_OK)
        return rc;
    if (!out_matrix) {
        ctx->err = "out_matrix is NULL";
        return SSYM_E_INVALID;
    }
    drop_pending(ctx);          // (the matrix lands in the scratch a begin .. finish would still need)
    const SegmentSet &src = dict->set;
    const SegmentSet &tgt = q->set;
    const uint32_t N = src.n, M = tgt.n;
    if (M == 0)
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    rc = ensure(ctx, ctx->part, sizeof(double) * (size_t)N * M);
    if (rc != SSYM_OK)
        return rc;
    double *mat = (double *)ctx->part.ptr;
    if (ctx->metric == SSYM_METRIC_REFCOS) {
        if (exact == 3 && !refcos_q8_ready(ctx, src, tgt)) {
            ctx->err = "the integer filter does not take these sets (a value that is not finite or far out of range, a "
                       "segment of more than 32768 values, SSYM_REFCOS_Q8=0): ask for exact = 2";
            return SSYM_E_UNSUPPORTED;
        }
        rc = exact >= 2 ? launch_refcos_mfma_sims(ctx, src, tgt, mat, exact == 3) : launch_refcos_sims(ctx, src, tgt, mat);
    } else if (exact) {
        rc = launch_dtw_exact(ctx, src, tgt, nullptr, nullptr, 0, mat);
    } else {
        if (!filter_supported(ctx, src, tgt)) {
            ctx->err = "dtw filter does not cover this shape (band / frames / dim); ask for exact = 1";
            return SSYM_E_UNSUPPORTED;
        }
        rc = ensure(ctx, ctx->cmat, sizeof(float) * (size_t)src.n_pad * tgt.n_pad);
        if (rc != SSYM_OK)
            return rc;
        rc = launch_dtw_filter(ctx, src, tgt, (float *)ctx->cmat.ptr);
        if (rc == SSYM_OK) {
            dim3 grid((M + 255) / 256, N);
            f32_to_f64_matrix_kernel<<<grid, 256, 0, st>>>((const float *)ctx->cmat.ptr, N, M, tgt.n_pad, src.perm,
                                                           tgt.perm, mat);
            SSYM_HIP_CHECK(ctx, hipGetLastError());
        }
    }
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_matrix, mat, sizeof(double) * (size_t)N * M,
                                       hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return SSYM_OK;
}

extern "C" {

int32_t ssym_pair_matrix(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, int32_t exact,
                         double *out_matrix)
{
    return guarded(ctx, [&]() -> int32_t {
    return pair_matrix(ctx, dict, q, exact, out_matrix);
    });
}

// the call above with the step pattern in place of the mode: SSYM_STEP_SYMMETRIC is the call above with exact = 1
int32_t ssym_pair_matrix_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, uint32_t step, double *out_matrix)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (step == SSYM_STEP_SYMMETRIC)
        return pair_matrix(ctx, dict, q, 1, out_matrix);
    if (step != SSYM_STEP_PACED) {
        ctx->err = "ssym_pair_matrix_step: step must be SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED";
        return SSYM_E_INVALID;
    }
    return pair_matrix_paced(ctx, dict, q, out_matrix, "ssym_pair_matrix_step");
    });
}

int32_t ssym_merge_shards_at(ssym_ctx *ctx, uint32_t n_shards, uint32_t n_targets, const double *costs_dev,
                             const uint32_t *idx_dev, const double *distance, uint32_t *out_idx_dev,
                             double *out_cost_dev)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (n_shards == 0 || !costs_dev || !idx_dev || !out_idx_dev) {
        ctx->err = "ssym_merge_shards: bad arguments";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    StageScope stageScope(ctx);
    const double *distDev = nullptr;
    if (distance && n_targets) {
        // ctx->dist is where a begin with per-target distances left them for its finish: that pair ends here
        // (finish then reports "without begin"); a begin without distances, or one whose finish is a plain match, is
        // not touched
        if (ctx->pending.valid && ctx->pending.filter && ctx->pending.has_dist)
            ctx->pending.valid = false;
        int32_t rc = ensure(ctx, ctx->dist, sizeof(double) * n_targets);
        if (rc == SSYM_OK)
            rc = stage_h2d(ctx, ctx->dist.ptr, distance, sizeof(double) * n_targets);
        if (rc != SSYM_OK)
            return rc;
        distDev = (const double *)ctx->dist.ptr;
    }
    int32_t rc = launch_merge_shards(ctx, n_shards, n_targets, costs_dev, idx_dev, distDev, out_idx_dev, out_cost_dev);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
    });
}

int32_t ssym_merge_shards(ssym_ctx *ctx, uint32_t n_shards, uint32_t n_targets, const double *costs_dev,
                          const uint32_t *idx_dev, uint32_t *out_idx_dev, double *out_cost_dev)
{
    return guarded(ctx, [&]() -> int32_t {
    return ssym_merge_shards_at(ctx, n_shards, n_targets, costs_dev, idx_dev, nullptr, out_idx_dev, out_cost_dev);
    });
}

int32_t ssym_follow_envelope(ssym_ctx *ctx, const double *samples, const uint64_t *out_offsets, uint32_t n_targets,
                             const double *ref, const uint64_t *ref_offsets, double max_gain, uint32_t flags,
                             double *out_samples, int32_t *out_pcm32, double *out_gain)
{
    return guarded(ctx, [&]() -> int32_t {
    return follow_envelope(ctx, samples, out_offsets, n_targets, ref, ref_offsets, max_gain, flags, out_samples, out_pcm32,
                           out_gain);
    });
}

}  // extern "C"
