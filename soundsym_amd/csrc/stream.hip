// stream.hip -- growing sounds: Sound::push_samples (src/sound.rs:145-164) with the analysis resident on the device
// (DESIGN.md section 5.11).
//
// An ssym_stream holds n_lanes independent sounds of one (rate, n_coeffs, f_lo, f_hi).  Per lane the device keeps the
// samples, the MFCC frames, the bits of the running max_power and the running per-coefficient sum of the frames; the
// MFCC tables are built and uploaded once, when the stream is created.  A push appends a ragged chunk (lane l gets
// samples[off[l], off[l+1])) and analyses only what the chunk completes:
//   frames   [nF, num_frames(n_new)): the per-frame body of mfcc.hip (mfcc_frame.hpp) on the lane's own samples.  The
//            first new frame starts at sample 256 nF, on the window grid, and every window is full, so frame t reads
//            the same 1024 samples as frame t of the whole sound: bit for bit ssym_mfcc of the concatenation
//   power    windows [num_windows(n_old), num_windows(n_new)) of the 128 / 64 grid, pitch.hip's arithmetic per window
//            (sequential sum of 128 squares, / 128, sqrt), folded with integer atomicMax on the bits of non-negative
//            doubles (a NaN window is skipped, as there): a maximum does not depend on order
//   sums     per (lane, coefficient) ONE thread continues acc = acc + f[t][j] over the new frames in frame order: the
//            fold of ssym_mfcc's out_mean and of sequence.hip's means kernel, merely interrupted between pushes.  No
//            floating-point atomics anywhere.
// Launches of a push: [scatter of the uploaded chunk behind the lanes' samples, when more than one lane got samples;
// one lane's chunk is copied straight behind its samples], ONE grid-stride kernel whose work items are the new frames
// of all lanes followed by the power chunks (256 windows of one lane each; an item finds its lane by a wave-uniform
// binary search over the prefix sums, as mfcc_batch_kernel does), one small kernel for the sums, [a gather of the new
// frames when the caller asked for them].  One synchronisation, at the end.  Frames and power windows cannot share a
// launch with the sums: a sum reads every new frame of its lane, which other workgroups write.
//
// Growth doubles a lane's capacity; the old block is copied on the device and released after the call's
// synchronisation through the context's deferred-free list.  Old samples are never uploaded again.
#include "ssym_internal.hpp"

namespace ssym {

constexpr int kBin = SSYM_MFCC_BIN, kHop = SSYM_MFCC_HOP, kSpec = kBin / 2 + 1;
constexpr int kMaxFilters = 130;      // n_coeffs <= 64

}  // namespace ssym

#include "mfcc_frame.hpp"

namespace ssym {
namespace {

constexpr int kPW = SSYM_POWER_WINDOW, kPH = SSYM_POWER_HOP;
constexpr int kThreads = 256, kWaves = kThreads / 64;
static_assert(kHop % kPH == 0, "a frame start lies on the power grid");

// what one call does to one lane (a lane the call leaves alone has empty ranges)
struct LaneStep {
    double *smp, *frm;          // the lane's samples and frames (DEVICE)
    uint64_t nOld, nNew;        // samples before / after
    uint64_t src;               // the lane's chunk starts here in the uploaded chunk
    uint64_t fa, fb;            // frames analysed: [fa, fb)
    uint64_t sa;                // the sums continue over frames [sa, fb), sa <= fa
    uint64_t wa, wb;            // power windows folded: [wa, wb)
};

uint64_t num_frames(uint64_t n) { return n >= (uint64_t)kBin ? (n - kBin) / kHop + 1 : 0; }
uint64_t num_power_windows(uint64_t n) { return n >= (uint64_t)kPW ? (n - kPW) / kPH + 1 : 0; }

// the last s with off[s] <= t (lanes without work hold no item); uniform over the workgroup
__device__ __forceinline__ uint32_t lane_of(const uint64_t *__restrict__ off, uint32_t n, uint64_t t)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void stream_append_kernel(const LaneStep *__restrict__ steps,
                                                                 const double *__restrict__ chunk)
{
    const LaneStep ls = steps[blockIdx.y];
    const uint64_t n = ls.nNew - ls.nOld;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads)
        ls.smp[ls.nOld + i] = chunk[ls.src + i];
}

// work items [0, F): the new frames of all lanes; [F, F + C): power chunks, 256 windows of one lane each
__global__ __launch_bounds__(kThreads) void stream_step_kernel(const LaneStep *__restrict__ steps,
                                                               const uint64_t *__restrict__ frameOff,
                                                               const uint64_t *__restrict__ chunkOff, uint32_t nLanes,
                                                               MfccTables tb, int nf, int nCoeffs,
                                                               unsigned long long *__restrict__ power)
{
    __shared__ double re[kBin], im[kBin];
    __shared__ double logE[kMaxFilters];
    const uint64_t F = frameOff[nLanes], C = chunkOff[nLanes];
    for (uint64_t t = blockIdx.x; t < F + C; t += gridDim.x) {
        if (t < F) {
            const uint32_t l = lane_of(frameOff, nLanes, t);
            const LaneStep ls = steps[l];
            const uint64_t f = ls.fa + (t - frameOff[l]);
            mfcc_frame(ls.smp, ls.nNew, f * kHop, tb, nf, nCoeffs, ls.frm + f * nCoeffs, re, im, logE);
            continue;
        }
        const uint32_t l = lane_of(chunkOff, nLanes, t - F);
        const LaneStep ls = steps[l];
        const uint64_t w = ls.wa + (t - F - chunkOff[l]) * kThreads + threadIdx.x;
        double p = 0.0;
        if (w < ls.wb) {                         // w * kPH + kPW <= nNew: the window lies inside the lane's samples
            const double *x = ls.smp + w * kPH;
            double acc = 0.0;
            for (int i = 0; i < kPW; ++i)
                acc = __dadd_rn(acc, __dmul_rn(x[i], x[i]));
            const double rms = sqrt(acc / (double)kPW);
            if (rms > p)                         // a NaN never compares greater: skipped, as by f64::max
                p = rms;
        }
        // the workgroup's maximum (non-negative, not NaN) through logE, free between frames
        for (int o = 32; o > 0; o >>= 1)
            p = fmax(p, __shfl_down(p, o));
        if ((threadIdx.x & 63) == 0)
            logE[threadIdx.x >> 6] = p;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < kWaves; ++i)
                p = fmax(p, logE[i]);
            if (p > 0.0)                         // the bits of non-negative doubles order like the doubles
                atomicMax(power + l, (unsigned long long)__double_as_longlong(p));
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void stream_sums_kernel(const LaneStep *__restrict__ steps, uint32_t nLanes,
                                                               uint32_t dim, double *__restrict__ sums)
{
    const uint64_t total = (uint64_t)nLanes * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t l = i / dim, j = i % dim;
        const LaneStep ls = steps[l];
        if (ls.sa == ls.fb)
            continue;
        double acc = sums[i];
        for (uint64_t t = ls.sa; t < ls.fb; ++t)
            acc = __dadd_rn(acc, ls.frm[t * dim + j]);
        sums[i] = acc;
    }
}

// the frames [fa, fb) of every lane, lane after lane
__global__ __launch_bounds__(kThreads) void stream_gather_kernel(const LaneStep *__restrict__ steps,
                                                                 const uint64_t *__restrict__ frameOff, uint32_t dim,
                                                                 double *__restrict__ out)
{
    const LaneStep ls = steps[blockIdx.y];
    const uint64_t n = (ls.fb - ls.fa) * dim;
    const double *src = ls.frm + ls.fa * dim;
    double *dst = out + frameOff[blockIdx.y] * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads)
        dst[i] = src[i];
}

#define SSYM_STREAM_TRY(expr)                  \
    do {                                       \
        const int32_t rc__ = (expr);           \
        if (rc__ != SSYM_OK)                   \
            return rc__;                       \
    } while (0)

struct Lane {
    double *smp = nullptr, *frm = nullptr;
    uint64_t smpCap = 0, frmCap = 0;         // samples / frames
    uint64_t nS = 0, nF = 0;
};

}  // namespace
}  // namespace ssym

struct ssym_stream {
    ssym_ctx *ctx = nullptr;
    uint32_t nLanes = 0, nc = 0;
    int nf = 0;
    ssym::HostTables ht;                     // the offsets into dTab (its host vectors are released after the upload)
    double *dTab = nullptr;
    int *dRange = nullptr;
    std::vector<ssym::Lane> lanes;
    double *dState = nullptr;                // [nLanes] max_power, then [nLanes][nc] the running sums
    char *dMeta = nullptr;                   // one call's LaneStep [nLanes], frame offsets [nLanes + 1], chunk offsets [nLanes + 1]
    double *dChunk = nullptr;                // the uploaded chunk of a push to several lanes
    uint64_t chunkCap = 0;
    std::vector<ssym::LaneStep> steps;       // host side of dMeta
    std::vector<uint64_t> offs;
};

namespace ssym {
namespace {

size_t meta_bytes(uint32_t n) { return (size_t)n * sizeof(LaneStep) + 2 * ((size_t)n + 1) * sizeof(uint64_t); }

// room for `need` values in a block that holds `used`: at least twice the old capacity, the old values copied on the
// device, the old block released after the call's synchronisation
int32_t grow(ssym_ctx *ctx, double **p, uint64_t *cap, uint64_t used, uint64_t need)
{
    if (need <= *cap)
        return SSYM_OK;
    const uint64_t want = std::max<uint64_t>(need, 2 * *cap);
    double *q = nullptr;
    if (hipMalloc((void **)&q, want * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        ctx->err = "ssym_stream: out of device memory";
        return SSYM_E_NOMEM;
    }
    if (used) {
        const hipError_t e = hipMemcpyAsync(q, *p, used * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(q);
            ctx->err = std::string("ssym_stream: ") + hipGetErrorString(e);
            return SSYM_E_HIP;
        }
    }
    if (*p)
        ctx->deferred_free.push_back(*p);
    *p = q;
    *cap = want;
    return SSYM_OK;
}

int32_t finish(ssym_ctx *ctx)
{
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    release_deferred(ctx);
    if (e != hipSuccess) {
        ctx->err = std::string("ssym_stream: ") + hipGetErrorString(e);
        return SSYM_E_HIP;
    }
    stage_finish(ctx);
    return SSYM_OK;
}

// st->steps is filled in for every lane and the lanes' blocks hold their new sizes: upload the chunk, analyse,
// hand out the new frames when asked, synchronise.  The lanes' counts are the caller's to update afterwards.
int32_t run_steps(ssym_stream *st, const double *chunk, uint64_t total, bool outDev, double *outMfccs)
{
    ssym_ctx *ctx = st->ctx;
    hipStream_t s = ctx->stream;
    const uint32_t n = st->nLanes;
    std::vector<uint64_t> &offs = st->offs;
    offs.assign(2 * ((size_t)n + 1), 0);
    uint64_t *fo = offs.data(), *co = offs.data() + n + 1;
    uint32_t fed = 0, fedLane = 0;
    uint64_t longest = 0, mostFrames = 0;
    bool sums = false;
    for (uint32_t l = 0; l < n; ++l) {
        const LaneStep &ls = st->steps[l];
        fo[l + 1] = fo[l] + (ls.fb - ls.fa);
        co[l + 1] = co[l] + (ls.wb - ls.wa + kThreads - 1) / kThreads;
        if (ls.nNew > ls.nOld) {
            ++fed;
            fedLane = l;
            longest = std::max(longest, ls.nNew - ls.nOld);
        }
        mostFrames = std::max(mostFrames, ls.fb - ls.fa);
        sums = sums || ls.sa < ls.fb;
    }
    const uint64_t F = fo[n], C = co[n];
    LaneStep *dSteps = (LaneStep *)st->dMeta;
    uint64_t *dFo = (uint64_t *)(st->dMeta + (size_t)n * sizeof(LaneStep)), *dCo = dFo + n + 1;
    if (fed > 1)
        SSYM_STREAM_TRY(grow(ctx, &st->dChunk, &st->chunkCap, 0, total));
    SSYM_STREAM_TRY(stage_h2d(ctx, dSteps, st->steps.data(), (size_t)n * sizeof(LaneStep)));
    SSYM_STREAM_TRY(stage_h2d(ctx, dFo, offs.data(), offs.size() * sizeof(uint64_t)));
    if (fed == 1) {
        const LaneStep &ls = st->steps[fedLane];
        SSYM_STREAM_TRY(stage_h2d(ctx, ls.smp + ls.nOld, chunk + ls.src, (ls.nNew - ls.nOld) * sizeof(double)));
    } else if (fed > 1) {
        SSYM_STREAM_TRY(stage_h2d(ctx, st->dChunk, chunk, total * sizeof(double)));
        const dim3 grid((unsigned)std::min<uint64_t>((longest + kThreads - 1) / kThreads, 64), n);
        stream_append_kernel<<<grid, kThreads, 0, s>>>(dSteps, st->dChunk);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    if (F + C) {
        const unsigned grid = (unsigned)std::min<uint64_t>(F + C, (uint64_t)ctx->num_cus * 16);
        stream_step_kernel<<<grid, kThreads, 0, s>>>(dSteps, dFo, dCo, n, st->ht.on(st->dTab, st->dRange), st->nf,
                                                     (int)st->nc, (unsigned long long *)st->dState);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    if (sums) {
        const uint64_t cells = (uint64_t)n * st->nc;
        stream_sums_kernel<<<(unsigned)((cells + kThreads - 1) / kThreads), kThreads, 0, s>>>(dSteps, n, st->nc,
                                                                                              st->dState + n);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    if (outMfccs && F) {
        Blocks bl(ctx);
        double *packed = outMfccs;
        if (!outDev)
            SSYM_STREAM_TRY(bl.get(&packed, F * st->nc));
        const dim3 grid((unsigned)std::min<uint64_t>((mostFrames * st->nc + kThreads - 1) / kThreads, 64), n);
        stream_gather_kernel<<<grid, kThreads, 0, s>>>(dSteps, dFo, st->nc, packed);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
        if (!outDev)
            SSYM_STREAM_TRY(stage_d2h(ctx, outMfccs, packed, F * st->nc * sizeof(double)));
        return finish(ctx);                  // (before the block goes back to the cache)
    }
    return finish(ctx);
}

int32_t check_handle(ssym_ctx *ctx, const ssym_stream *st, const char *fn)
{
    if (!ctx)
        return SSYM_E_INVALID;
    if (!st || st->ctx != ctx) {
        ctx->err = std::string(fn) + ": NULL stream, or a stream of another context";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

int32_t stream_create(ssym_ctx *ctx, uint32_t nLanes, double rate, uint32_t nc, double fLo, double fHi, uint64_t hint,
                      ssym_stream **out)
{
    const char *fn = "ssym_stream_create";
    if (!ctx)
        return SSYM_E_INVALID;
    if (!out) {
        ctx->err = std::string(fn) + ": NULL out";
        return SSYM_E_INVALID;
    }
    *out = nullptr;
    if (nLanes == 0) {
        ctx->err = std::string(fn) + ": need n_lanes >= 1";
        return SSYM_E_INVALID;
    }
    if (!std::isfinite(rate) || !mfcc_args_ok(rate, nc, fLo, fHi)) {
        ctx->err = std::string(fn) + ": need 1 <= n_coeffs <= 64, a finite sample_rate > 0, 0 <= f_lo < min(f_hi, sample_rate / 2)";
        return SSYM_E_INVALID;
    }
    if (hint > ((uint64_t)1 << 40)) {
        ctx->err = std::string(fn) + ": capacity_hint_samples beyond 2^40";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ssym_stream *st = new ssym_stream;
    st->ctx = ctx;
    st->nLanes = nLanes;
    st->nc = nc;
    build_tables(st->ht, rate, nc, fLo, fHi);
    st->nf = st->ht.nf;
    st->lanes.resize(nLanes);
    st->steps.resize(nLanes);
    const size_t stateBytes = ((size_t)nLanes + (size_t)nLanes * nc) * sizeof(double);
    hipError_t e = hipMalloc((void **)&st->dTab, st->ht.tab.size() * sizeof(double));
    if (e == hipSuccess)
        e = hipMalloc((void **)&st->dRange, st->ht.range.size() * sizeof(int));
    if (e == hipSuccess)
        e = hipMalloc((void **)&st->dState, stateBytes);
    if (e == hipSuccess)
        e = hipMalloc((void **)&st->dMeta, meta_bytes(nLanes));
    const uint64_t hintFrames = num_frames(hint);
    for (uint32_t l = 0; l < nLanes && e == hipSuccess && hint; ++l) {
        Lane &ln = st->lanes[l];
        e = hipMalloc((void **)&ln.smp, hint * sizeof(double));
        if (e == hipSuccess) {
            ln.smpCap = hint;
            if (hintFrames)
                e = hipMalloc((void **)&ln.frm, hintFrames * nc * sizeof(double));
            if (e == hipSuccess)
                ln.frmCap = hintFrames;
        }
    }
    hipStream_t s = ctx->stream;
    if (e == hipSuccess)
        e = hipMemcpyAsync(st->dTab, st->ht.tab.data(), st->ht.tab.size() * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(st->dRange, st->ht.range.data(), st->ht.range.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemsetAsync(st->dState, 0, stateBytes, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->err = std::string(fn) + ": " + hipGetErrorString(e);
        for (Lane &ln : st->lanes) {
            (void)hipFree(ln.smp);
            (void)hipFree(ln.frm);
        }
        (void)hipFree(st->dTab);
        (void)hipFree(st->dRange);
        (void)hipFree(st->dState);
        (void)hipFree(st->dMeta);
        delete st;
        return e == hipErrorOutOfMemory ? SSYM_E_NOMEM : SSYM_E_HIP;
    }
    std::vector<double>().swap(st->ht.tab);
    std::vector<int>().swap(st->ht.range);
    *out = st;
    return SSYM_OK;
}

// a step that leaves every lane as it is
void idle_steps(ssym_stream *st)
{
    for (uint32_t l = 0; l < st->nLanes; ++l) {
        const Lane &ln = st->lanes[l];
        const uint64_t w = num_power_windows(ln.nS);
        st->steps[l] = LaneStep{ln.smp, ln.frm, ln.nS, ln.nS, 0, ln.nF, ln.nF, ln.nF, w, w};
    }
}

int32_t stream_push(ssym_ctx *ctx, ssym_stream *st, const double *samples, const uint64_t *off, uint32_t flags,
                    uint64_t *outNewFrames, double *outMfccs)
{
    const char *fn = "ssym_stream_push";
    SSYM_STREAM_TRY(check_handle(ctx, st, fn));
    if (!off) {
        ctx->err = std::string(fn) + ": NULL sample_offsets";
        return SSYM_E_INVALID;
    }
    const uint32_t n = st->nLanes;
    for (uint32_t l = 0; l < n; ++l)
        if (off[l + 1] < off[l]) {
            ctx->err = std::string(fn) + ": sample_offsets must not decrease";
            return SSYM_E_INVALID;
        }
    const uint64_t base = off[0], total = off[n] - base;
    if (total && !samples) {
        ctx->err = std::string(fn) + ": NULL samples";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    StageScope scope(ctx);
    // room first: a lane's block only ever grows, and growing keeps what it holds
    for (uint32_t l = 0; l < n; ++l) {
        Lane &ln = st->lanes[l];
        const uint64_t nNew = ln.nS + (off[l + 1] - off[l]);
        SSYM_STREAM_TRY(grow(ctx, &ln.smp, &ln.smpCap, ln.nS, nNew));
        SSYM_STREAM_TRY(grow(ctx, &ln.frm, &ln.frmCap, ln.nF * st->nc, num_frames(nNew) * st->nc));
    }
    for (uint32_t l = 0; l < n; ++l) {
        const Lane &ln = st->lanes[l];
        const uint64_t nNew = ln.nS + (off[l + 1] - off[l]);
        st->steps[l] = LaneStep{ln.smp,      ln.frm, ln.nS, nNew, off[l] - base, ln.nF, std::max(ln.nF, num_frames(nNew)),
                                ln.nF,       num_power_windows(ln.nS), num_power_windows(nNew)};
    }
    SSYM_STREAM_TRY(run_steps(st, samples ? samples + base : nullptr, total, (flags & SSYM_OUT_DEVICE) != 0, outMfccs));
    for (uint32_t l = 0; l < n; ++l) {
        const LaneStep &ls = st->steps[l];
        if (outNewFrames)
            outNewFrames[l] = ls.fb - ls.fa;
        st->lanes[l].nS = ls.nNew;
        st->lanes[l].nF = ls.fb;
    }
    return SSYM_OK;
}

int32_t stream_seed(ssym_ctx *ctx, ssym_stream *st, uint32_t lane, const double *samples, uint64_t nSamples,
                    const double *mfccs, uint64_t nFrames)
{
    const char *fn = "ssym_stream_seed";
    SSYM_STREAM_TRY(check_handle(ctx, st, fn));
    if (lane >= st->nLanes) {
        ctx->err = std::string(fn) + ": lane out of range";
        return SSYM_E_INVALID;
    }
    Lane &ln = st->lanes[lane];
    if (ln.nS || ln.nF) {
        ctx->err = std::string(fn) + ": the lane is not empty (ssym_stream_reset empties it)";
        return SSYM_E_INVALID;
    }
    if (nSamples && !samples) {
        ctx->err = std::string(fn) + ": NULL samples";
        return SSYM_E_INVALID;
    }
    const uint64_t full = num_frames(nSamples);
    if (mfccs && nFrames > full) {
        ctx->err = std::string(fn) + ": more frames than the samples allow (ssym_mfcc_num_frames)";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    StageScope scope(ctx);
    SSYM_STREAM_TRY(grow(ctx, &ln.smp, &ln.smpCap, 0, nSamples));
    SSYM_STREAM_TRY(grow(ctx, &ln.frm, &ln.frmCap, 0, full * st->nc));
    idle_steps(st);
    const uint64_t have = mfccs ? nFrames : 0;       // adopted as given; the rest is left to the next push
    if (have)
        SSYM_STREAM_TRY(stage_h2d(ctx, ln.frm, mfccs, have * st->nc * sizeof(double)));
    st->steps[lane] = LaneStep{ln.smp, ln.frm, 0, nSamples, 0, have, mfccs ? have : full, 0, 0,
                               num_power_windows(nSamples)};
    SSYM_STREAM_TRY(run_steps(st, samples, nSamples, false, nullptr));
    ln.nS = nSamples;
    ln.nF = st->steps[lane].fb;
    return SSYM_OK;
}

int32_t stream_read(ssym_ctx *ctx, ssym_stream *st, uint32_t lane, uint64_t first, uint64_t count, uint32_t flags,
                    double *out)
{
    const char *fn = "ssym_stream_read";
    SSYM_STREAM_TRY(check_handle(ctx, st, fn));
    if (lane >= st->nLanes) {
        ctx->err = std::string(fn) + ": lane out of range";
        return SSYM_E_INVALID;
    }
    const Lane &ln = st->lanes[lane];
    if (first > ln.nF || count > ln.nF - first) {
        ctx->err = std::string(fn) + ": frames beyond the lane's frame count";
        return SSYM_E_INVALID;
    }
    if (count == 0)
        return SSYM_OK;
    if (!out) {
        ctx->err = std::string(fn) + ": NULL out_mfccs";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    StageScope scope(ctx);
    const double *src = ln.frm + first * st->nc;
    const size_t bytes = count * st->nc * sizeof(double);
    if (flags & SSYM_OUT_DEVICE)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    else
        SSYM_STREAM_TRY(stage_d2h(ctx, out, src, bytes));
    return finish(ctx);
}

int32_t stream_descriptors(ssym_ctx *ctx, ssym_stream *st, double *outPower, double *outMean)
{
    SSYM_STREAM_TRY(check_handle(ctx, st, "ssym_stream_descriptors"));
    if (!outPower && !outMean)
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t n = st->nLanes, nc = st->nc;
    std::vector<double> state((size_t)n + (size_t)n * nc);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(state.data(), st->dState, state.size() * sizeof(double), hipMemcpyDeviceToHost,
                                       ctx->stream));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t l = 0; l < n; ++l) {
        if (outPower)
            outPower[l] = state[l];
        if (!outMean)
            continue;
        // analyze_mean_mfccs (src/sound.rs:271-286): the sum over the frames, then / T; 0 / 0 without frames
        const uint64_t T = st->lanes[l].nF;
        for (uint32_t j = 0; j < nc; ++j)
            outMean[(size_t)l * nc + j] = T ? state[n + (size_t)l * nc + j] / (double)T : std::nan("");
    }
    return SSYM_OK;
}

int32_t stream_reset(ssym_ctx *ctx, ssym_stream *st, uint32_t lane)
{
    const char *fn = "ssym_stream_reset";
    SSYM_STREAM_TRY(check_handle(ctx, st, fn));
    if (lane >= st->nLanes) {
        ctx->err = std::string(fn) + ": lane out of range";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    SSYM_STREAM_TRY(zero_words(ctx, st->dState + lane, sizeof(double)));
    SSYM_STREAM_TRY(zero_words(ctx, st->dState + st->nLanes + (size_t)lane * st->nc, st->nc * sizeof(double)));
    st->lanes[lane].nS = st->lanes[lane].nF = 0;
    return SSYM_OK;
}

}  // namespace

// what ssym_spotter_follow (dtw_spotter.hip) checks a stream against; the frames it reads come through
// ssym_stream_frames_device
void stream_shape(const ssym_stream *st, uint32_t *n_lanes, uint32_t *n_coeffs, const ssym_ctx **ctx)
{
    *n_lanes = st->nLanes;
    *n_coeffs = st->nc;
    *ctx = st->ctx;
}

}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_stream_create(ssym_ctx *ctx, uint32_t n_lanes, double sample_rate, uint32_t n_coeffs, double f_lo,
                           double f_hi, uint64_t capacity_hint_samples, ssym_stream **out)
{
    return guarded(ctx, [&]() -> int32_t {
        return stream_create(ctx, n_lanes, sample_rate, n_coeffs, f_lo, f_hi, capacity_hint_samples, out);
    });
}

int32_t ssym_stream_destroy(ssym_ctx *ctx, ssym_stream *st)
{
    return guarded(ctx, [&]() -> int32_t {
        if (!st)
            return SSYM_OK;
        SSYM_STREAM_TRY(check_handle(ctx, st, "ssym_stream_destroy"));
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        release_deferred(ctx);
        for (Lane &ln : st->lanes) {
            (void)hipFree(ln.smp);
            (void)hipFree(ln.frm);
        }
        (void)hipFree(st->dTab);
        (void)hipFree(st->dRange);
        (void)hipFree(st->dState);
        (void)hipFree(st->dMeta);
        (void)hipFree(st->dChunk);
        delete st;
        return SSYM_OK;
    });
}

int32_t ssym_stream_push(ssym_ctx *ctx, ssym_stream *st, const double *samples, const uint64_t *sample_offsets,
                         uint32_t flags, uint64_t *out_new_frames, double *out_mfccs)
{
    return guarded(ctx, [&]() -> int32_t {
        return stream_push(ctx, st, samples, sample_offsets, flags, out_new_frames, out_mfccs);
    });
}

int32_t ssym_stream_seed(ssym_ctx *ctx, ssym_stream *st, uint32_t lane, const double *samples, uint64_t n_samples,
                         const double *mfccs, uint64_t n_frames)
{
    return guarded(ctx, [&]() -> int32_t { return stream_seed(ctx, st, lane, samples, n_samples, mfccs, n_frames); });
}

int32_t ssym_stream_counts(const ssym_stream *st, uint64_t *out_n_samples, uint64_t *out_n_frames)
{
    if (!st)
        return SSYM_E_INVALID;
    for (uint32_t l = 0; l < st->nLanes; ++l) {
        if (out_n_samples)
            out_n_samples[l] = st->lanes[l].nS;
        if (out_n_frames)
            out_n_frames[l] = st->lanes[l].nF;
    }
    return SSYM_OK;
}

int32_t ssym_stream_read(ssym_ctx *ctx, ssym_stream *st, uint32_t lane, uint64_t first_frame, uint64_t n_frames,
                         uint32_t flags, double *out_mfccs)
{
    return guarded(ctx, [&]() -> int32_t {
        return stream_read(ctx, st, lane, first_frame, n_frames, flags, out_mfccs);
    });
}

int32_t ssym_stream_frames_device(const ssym_stream *st, uint32_t lane, const double **out_ptr, uint64_t *out_n_frames)
{
    if (!st || lane >= st->nLanes || !out_ptr || !out_n_frames)
        return SSYM_E_INVALID;
    *out_ptr = st->lanes[lane].frm;
    *out_n_frames = st->lanes[lane].nF;
    return SSYM_OK;
}

int32_t ssym_stream_samples_device(const ssym_stream *st, uint32_t lane, const double **out_ptr,
                                   uint64_t *out_n_samples)
{
    if (!st || lane >= st->nLanes || !out_ptr || !out_n_samples)
        return SSYM_E_INVALID;
    *out_ptr = st->lanes[lane].smp;
    *out_n_samples = st->lanes[lane].nS;
    return SSYM_OK;
}

int32_t ssym_stream_descriptors(ssym_ctx *ctx, ssym_stream *st, double *out_max_power, double *out_mean)
{
    return guarded(ctx, [&]() -> int32_t { return stream_descriptors(ctx, st, out_max_power, out_mean); });
}

int32_t ssym_stream_reset(ssym_ctx *ctx, ssym_stream *st, uint32_t lane)
{
    return guarded(ctx, [&]() -> int32_t { return stream_reset(ctx, st, lane); });
}

}  // extern "C"
