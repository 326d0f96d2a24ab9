// follower.hip -- live envelope following: loudness tracking, push by push (DESIGN.md 2 "Live envelope following", 5.29; the
// header carries the definition, tests/live_follow_ref.py restates it).
//
// Role on the path: ssym_follow_envelope (follow.hip) is a post-pass over whole targets.  A follower is its resumable form,
// lane by lane, as a resynthesiser is the offline render's: a lane receives the resynthesis y and the reference x as they
// grow, in any amounts, and releases every output hop as soon as its bits can no longer change.  From reset to flush a
// lane's samples and gains are ssym_follow_envelope's for (y[0 .. ny), x[0 .. nx)), bit for bit.
//
// Release (follower_plan.hpp holds the arithmetic; nothing here decides a count): with h = floor(min(ny, nx) / HOP), boundary
// b is settled when (b + 2) HOP <= min(ny, nx) and hop j is released when boundaries j and j + 1 are settled.  A settled
// boundary's window [(b - 2) HOP, (b + 2) HOP) lies wholly below both counts: no later sample and no later n enters its sum.
// The flush settles every boundary up to J = ceil(ny / HOP) with the offline clipping and releases the rest of y.
//
// State: per lane and signal a ring of samples indexed by absolute sample index modulo a power-of-two capacity shared by the
// lanes; it holds the lane from two hops below its first unreleased hop.  g(r), the gain at the first unreleased hop, sits
// in the lane's record: the boundary is settled a call before the hop leaves.
//
// Mapping.
//   append   follower_append_kernel, one thread per sample, the lanes on the grid's y: the call's new y and x into the rings,
//            from the staged upload or from the caller's device arrays.
//   gain     follower_gain_kernel, one workgroup per entry of the plan's block table (lane, first boundary, count <= 32):
//            follow_gain_kernel's layout (follow_common.hpp) staged from the rings, +0.0 for k < 0, k >= ny and for x at
//            k >= min(nx, ny), the bound tested before the load; wave 0 runs follow_chain and follow_gain.
//   apply    follower_apply_kernel, a workgroup per (lane, 4096 released samples): follow_sample over the ring into the call's
//            sample log (a LaneLog, one entry per sample) beside the gain log.  Only the lane's first workgroup reads g(r) from
//            the record, and it alone writes the next one there, behind a barrier.
// No atomics, no workgroup waits on another; stream order is the only ordering between kernels.  One synchronisation per
// push or flush.
#include "follow_common.hpp"
#include "follower_plan.hpp"
#include "lane_feed.hpp"

namespace ssym {

static_assert(kFollowerHop == (uint64_t)kWarpHop && kFollowerBlock == (uint32_t)kFollowBlock && kFollowerMaxLen == kFollowMaxLen &&
                  kFollowerLook + 2 == (uint64_t)kWarpTaps,
              "the plan and the kernels speak of the same hops, blocks and limits");

struct FwRegrow {
    uint64_t from, ny, nx;       // the lane holds [from, ny) of y and [from, nx) of x
};

}  // namespace ssym

struct ssym_follower {
    ssym_ctx *ctx = nullptr;
    uint32_t nLanes = 0;
    double maxGain = 0.0;
    std::vector<ssym::FollowerLane> lanes;       // host: everything the plan needs
    std::vector<uint64_t> consumed;              // ny per lane (what lane_feed.hpp's lane check looks at)
    std::vector<uint8_t> ended;
    // device
    double *ringY = nullptr, *ringX = nullptr;   // [nLanes][cap]
    uint64_t cap = 0;
    double *gPrev = nullptr;                     // [nLanes]: g(r) of the lane's first unreleased hop
    double *win = nullptr;                       // [1024]
    ssym::FollowerStep *dSteps = nullptr;        // [nLanes]
    // the logs of the last push / flush: samples (cost: f64, word 0: pcm), one entry per sample; the gains settled
    ssym::LaneLog out{1};
    double *gains = nullptr;
    uint64_t gainCap = 0;
    std::vector<uint64_t> gainOff;               // [nLanes + 1]
};

namespace ssym {
namespace {

constexpr const char *kNoun = "follower";

struct FwArgs {
    const FollowerStep *steps;
    const FollowerBlockEntry *table;
    double *ringY, *ringX;
    uint64_t cap;                // a power of two
    const double *y, *x;         // the call's new samples (DEVICE)
    const double *win;
    double *gPrev;
    double maxGain;
    double *gain;                // the gain log
    double *out;                 // the sample log
    int32_t *pcm;
};

// grid (blocks of 256 samples, lanes)
__global__ __launch_bounds__(256) void follower_append_kernel(const FwArgs a)
{
    const uint32_t l = blockIdx.y;
    const FollowerStep s = a.steps[l];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, mask = a.cap - 1;
    if (i < s.my)
        a.ringY[(size_t)l * a.cap + ((s.ny - s.my + i) & mask)] = a.y[s.yAt + i];
    if (i < s.mx)
        a.ringX[(size_t)l * a.cap + ((s.nx - s.mx + i) & mask)] = a.x[s.xAt + i];
}

__global__ __launch_bounds__(256) void follower_gain_kernel(const FwArgs a)
{
    extern __shared__ double sm[];               // [1024] the window, then [2][hops][257]: y's span, then x's
    const FollowerBlockEntry e = a.table[blockIdx.x];
    const FollowerStep st = a.steps[e.lane];
    const uint64_t ny = st.ny, nxy = st.nx < st.ny ? st.nx : st.ny, mask = a.cap - 1;
    const int nb = (int)e.count;
    const int hops = nb + kWarpTaps - 1;
    double *sw = sm, *sy = sm + kWarpBin, *sx = sy + hops * kFollowPitch;
    const int tid = (int)threadIdx.x;
    const double *__restrict__ y = a.ringY + (size_t)e.lane * a.cap;
    const double *__restrict__ x = a.ringX + (size_t)e.lane * a.cap;
#pragma unroll
    for (int q = 0; q < kWarpTaps; ++q)
        sw[tid + 256 * q] = a.win[tid + 256 * q];
    // twelve hops of both signals in flight per thread, as follow_gain_kernel
    constexpr int G = 12;
    for (int i0 = 0; i0 < hops; i0 += G) {
        double vy[G], vx[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int64_t k = ((int64_t)e.first - 2 + i0 + u) * kWarpHop + tid;
            const bool in = i0 + u < hops && k >= 0 && (uint64_t)k < ny;     // tested before the loads: the ring holds [from, ny) / [from, nx)
            vy[u] = in ? y[(uint64_t)k & mask] : 0.0;
            vx[u] = (in && (uint64_t)k < nxy) ? x[(uint64_t)k & mask] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < G; ++u)
            if (i0 + u < hops) {
                sy[(i0 + u) * kFollowPitch + tid] = vy[u];
                sx[(i0 + u) * kFollowPitch + tid] = vx[u];
            }
    }
    __syncthreads();
    if (tid >= 64)
        return;
    const int sig = tid >> 5, bl = tid & 31;
    // a lane past the block's last boundary repeats it: reads stay in the staged span
    const double *s = (sig ? sx : sy) + std::min(bl, nb - 1) * kFollowPitch;
    const double acc = follow_chain(s, sw);
    const double ex = __shfl(acc, bl + 32, 64);
    if (sig == 0 && bl < nb)
        a.gain[st.gainAt + ((uint64_t)e.first - st.setFirst) + (uint32_t)bl] = follow_gain(ex, acc, a.maxGain);
}

// grid (chunks of 4096 released samples, at least one; lanes)
__global__ __launch_bounds__(256) void follower_apply_kernel(const FwArgs a)
{
    __shared__ double sG[kWarpChunk / kWarpHop + 1];
    const uint32_t l = blockIdx.y;
    const FollowerStep st = a.steps[l];
    const uint64_t c0 = (uint64_t)blockIdx.x * kWarpChunk;
    if ((c0 >= st.relCount && blockIdx.x) || (st.relCount == 0 && st.setCount == 0))
        return;                                  // the whole workgroup: nothing of this lane in the chunk
    const uint32_t tid = threadIdx.x;
    if (tid < (uint32_t)(kWarpChunk / kWarpHop + 1)) {
        // a released hop starts on a hop: boundary b is the gain at the chunk's hop tid
        const uint64_t b = (st.relFirst + c0) / kWarpHop + tid;
        double g = 0.0;                          // beyond the settled: no sample of the chunk asks for it
        if (b < st.setFirst)
            g = a.gPrev[l];                      // b = r = setFirst - 1: the lane's first workgroup, its thread 0 alone
        else if (b < st.setFirst + st.setCount)
            g = a.gain[st.gainAt + (b - st.setFirst)];
        sG[tid] = g;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0 && st.setCount)
        a.gPrev[l] = a.gain[st.gainAt + st.setCount - 1];       // g(r) of the next call: its first unreleased hop's, or a later one
    const double f = (double)tid / 256.0, fm = 1.0 - f;         // both exact
    const uint64_t mask = a.cap - 1;
    const double *__restrict__ y = a.ringY + (size_t)l * a.cap;
#pragma unroll
    for (int u = 0; u < 16; u += 4) {
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t k = c0 + tid + (uint64_t)(u + q) * 256;
            v[q] = k < st.relCount ? y[(st.relFirst + k) & mask] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t k = c0 + tid + (uint64_t)(u + q) * 256;
            if (k >= st.relCount)
                continue;
            const double r = follow_sample(v[q], sG[u + q], sG[u + q + 1], f, fm);
            a.out[st.outAt + k] = r;
            a.pcm[st.outAt + k] = warp_pcm32(r);
        }
    }
}

// what the lanes hold, from rings of oldCap samples into rings of newCap; grid (blocks, lanes)
__global__ __launch_bounds__(256) void follower_regrow_kernel(const FwRegrow *held, uint64_t oldCap, uint64_t newCap, const double *oldY,
                                                              const double *oldX, double *newY, double *newX)
{
    const uint32_t l = blockIdx.y;
    const FwRegrow h = held[l];
    const uint64_t top = h.ny > h.nx ? h.ny : h.nx;
    for (uint64_t k = h.from + (uint64_t)blockIdx.x * 256 + threadIdx.x; k < top; k += (uint64_t)gridDim.x * 256) {
        if (k < h.ny)
            newY[(size_t)l * newCap + (k & (newCap - 1))] = oldY[(size_t)l * oldCap + (k & (oldCap - 1))];
        if (k < h.nx)
            newX[(size_t)l * newCap + (k & (newCap - 1))] = oldX[(size_t)l * oldCap + (k & (oldCap - 1))];
    }
}

void follower_free(ssym_ctx *ctx, ssym_follower *fl)
{
    for (void *p : {(void *)fl->ringY, (void *)fl->ringX, (void *)fl->gPrev, (void *)fl->win, (void *)fl->dSteps, (void *)fl->gains})
        if (p)
            dev_free(ctx, p);
    fl->out.free(ctx);
    delete fl;
}

LaneFeed feed_of(const ssym_follower *fl)
{
    return LaneFeed{kNoun, "out_n_samples", fl->nLanes, 0, fl->consumed, &fl->ended, false, nullptr};
}

int32_t refuse(ssym_ctx *ctx, const char *fn, const std::string &what, int32_t rc = SSYM_E_INVALID)
{
    ctx->err = fn + (": " + what);
    return rc;
}

int32_t follower_create(ssym_ctx *ctx, uint32_t n_lanes, double max_gain, ssym_follower **out)
{
    const char *fn = "ssym_follower_create";
    if (!out)
        return refuse(ctx, fn, "out is NULL");
    *out = nullptr;
    if (!(max_gain >= 1.0) || std::isinf(max_gain))
        return refuse(ctx, fn, "max_gain must be a finite number, 1 or more");
    if (n_lanes == 0)
        return refuse(ctx, fn, "n_lanes is 0");
    if (n_lanes > kFollowerMaxLanes)
        return refuse(ctx, fn, "more than " + std::to_string(kFollowerMaxLanes) + " lanes", SSYM_E_UNSUPPORTED);
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ssym_follower *fl = new ssym_follower;
    fl->ctx = ctx;
    fl->nLanes = n_lanes;
    fl->maxGain = max_gain;
    fl->lanes.assign(n_lanes, FollowerLane{});
    fl->consumed.assign(n_lanes, 0);
    fl->ended.assign(n_lanes, 0);
    fl->gainOff.assign((size_t)n_lanes + 1, 0);
    fl->out.off.assign((size_t)n_lanes + 1, 0);
    fl->out.count.assign(n_lanes, 0);
    fl->cap = kFollowerRingMin;
    int32_t rc = alloc_n(ctx, &fl->ringY, (size_t)n_lanes * fl->cap);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &fl->ringX, (size_t)n_lanes * fl->cap);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &fl->gPrev, (size_t)n_lanes);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &fl->win, (size_t)kWarpBin);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &fl->dSteps, (size_t)n_lanes);
    if (rc != SSYM_OK) {
        follower_free(ctx, fl);
        return rc;
    }
    hipError_t e = hipMemcpyAsync(fl->win, warp_window().data(), sizeof(double) * kWarpBin, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(fl->gPrev, 0, sizeof(double) * n_lanes, ctx->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->err = std::string(fn) + ": " + hipGetErrorString(e);
        follower_free(ctx, fl);
        return SSYM_E_HIP;
    }
    *out = fl;
    return SSYM_OK;
}

// rings of newCap samples, what the lanes hold moved over device to device
int32_t follower_regrow(ssym_ctx *ctx, ssym_follower *fl, uint64_t newCap, Blocks &bl)
{
    const uint32_t nL = fl->nLanes;
    double *y = nullptr, *x = nullptr;
    FwRegrow *dHeld = nullptr;
    int32_t rc = bl.get(&dHeld, (size_t)nL);
    if (rc != SSYM_OK)
        return rc;
    rc = alloc_n(ctx, &y, (size_t)nL * newCap);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &x, (size_t)nL * newCap);
    if (rc != SSYM_OK) {
        if (y)
            dev_free(ctx, y);
        return rc;
    }
    // the old rings live until the call's synchronisation: the regrow kernel reads them
    bl.list.push_back(fl->ringY);
    bl.list.push_back(fl->ringX);
    std::vector<FwRegrow> held(nL);
    uint64_t most = 0;
    for (uint32_t l = 0; l < nL; ++l) {
        const FollowerLane &ln = fl->lanes[l];
        held[l] = ln.ended ? FwRegrow{0, 0, 0} : FwRegrow{follower_held_from(ln), ln.ny, ln.nx};
        most = std::max(most, std::max(held[l].ny, held[l].nx) - held[l].from);
    }
    const double *oldY = fl->ringY, *oldX = fl->ringX;
    const uint64_t oldCap = fl->cap;
    fl->ringY = y;
    fl->ringX = x;
    fl->cap = newCap;
    if (!most)
        return SSYM_OK;
    // (pageable host memory: the copy has left `held` when the call returns)
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dHeld, held.data(), sizeof(FwRegrow) * nL, hipMemcpyHostToDevice, ctx->stream));
    const unsigned blocks = (unsigned)std::min<uint64_t>((most + 255) / 256, 64);
    follower_regrow_kernel<<<dim3(blocks, nL), 256, 0, ctx->stream>>>(dHeld, oldCap, newCap, oldY, oldX, y, x);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

// The body of push and flush: runs the plan.  y / x: the call's new samples (DEVICE).
int32_t follower_run(ssym_ctx *ctx, ssym_follower *fl, const FollowerPlan &p, const double *y, const double *x, uint32_t flushLane,
                     Blocks &bl, uint64_t *out_n_samples)
{
    const uint32_t nL = fl->nLanes;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    int32_t rc = SSYM_OK;
    if (p.ringCap > fl->cap) {
        rc = follower_regrow(ctx, fl, p.ringCap, bl);
        if (rc != SSYM_OK)
            return rc;
    }
    rc = fl->out.room(ctx, p.samples);
    if (rc != SSYM_OK)
        return rc;
    if (p.gains > fl->gainCap) {
        const uint64_t grown = pow2_at_least(std::max<uint64_t>(p.gains, 256));
        double *g = nullptr;
        rc = alloc_n(ctx, &g, (size_t)grown);
        if (rc != SSYM_OK)
            return rc;
        if (fl->gains)
            dev_free(ctx, fl->gains);            // (every call ends synchronised: no kernel reads the old log)
        fl->gains = g;
        fl->gainCap = grown;
    }
    FollowerBlockEntry *dTable = nullptr;
    if (!p.table.empty()) {
        rc = bl.get(&dTable, p.table.size());
        if (rc != SSYM_OK)
            return rc;
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dTable, p.table.data(), sizeof(FollowerBlockEntry) * p.table.size(), hipMemcpyHostToDevice, st));
    }
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(fl->dSteps, p.steps.data(), sizeof(FollowerStep) * nL, hipMemcpyHostToDevice, st));
    const FwArgs k{fl->dSteps, dTable, fl->ringY, fl->ringX, fl->cap, y, x, fl->win, fl->gPrev,
                   fl->maxGain, fl->gains, fl->out.cost, (int32_t *)fl->out.word(0)};
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    if (p.maxAppend) {
        follower_append_kernel<<<dim3((unsigned)((p.maxAppend + 255) / 256), nL), 256, 0, st>>>(k);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    if (!p.table.empty()) {
        const size_t lds = follow_lds_doubles(p.maxBlock) * sizeof(double);
        if (lds > 64 * 1024)
            SSYM_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)follower_gain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        follower_gain_kernel<<<dim3((unsigned)p.table.size()), 256, lds, st>>>(k);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    if (p.gains || p.samples) {
        const unsigned chunks = (unsigned)std::max<uint64_t>((p.maxReleased + kWarpChunk - 1) / kWarpChunk, 1);
        follower_apply_kernel<<<dim3(chunks, nL), 256, 0, st>>>(k);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    follower_commit(fl->lanes, p, flushLane);
    for (uint32_t l = 0; l < nL; ++l) {
        fl->consumed[l] = fl->lanes[l].ny;
        fl->ended[l] = fl->lanes[l].ended;
        fl->out.off[l] = p.steps[l].outAt;
        fl->out.count[l] = p.steps[l].relCount;
        fl->gainOff[l] = p.steps[l].gainAt;
    }
    fl->out.off[nL] = p.samples;
    fl->gainOff[nL] = p.gains;
    *out_n_samples = p.samples;
    ssym_timings tm{};
    tm.main_ms = ev_ms(ev[1], ev[2]);                            // the gain kernel
    tm.reduce_ms = ev_ms(ev[0], ev[1]) + ev_ms(ev[2], ev[3]);    // append and apply
    tm.total_ms = ev_ms(ev[0], ev[3]);
    tm.main_launches = p.table.empty() ? 0 : 1;
    tm.n_pairs = p.gains;                                        // boundaries settled
    ctx->timings = tm;
    return SSYM_OK;
}

int32_t follower_push(ssym_ctx *ctx, ssym_follower *fl, const double *samples, const uint64_t *sample_offsets, const double *ref,
                      const uint64_t *ref_offsets, uint32_t flags, uint64_t *out_n_samples)
{
    const char *fn = "ssym_follower_push";
    int32_t rc = check_handle(ctx, fl, kNoun, fn);
    if (rc != SSYM_OK)
        return rc;
    if (flags & ~(uint32_t)(SSYM_FOLLOW_SAMPLES_DEVICE | SSYM_FOLLOW_REF_DEVICE))
        return refuse(ctx, fn, "unknown flag bits");
    if (!sample_offsets || !ref_offsets || !out_n_samples)
        return refuse(ctx, fn, "sample_offsets, ref_offsets and out_n_samples must not be NULL");
    if (sample_offsets[0] != 0 || ref_offsets[0] != 0)
        return refuse(ctx, fn, "sample_offsets and ref_offsets must start at 0");
    const uint32_t nL = fl->nLanes;
    for (uint32_t l = 0; l < nL; ++l) {
        if (sample_offsets[l + 1] < sample_offsets[l] || ref_offsets[l + 1] < ref_offsets[l])
            return refuse(ctx, fn, "sample_offsets or ref_offsets decrease (lane " + std::to_string(l) + ")");
        const uint64_t my = sample_offsets[l + 1] - sample_offsets[l], mx = ref_offsets[l + 1] - ref_offsets[l];
        if ((my || mx) && fl->lanes[l].ended)
            return refuse(ctx, fn, "lane " + std::to_string(l) + " was flushed and has ended; call ssym_follower_reset");
        if (my >= kFollowerMaxLen || mx >= kFollowerMaxLen || fl->lanes[l].ny + my >= kFollowerMaxLen ||
            fl->lanes[l].nx + mx >= kFollowerMaxLen)
            return refuse(ctx, fn, "lane " + std::to_string(l) + " would consume 2^40 samples or more of a signal", SSYM_E_UNSUPPORTED);
    }
    const FollowerPlan p = follower_plan(fl->lanes, sample_offsets, ref_offsets, kFollowerNoLane);
    if (!follower_ring_fits(p.ringCap, nL))
        return refuse(ctx, fn, "the lanes would hold more samples than the follower's rings may (" + std::to_string(kFollowerRingBytes >> 20) +
                                   " MiB for both signals of all lanes); feed both signals evenly, or in smaller amounts",
                      SSYM_E_UNSUPPORTED);
    const uint64_t total = sample_offsets[nL], refTotal = ref_offsets[nL];
    if ((total && !samples) || (refTotal && !ref))
        return refuse(ctx, fn, "samples and ref must not be NULL while they hold samples");
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    Blocks bl(ctx);
    const double *dY = samples, *dX = ref;
    if (total && !(flags & SSYM_FOLLOW_SAMPLES_DEVICE)) {
        double *d = nullptr;
        rc = bl.get(&d, (size_t)total);
        if (rc != SSYM_OK)
            return rc;
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(d, samples, sizeof(double) * total, hipMemcpyHostToDevice, ctx->stream));
        dY = d;
    }
    if (refTotal && !(flags & SSYM_FOLLOW_REF_DEVICE)) {
        double *d = nullptr;
        rc = bl.get(&d, (size_t)refTotal);
        if (rc != SSYM_OK)
            return rc;
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(d, ref, sizeof(double) * refTotal, hipMemcpyHostToDevice, ctx->stream));
        dX = d;
    }
    return follower_run(ctx, fl, p, dY, dX, kFollowerNoLane, bl, out_n_samples);
}

int32_t follower_flush(ssym_ctx *ctx, ssym_follower *fl, uint32_t lane, uint64_t *out_n_samples)
{
    const char *fn = "ssym_follower_flush";
    int32_t rc = check_handle(ctx, fl, kNoun, fn);
    if (rc != SSYM_OK)
        return rc;
    if (lane >= fl->nLanes || !out_n_samples)
        return refuse(ctx, fn, "lane outside the follower's lanes, or out_n_samples is NULL");
    if (fl->lanes[lane].ended)
        return refuse(ctx, fn, "lane " + std::to_string(lane) + " was flushed and has ended; call ssym_follower_reset");
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    Blocks bl(ctx);
    const FollowerPlan p = follower_plan(fl->lanes, nullptr, nullptr, lane);
    return follower_run(ctx, fl, p, nullptr, nullptr, lane, bl, out_n_samples);
}

int32_t follower_reset(ssym_ctx *ctx, ssym_follower *fl, uint32_t lane)
{
    const char *fn = "ssym_follower_reset";
    int32_t rc = check_handle(ctx, fl, kNoun, fn);
    if (rc == SSYM_OK)
        rc = feed_of(fl).lane(ctx, fn, lane, false, nullptr);
    if (rc != SSYM_OK)
        return rc;
    // nothing of the lane on the device outlives it: a lane that has released nothing reads neither its ring nor its record
    fl->lanes[lane] = FollowerLane{};
    fl->consumed[lane] = 0;
    fl->ended[lane] = 0;
    return SSYM_OK;
}

int32_t follower_samples(ssym_ctx *ctx, const ssym_follower *fl, uint64_t *out_lane_offsets, double *out_samples, int32_t *out_pcm32,
                         uint64_t *out_gain_offsets, double *out_gain, uint32_t flags)
{
    const char *fn = "ssym_follower_samples";
    int32_t rc = check_handle(ctx, fl, kNoun, fn);
    if (rc != SSYM_OK)
        return rc;
    if (flags & ~(uint32_t)SSYM_OUT_DEVICE)
        return refuse(ctx, fn, "unknown flag bits");
    if (out_lane_offsets)
        std::copy(fl->out.off.begin(), fl->out.off.end(), out_lane_offsets);
    if (out_gain_offsets)
        std::copy(fl->gainOff.begin(), fl->gainOff.end(), out_gain_offsets);
    const uint64_t total = fl->out.off[fl->nLanes], nGains = fl->gainOff[fl->nLanes];
    if ((!total || (!out_samples && !out_pcm32)) && (!nGains || !out_gain))
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;
    // the plan packs the lanes' stretches one behind the other: each log leaves in one copy
    rc = copy_out(ctx, out_samples, (const double *)fl->out.cost, (size_t)total, outDev);
    if (rc == SSYM_OK)
        rc = copy_out(ctx, out_pcm32, (const int32_t *)fl->out.word(0), (size_t)total, outDev);
    if (rc == SSYM_OK)
        rc = copy_out(ctx, out_gain, (const double *)fl->gains, (size_t)nGains, outDev);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_follower_create(ssym_ctx *ctx, uint32_t n_lanes, double max_gain, ssym_follower **out)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return follower_create(ctx, n_lanes, max_gain, out); });
}

int32_t ssym_follower_destroy(ssym_ctx *ctx, ssym_follower *fl)
{
    return lane_destroy(ctx, fl, follower_free);
}

int32_t ssym_follower_push(ssym_ctx *ctx, ssym_follower *fl, const double *samples, const uint64_t *sample_offsets, const double *ref,
                           const uint64_t *ref_offsets, uint32_t flags, uint64_t *out_n_samples)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return follower_push(ctx, fl, samples, sample_offsets, ref, ref_offsets, flags, out_n_samples); });
}

int32_t ssym_follower_flush(ssym_ctx *ctx, ssym_follower *fl, uint32_t lane, uint64_t *out_n_samples)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return follower_flush(ctx, fl, lane, out_n_samples); });
}

int32_t ssym_follower_samples(ssym_ctx *ctx, const ssym_follower *fl, uint64_t *out_lane_offsets, double *out_samples,
                              int32_t *out_pcm32, uint64_t *out_gain_offsets, double *out_gain, uint32_t flags)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        return follower_samples(ctx, fl, out_lane_offsets, out_samples, out_pcm32, out_gain_offsets, out_gain, flags);
    });
}

int32_t ssym_follower_counts(const ssym_follower *fl, uint64_t *out_ny, uint64_t *out_nx, uint64_t *out_released)
{
    if (!fl)
        return SSYM_E_INVALID;
    for (uint32_t l = 0; l < fl->nLanes; ++l) {
        if (out_ny)
            out_ny[l] = fl->lanes[l].ny;
        if (out_nx)
            out_nx[l] = fl->lanes[l].nx;
        if (out_released)
            out_released[l] = fl->lanes[l].released;
    }
    return SSYM_OK;
}

int32_t ssym_follower_reset(ssym_ctx *ctx, ssym_follower *fl, uint32_t lane)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return follower_reset(ctx, fl, lane); });
}

}  // extern "C"
