// follow.hip -- envelope following: a reconstruction takes the loudness of its target (DESIGN.md section 2 "Envelope
// following", 5.28).  A post-pass: any reconstruction the library makes goes in, the same samples scaled by a gain that
// moves hop by hop come out.
//
// Definition (the header carries it too; tests/follow_ref.py restates it).  For target t: y[0 .. n) the reconstruction,
// x[0 .. nx) the reference (x[k] reads +0.0 for k >= nx; x[k] for k >= n is never read), w[] the window table of
// mfcc_frame.hpp, J = ceil(n / HOP), boundaries b = 0 ... J when n > 0.
//   energy  E_s(b) = sum over m = 0 ... 1023 ascending, from +0.0, of w[m] * (s[k] * s[k]), k = (b - 2) * HOP + m, only the
//           m with 0 <= k < n; t = s * s; t = w[m] * t; acc = acc + t -- three roundings, no contraction
//   gain    g(b) = sqrt(E_x(b) / E_y(b)); NaN: 1.0; else above max_gain: max_gain
//   sample  j = k / HOP, f = (k - j * HOP) / 256.0, a = g(j) * (1.0 - f), c = g(j + 1) * f, out[k] = y[k] * (a + c)
//   pcm     ssym_reconstruct's conversion of out[k]
//
// Two kernels, stream order between them and nothing else.
//
// follow_gain_kernel: one workgroup per entry of a host-built block table, an entry = (target, first boundary of a block of
// up to 32 consecutive boundaries) -- so a batch of ragged targets is one dense 1-D grid and a short target costs the one
// workgroup it needs.  The 32 windows of a block span 35 hops; all 256 threads stage that span of y and of x in LDS once
// (+0.0 outside [0, n), and for x at or beyond nx), hop by hop with a pitch of 257 doubles.  Then wave 0 runs the chains,
// one lane per (boundary, signal): lanes 0 ... 31 the block's boundaries on y, lanes 32 ... 63 the same on x.  At step m lane
// l reads slot (l mod 32 + m / 256) * 257 + m mod 256: neighbouring lanes sit 257 doubles apart, 514 dwords, 2 banks -- the
// 32 lanes of a ds_read_b64 group fall on the 32 distinct bank pairs (at a pitch of 256 they would all share one).  A value
// outside the target is staged as +0.0 and adds w * (0 * 0) = +0.0, which leaves the sum's bits alone, so every lane runs
// all 1024 steps and nothing diverges.  w[m] is the same for every lane: the window sits in LDS beside the span and every
// read of it is a broadcast.  E_x crosses to the y lane by one shuffle; the division, the square root and the two selects
// run there.  Every sample comes from global memory once per block, 35 / 32 times in all.
//
// follow_apply_kernel: warp_kernel's grid, a workgroup per (target, 4096-sample chunk), one thread per output sample and
// hop, f the same for all 16 samples of a thread.  The chunk's 17 gains sit in LDS, every read a broadcast.
//
// The block geometry, the chain, the gain's division, square root and selects and a sample's arithmetic are
// follow_common.hpp's (follow_chain, follow_gain, follow_sample): the live follower (follower.hip) runs the same text.  Every
// product there is a __dmul_rn, every sum a __dadd_rn, the gain a __dsqrt_rn of a __ddiv_rn: nothing contracts, whatever the
// compiler is told.
#include "follow_common.hpp"

namespace ssym {
namespace {

constexpr uint32_t kFollowGridY = 65535;                   // targets per launch of follow_apply_kernel (the grid's y)

struct FollowArgs {
    const double *y;            // the reconstructions, packed by outOff (may be the array `out` of the apply kernel)
    const double *x;            // the references, packed by refOff
    const uint64_t *outOff;     // [nTargets + 1]
    const uint64_t *refOff;     // [nTargets + 1]
    const uint64_t *gainOff;    // [nTargets + 1]: target t's g(0) at gain[gainOff[t]]
    const uint2 *table;         // per workgroup of the gain kernel: (target, first boundary)
    const double *win;          // [1024]
    double maxGain;
    double *gain;
};

__global__ __launch_bounds__(256) void follow_gain_kernel(const FollowArgs a)
{
    extern __shared__ double sm[];               // [1024] the window, then [2][hops][257]: y's span, then x's
    const uint2 e = a.table[blockIdx.x];
    const uint32_t t = e.x, b0 = e.y;
    const uint64_t o0 = a.outOff[t], n = a.outOff[t + 1] - o0;
    const uint64_t r0 = a.refOff[t], nx = a.refOff[t + 1] - r0;
    const uint64_t B = (n + kWarpHop - 1) / kWarpHop + 1;       // a listed target has n > 0 and b0 < B
    const int nb = (int)std::min<uint64_t>(kFollowBlock, B - b0);
    const int hops = nb + kWarpTaps - 1;
    double *sw = sm, *sy = sm + kWarpBin, *sx = sy + hops * kFollowPitch;
    const int tid = (int)threadIdx.x;
    const double *__restrict__ y = a.y + o0;
    const double *__restrict__ x = a.x + r0;
    // the window beside the span: a scalar load in the chain's loop would make every wait there a wait for everything
#pragma unroll
    for (int q = 0; q < kWarpTaps; ++q)
        sw[tid + 256 * q] = a.win[tid + 256 * q];
    // twelve hops of both signals, 24 loads in flight per thread (35 = 12 + 12 + 11); a CU holds one workgroup, so the
    // registers are there
    constexpr int G = 12;
    for (int i0 = 0; i0 < hops; i0 += G) {
        double vy[G], vx[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int64_t k = ((int64_t)b0 - 2 + i0 + u) * kWarpHop + tid;
            const bool in = i0 + u < hops && k >= 0 && (uint64_t)k < n;      // tested before the loads: no read outside [0, n) / [0, nx)
            vy[u] = in ? y[k] : 0.0;
            vx[u] = (in && (uint64_t)k < nx) ? x[k] : 0.0;
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
    if (sig == 0 && bl < nb) {
        a.gain[a.gainOff[t] + b0 + (uint32_t)bl] = follow_gain(ex, acc, a.maxGain);
    }
}

// y may be out: a thread reads the sample it writes, nothing else of the array
__global__ __launch_bounds__(256) void follow_apply_kernel(const FollowArgs a, uint32_t t0, double *out, int32_t *pcm)
{
    __shared__ double sG[kWarpChunk / kWarpHop + 1];
    const uint32_t t = t0 + blockIdx.y;
    const uint64_t o0 = a.outOff[t], n = a.outOff[t + 1] - o0;
    const uint64_t c0 = (uint64_t)blockIdx.x * kWarpChunk;
    if (c0 >= n)
        return;                                  // the whole workgroup: nothing of this target in the chunk
    const uint32_t tid = threadIdx.x;
    if (tid < (uint32_t)(kWarpChunk / kWarpHop + 1)) {
        const uint64_t b = c0 / kWarpHop + tid, J = (n + kWarpHop - 1) / kWarpHop;
        sG[tid] = b <= J ? a.gain[a.gainOff[t] + b] : 0.0;      // beyond J: no sample of the chunk asks for it
    }
    __syncthreads();
    const double f = (double)tid / 256.0, fm = 1.0 - f;         // both exact
    const uint64_t k0 = c0 + tid;
    const double *y = a.y + o0;
#pragma unroll
    for (int u = 0; u < 16; u += 4) {
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t k = k0 + (uint64_t)(u + q) * 256;
            v[q] = k < n ? y[k] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t k = k0 + (uint64_t)(u + q) * 256;
            if (k >= n)
                continue;
            const double r = follow_sample(v[q], sG[u + q], sG[u + q + 1], f, fm);
            if (out)
                out[o0 + k] = r;
            if (pcm)
                pcm[o0 + k] = warp_pcm32(r);
        }
    }
}

}  // namespace

int32_t follow_envelope(ssym_ctx *ctx, const double *samples, const uint64_t *out_offsets, uint32_t n_targets, const double *ref,
                        const uint64_t *ref_offsets, double max_gain, uint32_t flags, double *out_samples, int32_t *out_pcm32,
                        double *out_gain)
{
    static const char *fn = "ssym_follow_envelope: ";
    if (!ctx)
        return SSYM_E_INVALID;
    auto refuse = [&](const std::string &what, int32_t rc = SSYM_E_INVALID) {
        ctx->err = fn + what;
        return rc;
    };
    if (flags & ~(uint32_t)(SSYM_OUT_DEVICE | SSYM_FOLLOW_SAMPLES_DEVICE | SSYM_FOLLOW_REF_DEVICE))
        return refuse("unknown flag bits");
    if (!(max_gain >= 1.0) || std::isinf(max_gain))
        return refuse("max_gain must be a finite number, 1 or more");
    if (n_targets >= 0x80000000u)
        return refuse("2^31 targets or more", SSYM_E_UNSUPPORTED);
    if (n_targets == 0)
        return SSYM_OK;
    if (!out_offsets || !ref_offsets)
        return refuse("out_offsets and ref_offsets must not be NULL");
    if (out_offsets[0] != 0 || ref_offsets[0] != 0)
        return refuse("out_offsets and ref_offsets must start at 0");
    uint64_t maxLen = 0, nBlocks = 0, nGains = 0;
    for (uint32_t t = 0; t < n_targets; ++t) {
        if (out_offsets[t + 1] < out_offsets[t] || ref_offsets[t + 1] < ref_offsets[t])
            return refuse("out_offsets or ref_offsets decrease (target " + std::to_string(t) + ")");
        const uint64_t n = out_offsets[t + 1] - out_offsets[t];
        if (n >= kFollowMaxLen)
            return refuse("a target of 2^40 samples or more (target " + std::to_string(t) + ")", SSYM_E_UNSUPPORTED);
        maxLen = std::max(maxLen, n);
        if (n) {
            const uint64_t B = (n + kWarpHop - 1) / kWarpHop + 1;
            nGains += B;
            nBlocks += (B + kFollowBlock - 1) / kFollowBlock;
        }
    }
    if (nBlocks > 0x7fffffffu)
        return refuse("more than 2^31 - 1 blocks of 32 boundaries", SSYM_E_UNSUPPORTED);
    const uint64_t total = out_offsets[n_targets], refTotal = ref_offsets[n_targets];
    if (total == 0)
        return SSYM_OK;
    if (!samples || (!ref && refTotal))
        return refuse("samples and ref must not be NULL while they hold samples");
    if (!out_samples && !out_pcm32 && !out_gain)
        return SSYM_OK;

    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;
    const bool yDev = (flags & SSYM_FOLLOW_SAMPLES_DEVICE) != 0, xDev = (flags & SSYM_FOLLOW_REF_DEVICE) != 0;
    // the one staging block, in ssym_reconstruct's scratch: [out offsets | ref offsets | gain offsets | window | block table],
    // 8-byte words all; behind it the host inputs
    const size_t n1 = (size_t)n_targets + 1;
    const size_t oRef = n1, oGain = 2 * n1, oWin = 3 * n1, oTab = oWin + kWarpBin, words = oTab + (size_t)nBlocks;
    std::vector<uint64_t> host(words);           // lives until the call's synchronisation
    std::copy(out_offsets, out_offsets + n1, host.data());
    std::copy(ref_offsets, ref_offsets + n1, host.data() + oRef);
    static_assert(sizeof(double) == sizeof(uint64_t) && sizeof(uint2) == sizeof(uint64_t), "one staging block");
    std::copy(warp_window().begin(), warp_window().end(), reinterpret_cast<double *>(host.data() + oWin));
    uint2 *tab = reinterpret_cast<uint2 *>(host.data() + oTab);
    uint64_t g = 0, maxB = 0;
    for (uint32_t t = 0; t < n_targets; ++t) {
        host[oGain + t] = g;
        const uint64_t n = out_offsets[t + 1] - out_offsets[t];
        if (!n)
            continue;
        const uint64_t B = (n + kWarpHop - 1) / kWarpHop + 1;
        for (uint64_t b = 0; b < B; b += kFollowBlock)
            *tab++ = make_uint2(t, (uint32_t)b);
        maxB = std::max(maxB, B);
        g += B;
    }
    host[oGain + n_targets] = g;
    const size_t inBytes = words * sizeof(uint64_t) + ((yDev ? 0 : (size_t)total) + (xDev ? 0 : (size_t)refTotal)) * sizeof(double);
    int32_t rc = ensure(ctx, ctx->best, inBytes + 16);
    if (rc != SSYM_OK)
        return rc;
    uint64_t *dev = (uint64_t *)ctx->best.ptr;
    double *dY = (double *)(dev + words), *dX = dY + (yDev ? 0 : total);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dev, host.data(), words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (!yDev)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dY, samples, total * sizeof(double), hipMemcpyHostToDevice, st));
    if (!xDev && refTotal)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dX, ref, refTotal * sizeof(double), hipMemcpyHostToDevice, st));
    // outputs: the caller's device arrays, or ctx->part as [samples | gains | pcm]; the gains are always written somewhere,
    // the apply kernel reads them
    double *dOut = out_samples, *dGain = out_gain;
    int32_t *dPcm = out_pcm32;
    if (!outDev) {
        rc = ensure(ctx, ctx->part, (total + nGains) * sizeof(double) + total * sizeof(int32_t));
        if (rc != SSYM_OK)
            return rc;
        dOut = out_samples ? (double *)ctx->part.ptr : nullptr;
        dGain = (double *)ctx->part.ptr + total;
        dPcm = out_pcm32 ? (int32_t *)((double *)ctx->part.ptr + total + nGains) : nullptr;
    } else if (!dGain) {
        rc = ensure(ctx, ctx->part, nGains * sizeof(double));
        if (rc != SSYM_OK)
            return rc;
        dGain = (double *)ctx->part.ptr;
    }
    FollowArgs a{};
    a.y = yDev ? samples : dY;
    a.x = xDev ? ref : dX;
    a.outOff = dev;
    a.refOff = dev + oRef;
    a.gainOff = dev + oGain;
    a.table = reinterpret_cast<const uint2 *>(dev + oTab);
    a.win = reinterpret_cast<const double *>(dev + oWin);
    a.maxGain = max_gain;
    a.gain = dGain;
    // LDS for the launch's largest block: a batch of short targets keeps several workgroups on a CU
    const size_t lds = follow_lds_doubles(maxB) * sizeof(double);
    if (lds > 64 * 1024)
        SSYM_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)follow_gain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const bool apply = dOut || dPcm;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], st));
    follow_gain_kernel<<<dim3((unsigned)nBlocks), 256, lds, st>>>(a);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[1], st));
    // warp_kernel's grid, the targets on its y extent kFollowGridY at a time: any n_targets the call accepts is launched
    for (uint32_t t0 = 0; apply && t0 < n_targets; t0 += kFollowGridY) {
        const dim3 grid((unsigned)((maxLen + kWarpChunk - 1) / kWarpChunk), std::min(kFollowGridY, n_targets - t0));
        follow_apply_kernel<<<grid, 256, 0, st>>>(a, t0, dOut, dPcm);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[2], st));
    if (!outDev && out_samples)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_samples, dOut, total * sizeof(double), hipMemcpyDeviceToHost, st));
    if (!outDev && out_pcm32)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_pcm32, dPcm, total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (!outDev && out_gain)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_gain, dGain, nGains * sizeof(double), hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    ssym_timings tm{};
    tm.main_ms = ev_ms(ctx->ev[0], ctx->ev[1]);                  // the gain kernel
    tm.reduce_ms = apply ? ev_ms(ctx->ev[1], ctx->ev[2]) : 0.f;  // the apply kernel
    tm.total_ms = ev_ms(ctx->ev[0], ctx->ev[2]);
    tm.main_launches = 1;
    ctx->timings = tm;
    return SSYM_OK;
}

}  // namespace ssym
