// warp.hip -- warped reconstruction: every match resynthesised along the target-frame -> source-frame map that
// ssym_dtw_align gives, so that it follows the target's timing (DESIGN.md section 2 "Warped reconstruction", 5.13).
//
// Definition (the header carries it too; tests/warp_ref.py restates it).  HOP = 256, BIN = 1024, w[m] = 0.5 - 0.5 *
// cos(2 pi m / 1024) (mfcc_frame.hpp's table, built on the host with libm cos).  For target t: n output samples,
// x[0 .. sLen) the samples of dictionary sound idx[t], map[0 .. F) its source frame per target frame.  Output sample
// k < n has the taps j (target frames) with j * HOP <= k < j * HOP + BIN and j < F, at most four, visited in ascending
// j: m = k - j * HOP, p = map[j] * HOP + m (64-bit), valid when p < sLen.  num = sum of w[m] * x[p] and den = sum of
// w[m] over the valid taps, both sums starting at +0.0, product and sums rounded separately; out[k] = num / den when
// den > 0, else +0.0.  A target with F = 0 or pair_len[t] = 0 takes ssym_reconstruct's length fit.
//
// Gather form: one thread per output sample, no atomics.  One 256-thread workgroup per (target, 4096-sample chunk),
// as reconstruct_kernel.  Thread `tid` computes samples k = chunk + tid + 256 u, u = 0 .. 15; for a fixed u the whole
// workgroup shares k / 256, so its taps are the same four target frames and m = tid + 256 q, q = 3 .. 0: a thread
// only ever needs the window at tid, tid + 256, tid + 512 and tid + 768, which it keeps in registers.  The chunk touches
// target frames chunk / 256 - 3 ... chunk / 256 + 15: their 19 source positions map[j] * HOP sit in LDS (sLen for a
// frame outside [0, F): such a tap is never valid), every read of them a broadcast.
#include "warp_common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace ssym {
namespace {

struct WarpArgs {
    const double *src;          // the store's samples
    const uint64_t *srcOff;     // [nSounds + 1]
    uint32_t nSounds;
    const uint32_t *idx;        // [nTargets]
    const uint64_t *outOff;     // [nTargets + 1]
    const uint32_t *map;        // source frame per target frame, target t from mapOff[t] on
    const uint64_t *mapOff;     // [nTargets + 1], rebased to map
    const uint32_t *mapFrames;  // [nTargets]
    const uint32_t *pairLen;    // nullable, [nTargets]: 0 = no path, the length fit
    const double *win;          // [1024]
    double *out;                // nullable
    int32_t *pcm;               // nullable
};

__global__ __launch_bounds__(256) void warp_kernel(const WarpArgs a)
{
    __shared__ uint64_t sPos[kWarpFrames];
    const uint32_t t = blockIdx.y;
    const uint64_t o0 = a.outOff[t], n = a.outOff[t + 1] - o0;
    const uint64_t c0 = (uint64_t)blockIdx.x * kWarpChunk;
    if (c0 >= n)
        return;                                  // the whole workgroup: nothing of this target in the chunk
    const uint32_t s = a.idx[t];
    uint64_t sBase = 0, sLen = 0;
    if (s < a.nSounds) {
        sBase = a.srcOff[s];
        sLen = a.srcOff[s + 1] - sBase;
    }
    const double *__restrict__ x = a.src + sBase;
    const uint32_t F = (a.pairLen && a.pairLen[t] == 0) ? 0u : a.mapFrames[t];
    const uint32_t tid = threadIdx.x;
    const uint64_t k0 = c0 + tid;

    if (F == 0) {
        // no map: ssym_reconstruct's length fit (src/sound.rs:457-462), four loads in flight
#pragma unroll
        for (int u = 0; u < 16; u += 4) {
            double v[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint64_t k = k0 + (uint64_t)(u + w) * 256;
                v[w] = (k < n && k < sLen) ? x[k] : 0.0;
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint64_t k = k0 + (uint64_t)(u + w) * 256;
                if (k >= n)
                    continue;
                if (a.out)
                    a.out[o0 + k] = v[w];
                if (a.pcm)
                    a.pcm[o0 + k] = warp_pcm32(v[w]);
            }
        }
        return;
    }

    // source position of the 19 target frames that reach into this chunk; sLen: no such frame, never a valid tap
    if (tid < (uint32_t)kWarpFrames) {
        const int64_t j = (int64_t)(c0 / kWarpHop) - (kWarpTaps - 1) + (int64_t)tid;
        uint64_t pos = sLen;
        if (j >= 0 && j < (int64_t)F)
            pos = (uint64_t)a.map[a.mapOff[t] + (uint64_t)j] * (uint64_t)kWarpHop;     // < 2^40: no overflow below
        sPos[tid] = pos;
    }
    double wq[kWarpTaps];
#pragma unroll
    for (int q = 0; q < kWarpTaps; ++q)
        wq[q] = a.win[tid + 256 * q];
    __syncthreads();

    // two output samples, eight source loads in flight per thread
#pragma unroll
    for (int u = 0; u < 16; u += 2) {
        double v[2][kWarpTaps];
        bool ok[2][kWarpTaps];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < kWarpTaps; ++i) {
                // tap i in ascending target frame: frame slot u + h + i, window quarter q = 3 - i
                const uint64_t p = sPos[u + h + i] + (uint64_t)(tid + 256 * (kWarpTaps - 1 - i));
                ok[h][i] = p < sLen;                       // tested before the load: no map content reads outside x
                v[h][i] = ok[h][i] ? x[p] : 0.0;
            }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint64_t k = k0 + (uint64_t)(u + h) * 256;
            if (k >= n)
                continue;
            double num = 0.0, den = 0.0;
#pragma unroll
            for (int i = 0; i < kWarpTaps; ++i)
                if (ok[h][i]) {
                    const double w = wq[kWarpTaps - 1 - i];
                    num = __dadd_rn(num, __dmul_rn(w, v[h][i]));
                    den = __dadd_rn(den, w);
                }
            const double r = den > 0.0 ? __ddiv_rn(num, den) : 0.0;
            if (a.out)
                a.out[o0 + k] = r;
            if (a.pcm)
                a.pcm[o0 + k] = warp_pcm32(r);
        }
    }
}

int32_t reconstruct_warped(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx, const uint64_t *out_offsets,
                           uint32_t n_targets, const uint32_t *frame_map, const uint64_t *map_offsets,
                           const uint32_t *map_frames, const uint32_t *pair_len, uint32_t flags, double *out_samples,
                           int32_t *out_pcm32, const SampleWindows &wn = SampleWindows(),
                           const char *fn = "ssym_reconstruct_warped")
{
    if (!ctx)
        return SSYM_E_INVALID;
    const std::string name(fn);
    if (!s || !idx || !out_offsets || !map_offsets || !map_frames) {
        ctx->err = name + ": s, idx, out_offsets, map_offsets and map_frames must not be NULL";
        return SSYM_E_INVALID;
    }
    if (out_offsets[0] != 0) {
        ctx->err = name + ": out_offsets must start at 0";
        return SSYM_E_INVALID;
    }
    if (flags & ~(uint32_t)(SSYM_OUT_DEVICE | SSYM_WARP_MAP_DEVICE)) {
        ctx->err = name + ": unknown flag bits";
        return SSYM_E_INVALID;
    }
    if (s->n == 0) {
        ctx->err = "empty dictionary";
        return SSYM_E_EMPTY_DICT;
    }
    uint64_t maxLen = 0;
    bool anyMap = false;
    for (uint32_t t = 0; t < n_targets; ++t) {
        if (out_offsets[t + 1] < out_offsets[t] || idx[t] >= s->n) {
            ctx->err = name + ": out_offsets decrease or an index is outside the sample store (target " +
                       std::to_string(t) + ")";
            return SSYM_E_INVALID;
        }
        if (map_offsets[t + 1] < map_offsets[t] || map_offsets[t + 1] - map_offsets[t] < map_frames[t]) {
            ctx->err = name + ": map_offsets decrease or leave less room than map_frames (target " +
                       std::to_string(t) + ")";
            return SSYM_E_INVALID;
        }
        anyMap = anyMap || map_frames[t] > 0;
        maxLen = std::max<uint64_t>(maxLen, out_offsets[t + 1] - out_offsets[t]);
    }
    if (anyMap && !frame_map) {
        ctx->err = name + ": frame_map is NULL although a target has map frames";
        return SSYM_E_INVALID;
    }
    if (wn) {
        const int32_t wrc = wn.check(ctx->err, fn, s, idx, n_targets);
        if (wrc != SSYM_OK)
            return wrc;
    }
    const uint64_t total = out_offsets[n_targets];
    if (n_targets == 0 || total == 0 || (!out_samples && !out_pcm32))
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0, mapDev = (flags & SSYM_WARP_MAP_DEVICE) != 0;
    const uint64_t mapTotal = map_offsets[n_targets] - map_offsets[0];
    const bool upLen = !mapDev && pair_len, upMap = !mapDev && anyMap && mapTotal;

    // staging, in ssym_reconstruct's scratch: [out offsets | map offsets | window] f64 / u64, then [idx | map frames |
    // pair_len | map] u32 -- one block, uploaded in one copy (plus the caller's map itself)
    const size_t n1 = (size_t)n_targets + 1;
    const size_t words64 = 2 * n1 + kWarpBin + (wn ? 2 * (size_t)n_targets : 0);     // ... | window table] with windows
    const size_t words32 = (size_t)n_targets * (upLen ? 3 : 2);
    std::vector<uint64_t> host(words64 + (words32 + 1) / 2);
    std::copy(out_offsets, out_offsets + n1, host.begin());
    for (size_t t = 0; t < n1; ++t)
        host[n1 + t] = map_offsets[t] - map_offsets[0];
    static_assert(sizeof(double) == sizeof(uint64_t), "one staging block");
    std::copy(warp_window().begin(), warp_window().end(), reinterpret_cast<double *>(host.data() + 2 * n1));
    uint32_t *h32 = reinterpret_cast<uint32_t *>(host.data() + words64);
    if (wn)
        wn.fill(s, idx, n_targets, host.data() + 2 * n1 + kWarpBin, h32);
    else
        std::copy(idx, idx + n_targets, h32);
    std::copy(map_frames, map_frames + n_targets, h32 + n_targets);
    if (upLen)
        std::copy(pair_len, pair_len + n_targets, h32 + 2 * (size_t)n_targets);
    const size_t metaBytes = host.size() * sizeof(uint64_t);
    int32_t rc = ensure(ctx, ctx->best, metaBytes + (upMap ? (size_t)mapTotal * sizeof(uint32_t) : 0) + 16);
    if (rc != SSYM_OK)
        return rc;
    uint64_t *d64 = (uint64_t *)ctx->best.ptr;
    uint32_t *d32 = (uint32_t *)(d64 + words64);
    uint32_t *dMap = (uint32_t *)((char *)ctx->best.ptr + metaBytes);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(d64, host.data(), metaBytes, hipMemcpyHostToDevice, st));
    if (upMap)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dMap, frame_map + map_offsets[0], (size_t)mapTotal * sizeof(uint32_t),
                                           hipMemcpyHostToDevice, st));
    double *dOut = out_samples;
    int32_t *dPcm = out_pcm32;
    if (!outDev) {
        rc = ensure(ctx, ctx->part, total * (sizeof(double) + sizeof(int32_t)));
        if (rc != SSYM_OK)
            return rc;
        dOut = out_samples ? (double *)ctx->part.ptr : nullptr;
        dPcm = out_pcm32 ? (int32_t *)((double *)ctx->part.ptr + total) : nullptr;
    }
    WarpArgs a{};
    a.src = s->samples;
    a.srcOff = wn ? d64 + 2 * n1 + kWarpBin : s->off;
    a.nSounds = wn ? 2 * n_targets : s->n;
    a.idx = d32;
    a.outOff = d64;
    a.map = mapDev ? (frame_map ? frame_map + map_offsets[0] : nullptr) : dMap;
    a.mapOff = d64 + n1;
    a.mapFrames = d32 + n_targets;
    a.pairLen = mapDev ? pair_len : (upLen ? d32 + 2 * (size_t)n_targets : nullptr);
    a.win = reinterpret_cast<const double *>(d64 + 2 * n1);
    a.out = dOut;
    a.pcm = dPcm;
    dim3 grid((unsigned)((maxLen + kWarpChunk - 1) / kWarpChunk), n_targets);
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], st));
    warp_kernel<<<grid, 256, 0, st>>>(a);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[1], st));
    if (!outDev) {
        if (out_samples)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_samples, dOut, total * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out_pcm32)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_pcm32, dPcm, total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));       // the call's one synchronisation (the host block above lives until here)
    ssym_timings tm{};
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess)
        tm.main_ms = tm.total_ms = ms;       // the synthesis kernel alone (ssym_get_timings)
    tm.main_launches = 1;
    ctx->timings = tm;
    return SSYM_OK;
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_reconstruct_warped(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx, const uint64_t *out_offsets,
                                uint32_t n_targets, const uint32_t *frame_map, const uint64_t *map_offsets,
                                const uint32_t *map_frames, const uint32_t *pair_len, uint32_t flags,
                                double *out_samples, int32_t *out_pcm32)
{
    return guarded(ctx, [&]() -> int32_t {
        return reconstruct_warped(ctx, s, idx, out_offsets, n_targets, frame_map, map_offsets, map_frames, pair_len,
                                  flags, out_samples, out_pcm32);
    });
}

// the call above with a window of samples per target: the same driver, the kernel untouched (SampleWindows)
int32_t ssym_reconstruct_warped_spans(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx, const uint64_t *win_first,
                                      const uint64_t *win_len, const uint64_t *out_offsets, uint32_t n_targets,
                                      const uint32_t *frame_map, const uint64_t *map_offsets, const uint32_t *map_frames,
                                      const uint32_t *pair_len, uint32_t flags, double *out_samples, int32_t *out_pcm32)
{
    return guarded(ctx, [&]() -> int32_t {
        if (ctx && (!win_first || !win_len)) {
            ctx->err = "ssym_reconstruct_warped_spans: win_first and win_len must not be NULL";
            return SSYM_E_INVALID;
        }
        SampleWindows wn;
        wn.first = win_first;
        wn.len = win_len;
        return reconstruct_warped(ctx, s, idx, out_offsets, n_targets, frame_map, map_offsets, map_frames, pair_len,
                                  flags, out_samples, out_pcm32, wn, "ssym_reconstruct_warped_spans");
    });
}

}  // extern "C"
