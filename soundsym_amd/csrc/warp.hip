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
// warp_common.hpp holds the gather itself (warp_synth, shared with wsola.hip's synthesis) and the host driver's steps
// (WarpCall); this file says where a target frame's source position comes from -- map[j] * HOP -- and owns the launch and
// its timings.
#include "warp_common.hpp"

namespace ssym {
namespace {

__global__ __launch_bounds__(256) void warp_kernel(const WarpArgs a)
{
    warp_synth(a, [&](uint64_t o) { return (uint64_t)a.map[o] * (uint64_t)kWarpHop; });       // < 2^40
}

int32_t reconstruct_warped(WarpCall &c)
{
    int32_t rc = c.check_pointers();
    if (rc == SSYM_OK)
        rc = c.check();
    if (rc != SSYM_OK || c.idle())
        return rc;
    ssym_ctx *ctx = c.ctx;
    WarpArgs a{};
    rc = c.stage(a);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    warp_kernel<<<c.grid(), 256, 0, ctx->stream>>>(a);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    rc = c.finish();
    if (rc != SSYM_OK)
        return rc;
    ssym_timings tm{};
    tm.main_ms = tm.total_ms = ev_ms(ctx->ev[0], ctx->ev[1]);       // the synthesis kernel alone (ssym_get_timings)
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
        WarpCall c{ctx, s, idx, out_offsets, n_targets, frame_map, map_offsets, map_frames, pair_len, flags, out_samples,
                   out_pcm32, SampleWindows(), "ssym_reconstruct_warped"};
        return reconstruct_warped(c);
    });
}

// the call above with a window of samples per target: the same driver, the kernel untouched (SampleWindows)
int32_t ssym_reconstruct_warped_spans(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx, const uint64_t *win_first,
                                      const uint64_t *win_len, const uint64_t *out_offsets, uint32_t n_targets,
                                      const uint32_t *frame_map, const uint64_t *map_offsets, const uint32_t *map_frames,
                                      const uint32_t *pair_len, uint32_t flags, double *out_samples, int32_t *out_pcm32)
{
    return guarded(ctx, [&]() -> int32_t {
        WarpCall c{ctx, s, idx, out_offsets, n_targets, frame_map, map_offsets, map_frames, pair_len, flags, out_samples,
                   out_pcm32, SampleWindows(), "ssym_reconstruct_warped_spans"};
        const int32_t rc = warp_windows(ctx, c.fn, win_first, win_len, c.wn);
        return rc == SSYM_OK ? reconstruct_warped(c) : rc;
    });
}

}  // extern "C"
