// wsola.hip -- warped reconstruction with a waveform-similarity search (WSOLA): warp.hip's overlap-add, but every source
// frame may start up to `search` samples off its nominal place map[j] * HOP, where it continues the frame laid down before
// it best (DESIGN.md section 2 "WSOLA", 5.14; the header carries the definition, tests/wsola_ref.py restates it).
//
// Definition.  HOP, BIN, w[], x[0 .. sLen), F, map[] as in warp.hip; S = search <= 512.  pos[0] = map[0] * HOP.  For j >= 1:
// nom = map[j] * HOP; tmpl[n] = x[pos[j-1] + HOP + n], n < BIN (a sample >= sLen reads +0.0); for every lag d in -S .. S
// with 0 <= nom + d < sLen: cand[n] = x[nom + d + n] (>= sLen reads +0.0), c = sum of tmpl[n] * cand[n], e = sum of cand[n]
// * cand[n], both from +0.0 in ascending n, every product and sum rounded on its own; score = c / sqrt(e), 0 when e = 0.
// pos[j] = nom + d*, d* the lag of the greatest score, ties to the smaller |d|, then to the negative d; a NaN score never
// wins; d* = 0 when no lag is admissible or none has a score that is a number.  Synthesis: warp.hip's taps / value / pcm with
// p = pos[j] + m.  Fallback: warp.hip's.
//
// wsola_search_kernel: the chain over j is serial, the targets are independent: one 256-thread workgroup per target,
// grid-stride.  A step is wsola_step (warp_common.hpp), which resynth_search_kernel (resynth.hip) runs as well.  Per step
// the template (8 KiB) and the candidate span x[nom - S .. nom + S + BIN) (<= 16 KiB) go to LDS;
// thread tid owns the lags tid, tid + 256, ... (at most five) and runs their sums n = 0 .. 1023 in the defined order, one
// template read (a broadcast) and one span read (consecutive lanes, consecutive doubles) per lag and n.  A wave runs only
// the rounds in which it owns a lag, so the odd 2 S + 1-th lag costs one wave one round.  The argmax is a butterfly over
// the wave and a pass over the four waves' winners; the order (score, -|d|, -d) is total over distinct lags, so the tree's
// shape cannot change the winner.
// wsola_synth_kernel: warp_kernel's gather (warp_common.hpp's warp_synth) with the 19 staged frame positions read from pos.
// The host driver takes warp.hip's steps from warp_common.hpp (WarpCall); this file adds the search width, the positions,
// its two launches and its timings.
#include "warp_common.hpp"

namespace ssym {
namespace {

constexpr unsigned kWsolaMaxGrid = 2048;                                         // search workgroups; targets beyond: grid-stride
constexpr uint64_t kWsolaUnset = ~(uint64_t)0;                                   // a position slot the search did not write

struct WsolaArgs : WarpArgs {   // the plain warp's (WarpCall::stage fills them), and:
    uint32_t nTargets;
    uint32_t search;            // S
    uint64_t *pos;              // sample start of every source frame, laid out as map (mapOff is rebased to both)
};

__global__ __launch_bounds__(256) void wsola_search_kernel(const WsolaArgs a)
{
    extern __shared__ double sm[];               // [BIN] template, then [BIN + 2 S] candidate span
    __shared__ double wScore[4];
    __shared__ int wLag[4];
    const WsolaStep w(sm, wScore, wLag, a.search);

    for (uint32_t t = blockIdx.x; t < a.nTargets; t += gridDim.x) {
        const uint32_t F = (a.pairLen && a.pairLen[t] == 0) ? 0u : a.mapFrames[t];
        if (F == 0)
            continue;                            // the length fit: no positions
        const uint32_t s = a.idx[t];
        uint64_t sBase = 0, sLen = 0;
        if (s < a.nSounds) {
            sBase = a.srcOff[s];
            sLen = a.srcOff[s + 1] - sBase;
        }
        const double *__restrict__ x = a.src + sBase;
        const uint32_t *__restrict__ map = a.map + a.mapOff[t];
        uint64_t *pos = a.pos + a.mapOff[t];
        uint64_t prev = (uint64_t)map[0] * (uint64_t)kWarpHop;
        if (w.tid == 0)
            pos[0] = prev;
        for (uint32_t j = 1; j < F; ++j) {
            const int64_t nom = (int64_t)((uint64_t)map[j] * (uint64_t)kWarpHop);       // < 2^40
            prev = (uint64_t)(nom + (int64_t)wsola_step(w, x, sLen, prev, nom));
            if (w.tid == 0)
                pos[j] = prev;
        }
    }
}

__global__ __launch_bounds__(256) void wsola_synth_kernel(const WsolaArgs a)
{
    warp_synth(a, [&](uint64_t o) { return a.pos[o]; });       // the searched position, < 2^40 + 512
}

int32_t reconstruct_wsola(WarpCall &c, uint32_t search, uint64_t *out_pos)
{
    int32_t rc = c.check_pointers();
    if (rc == SSYM_OK && search > kWsolaMaxSearch)
        rc = c.refuse("search must not exceed 512 samples");
    if (rc == SSYM_OK)
        rc = c.check();
    if (rc != SSYM_OK || c.idle())
        return rc;
    ssym_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    const bool doSearch = c.anyMap && c.mapTotal;
    const bool posDev = (c.flags & SSYM_OUT_DEVICE) && out_pos;      // the search writes the caller's device array itself
    const bool posBack = doSearch && out_pos && !posDev;
    // the positions: behind the staging block and the map, unless they are device memory of the caller's
    const size_t posBytes = (doSearch && !posDev) ? (size_t)c.mapTotal * sizeof(uint64_t) : 0;
    WsolaArgs a{};
    void *scratch = nullptr;
    rc = c.stage(a, posBytes, &scratch);
    if (rc != SSYM_OK)
        return rc;
    a.nTargets = c.n_targets;
    a.search = search;
    a.pos = posDev ? out_pos + c.map_offsets[0] : (uint64_t *)scratch;
    if (posBack)        // slots the search leaves alone (slack, targets without a path) must stay the caller's
        SSYM_HIP_CHECK(ctx, hipMemsetAsync(a.pos, 0xFF, posBytes, st));
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], st));
    if (doSearch) {
        const size_t lds = (size_t)(2 * kWarpBin + 2 * search) * sizeof(double);
        wsola_search_kernel<<<std::min<unsigned>(c.n_targets, kWsolaMaxGrid), 256, lds, st>>>(a);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[1], st));
    wsola_synth_kernel<<<c.grid(), 256, 0, st>>>(a);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[2], st));
    std::vector<uint64_t> hostPos(posBack ? (size_t)c.mapTotal : 0);
    if (posBack)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(hostPos.data(), a.pos, posBytes, hipMemcpyDeviceToHost, st));
    rc = c.finish();
    if (rc != SSYM_OK)
        return rc;
    for (size_t i = 0; i < hostPos.size(); ++i)
        if (hostPos[i] != kWsolaUnset)                   // a position is below 2^41
            out_pos[c.map_offsets[0] + i] = hostPos[i];
    ssym_timings tm{};
    tm.main_ms = doSearch ? ev_ms(ctx->ev[0], ctx->ev[1]) : 0.f;       // the search kernel
    tm.reduce_ms = ev_ms(ctx->ev[1], ctx->ev[2]);                      // the synthesis kernel
    tm.total_ms = ev_ms(ctx->ev[0], ctx->ev[2]);
    tm.main_launches = doSearch ? 1 : 0;
    ctx->timings = tm;
    return SSYM_OK;
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_reconstruct_wsola(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx, const uint64_t *out_offsets,
                               uint32_t n_targets, const uint32_t *frame_map, const uint64_t *map_offsets,
                               const uint32_t *map_frames, const uint32_t *pair_len, uint32_t search, uint32_t flags,
                               uint64_t *out_pos, double *out_samples, int32_t *out_pcm32)
{
    return guarded(ctx, [&]() -> int32_t {
        WarpCall c{ctx, s, idx, out_offsets, n_targets, frame_map, map_offsets, map_frames, pair_len, flags, out_samples,
                   out_pcm32, SampleWindows(), "ssym_reconstruct_wsola"};
        return reconstruct_wsola(c, search, out_pos);
    });
}

// the call above with a window of samples per target: the same driver, the kernels untouched (SampleWindows)
int32_t ssym_reconstruct_wsola_spans(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx, const uint64_t *win_first,
                                     const uint64_t *win_len, const uint64_t *out_offsets, uint32_t n_targets,
                                     const uint32_t *frame_map, const uint64_t *map_offsets, const uint32_t *map_frames,
                                     const uint32_t *pair_len, uint32_t search, uint32_t flags, uint64_t *out_pos,
                                     double *out_samples, int32_t *out_pcm32)
{
    return guarded(ctx, [&]() -> int32_t {
        WarpCall c{ctx, s, idx, out_offsets, n_targets, frame_map, map_offsets, map_frames, pair_len, flags, out_samples,
                   out_pcm32, SampleWindows(), "ssym_reconstruct_wsola_spans"};
        const int32_t rc = warp_windows(ctx, c.fn, win_first, win_len, c.wn);
        return rc == SSYM_OK ? reconstruct_wsola(c, search, out_pos) : rc;
    });
}

}  // extern "C"
