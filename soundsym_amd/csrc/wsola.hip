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
// grid-stride.  Per step the template (8 KiB) and the candidate span x[nom - S .. nom + S + BIN) (<= 16 KiB) go to LDS;
// thread tid owns the lags tid, tid + 256, ... (at most five) and runs their sums n = 0 .. 1023 in the defined order, one
// template read (a broadcast) and one span read (consecutive lanes, consecutive doubles) per lag and n.  A wave runs only
// the rounds in which it owns a lag, so the odd 2 S + 1-th lag costs one wave one round.  The argmax is a butterfly over
// the wave and a pass over the four waves' winners; the order (score, -|d|, -d) is total over distinct lags, so the tree's
// shape cannot change the winner.
// wsola_synth_kernel: warp_kernel's gather with the 19 staged frame positions read from pos.
#include "warp_common.hpp"

#include <algorithm>
#include <vector>

namespace ssym {
namespace {

constexpr uint32_t kWsolaMaxSearch = 512;
constexpr int kWsolaMaxRounds = (2 * (int)kWsolaMaxSearch + 1 + 255) / 256;      // 5 lags per thread at most
constexpr unsigned kWsolaMaxGrid = 2048;                                         // search workgroups; targets beyond: grid-stride
constexpr int kWsolaNone = INT32_MIN;                                            // "no lag yet" in the argmax
constexpr uint64_t kWsolaUnset = ~(uint64_t)0;                                   // a position slot the search did not write

struct WsolaArgs {
    const double *src;          // the store's samples
    const uint64_t *srcOff;     // [nSounds + 1]
    uint32_t nSounds;
    uint32_t nTargets;
    uint32_t search;            // S
    const uint32_t *idx;        // [nTargets]
    const uint64_t *outOff;     // [nTargets + 1]
    const uint32_t *map;        // source frame per target frame, target t from mapOff[t] on
    const uint64_t *mapOff;     // [nTargets + 1], rebased to map (and to pos)
    const uint32_t *mapFrames;  // [nTargets]
    const uint32_t *pairLen;    // nullable, [nTargets]: 0 = no path, the length fit
    const double *win;          // [1024]
    uint64_t *pos;              // sample start of every source frame, laid out as map
    double *out;                // nullable
    int32_t *pcm;               // nullable
};

// does lag a (score sa) beat lag b?  Neither score is NaN; kWsolaNone loses to everything.
__device__ __forceinline__ bool wsola_beats(double sa, int da, double sb, int db)
{
    if (da == kWsolaNone) return false;
    if (db == kWsolaNone) return true;
    if (sa != sb) return sa > sb;
    const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
    if (aa != ab) return aa < ab;
    return da < db;
}

// the two sums of R lags of one thread, n ascending, products and sums rounded separately
template <int R>
__device__ __forceinline__ void wsola_sums(const double *__restrict__ sT, const double *__restrict__ sC, const int *lag,
                                           double *c, double *e)
{
#pragma unroll
    for (int r = 0; r < R; ++r)
        c[r] = e[r] = 0.0;
#pragma unroll 4
    for (int n = 0; n < kWarpBin; ++n) {
        const double tv = sT[n];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double v = sC[lag[r] + n];
            c[r] = __dadd_rn(c[r], __dmul_rn(tv, v));
            e[r] = __dadd_rn(e[r], __dmul_rn(v, v));
        }
    }
}

__global__ __launch_bounds__(256) void wsola_search_kernel(const WsolaArgs a)
{
    extern __shared__ double sm[];               // [BIN] template, then [BIN + 2 S] candidate span
    __shared__ double wScore[4];
    __shared__ int wLag[4];
    double *sT = sm, *sC = sm + kWarpBin;
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    const int S = (int)a.search, L = 2 * S + 1;
    // rounds in which this wave owns a lag: lags wave * 64 + 256 r < L
    const int rounds = L > wave * 64 ? (L - wave * 64 + 255) / 256 : 0;

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
        if (tid == 0)
            pos[0] = prev;
        for (uint32_t j = 1; j < F; ++j) {
            const int64_t nom = (int64_t)((uint64_t)map[j] * (uint64_t)kWarpHop);       // < 2^40
            // admissible lags lo .. hi: 0 <= nom + d < sLen (sLen < 2^61: a store of doubles)
            const int64_t lo = nom < (int64_t)S ? -nom : -(int64_t)S;
            const int64_t hi = std::min<int64_t>((int64_t)S, (int64_t)sLen - 1 - nom);
            int best = 0;
            if (S > 0 && lo <= hi) {             // the same for every thread of the workgroup
                __syncthreads();                 // the step before has read its template and span
                for (int i = tid; i < kWarpBin; i += 256) {
                    const uint64_t q = prev + (uint64_t)kWarpHop + (uint64_t)i;
                    sT[i] = q < sLen ? x[q] : 0.0;
                }
                for (int i = tid; i < kWarpBin + 2 * S; i += 256) {
                    const int64_t p = nom - (int64_t)S + (int64_t)i;
                    sC[i] = (p >= 0 && (uint64_t)p < sLen) ? x[p] : 0.0;
                }
                __syncthreads();
                int lag[kWsolaMaxRounds];
                double c[kWsolaMaxRounds], e[kWsolaMaxRounds];
#pragma unroll
                for (int r = 0; r < kWsolaMaxRounds; ++r)
                    lag[r] = std::min(tid + 256 * r, L - 1);     // a lane past the last lag repeats it: reads stay in the span
                switch (rounds) {
                case 1: wsola_sums<1>(sT, sC, lag, c, e); break;
                case 2: wsola_sums<2>(sT, sC, lag, c, e); break;
                case 3: wsola_sums<3>(sT, sC, lag, c, e); break;
                case 4: wsola_sums<4>(sT, sC, lag, c, e); break;
                case 5: wsola_sums<5>(sT, sC, lag, c, e); break;
                default: break;
                }
                double bs = 0.0;
                int bd = kWsolaNone;
#pragma unroll
                for (int r = 0; r < kWsolaMaxRounds; ++r) {
                    if (r >= rounds || tid + 256 * r >= L)
                        continue;
                    const int d = tid + 256 * r - S;
                    if ((int64_t)d < lo || (int64_t)d > hi)
                        continue;
                    const double sc = e[r] == 0.0 ? 0.0 : __ddiv_rn(c[r], __dsqrt_rn(e[r]));
                    if (sc != sc)
                        continue;                // NaN never wins
                    if (wsola_beats(sc, d, bs, bd)) {
                        bs = sc;
                        bd = d;
                    }
                }
#pragma unroll
                for (int w = 32; w >= 1; w >>= 1) {
                    const double os = __shfl_xor(bs, w, 64);
                    const int od = __shfl_xor(bd, w, 64);
                    if (wsola_beats(os, od, bs, bd)) {
                        bs = os;
                        bd = od;
                    }
                }
                if ((tid & 63) == 0) {
                    wScore[wave] = bs;
                    wLag[wave] = bd;
                }
                __syncthreads();
                bs = wScore[0];
                bd = wLag[0];
#pragma unroll
                for (int w = 1; w < 4; ++w)
                    if (wsola_beats(wScore[w], wLag[w], bs, bd)) {
                        bs = wScore[w];
                        bd = wLag[w];
                    }
                best = bd == kWsolaNone ? 0 : bd;
            }
            prev = (uint64_t)(nom + (int64_t)best);
            if (tid == 0)
                pos[j] = prev;
        }
    }
}

__global__ __launch_bounds__(256) void wsola_synth_kernel(const WsolaArgs a)
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
        // no map: ssym_reconstruct's length fit, as warp_kernel
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

    // searched source position of the 19 target frames that reach into this chunk; sLen: no such frame, never a valid tap
    if (tid < (uint32_t)kWarpFrames) {
        const int64_t j = (int64_t)(c0 / kWarpHop) - (kWarpTaps - 1) + (int64_t)tid;
        uint64_t pos = sLen;
        if (j >= 0 && j < (int64_t)F)
            pos = a.pos[a.mapOff[t] + (uint64_t)j];               // < 2^40 + 512: no overflow below
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
                ok[h][i] = p < sLen;                       // tested before the load: no position reads outside x
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

int32_t reconstruct_wsola(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx, const uint64_t *out_offsets,
                          uint32_t n_targets, const uint32_t *frame_map, const uint64_t *map_offsets,
                          const uint32_t *map_frames, const uint32_t *pair_len, uint32_t search, uint32_t flags,
                          uint64_t *out_pos, double *out_samples, int32_t *out_pcm32,
                          const SampleWindows &wn = SampleWindows(), const char *fn = "ssym_reconstruct_wsola")
{
    if (!ctx)
        return SSYM_E_INVALID;
    const std::string name(fn);
    if (!s || !idx || !out_offsets || !map_offsets || !map_frames) {
        ctx->err = name + ": s, idx, out_offsets, map_offsets and map_frames must not be NULL";
        return SSYM_E_INVALID;
    }
    if (search > kWsolaMaxSearch) {
        ctx->err = name + ": search must not exceed 512 samples";
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
    const bool doSearch = anyMap && mapTotal;
    const bool posDev = outDev && out_pos;               // the search writes the caller's device array itself
    const bool posBack = doSearch && out_pos && !outDev;

    // staging, in ssym_reconstruct's scratch: [out offsets | map offsets | window] f64 / u64, then [idx | map frames |
    // pair_len] u32 -- one block, uploaded in one copy; behind it the caller's map and the positions, unless they are
    // device memory of the caller's
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
    const size_t mapBytes = upMap ? (((size_t)mapTotal * sizeof(uint32_t) + 7) & ~(size_t)7) : 0;
    const size_t posBytes = (doSearch && !posDev) ? (size_t)mapTotal * sizeof(uint64_t) : 0;
    int32_t rc = ensure(ctx, ctx->best, metaBytes + mapBytes + posBytes + 16);
    if (rc != SSYM_OK)
        return rc;
    uint64_t *d64 = (uint64_t *)ctx->best.ptr;
    uint32_t *d32 = (uint32_t *)(d64 + words64);
    uint32_t *dMap = (uint32_t *)((char *)ctx->best.ptr + metaBytes);
    uint64_t *dPos = posDev ? out_pos + map_offsets[0] : (uint64_t *)((char *)ctx->best.ptr + metaBytes + mapBytes);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(d64, host.data(), metaBytes, hipMemcpyHostToDevice, st));
    if (upMap)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dMap, frame_map + map_offsets[0], (size_t)mapTotal * sizeof(uint32_t),
                                           hipMemcpyHostToDevice, st));
    if (posBack)        // slots the search leaves alone (slack, targets without a path) must stay the caller's
        SSYM_HIP_CHECK(ctx, hipMemsetAsync(dPos, 0xFF, posBytes, st));
    double *dOut = out_samples;
    int32_t *dPcm = out_pcm32;
    if (!outDev) {
        rc = ensure(ctx, ctx->part, total * (sizeof(double) + sizeof(int32_t)));
        if (rc != SSYM_OK)
            return rc;
        dOut = out_samples ? (double *)ctx->part.ptr : nullptr;
        dPcm = out_pcm32 ? (int32_t *)((double *)ctx->part.ptr + total) : nullptr;
    }
    WsolaArgs a{};
    a.src = s->samples;
    a.srcOff = wn ? d64 + 2 * n1 + kWarpBin : s->off;
    a.nSounds = wn ? 2 * n_targets : s->n;
    a.nTargets = n_targets;
    a.search = search;
    a.idx = d32;
    a.outOff = d64;
    a.map = mapDev ? (frame_map ? frame_map + map_offsets[0] : nullptr) : dMap;
    a.mapOff = d64 + n1;
    a.mapFrames = d32 + n_targets;
    a.pairLen = mapDev ? pair_len : (upLen ? d32 + 2 * (size_t)n_targets : nullptr);
    a.win = reinterpret_cast<const double *>(d64 + 2 * n1);
    a.pos = dPos;
    a.out = dOut;
    a.pcm = dPcm;
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], st));
    if (doSearch) {
        const size_t lds = (size_t)(2 * kWarpBin + 2 * search) * sizeof(double);
        wsola_search_kernel<<<std::min<unsigned>(n_targets, kWsolaMaxGrid), 256, lds, st>>>(a);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[1], st));
    dim3 grid((unsigned)((maxLen + kWarpChunk - 1) / kWarpChunk), n_targets);
    wsola_synth_kernel<<<grid, 256, 0, st>>>(a);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ctx->ev[2], st));
    std::vector<uint64_t> hostPos(posBack ? (size_t)mapTotal : 0);
    if (!outDev) {
        if (out_samples)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_samples, dOut, total * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out_pcm32)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_pcm32, dPcm, total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (posBack)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(hostPos.data(), dPos, posBytes, hipMemcpyDeviceToHost, st));
    }
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));       // the call's one synchronisation (the host blocks above live until here)
    for (size_t i = 0; i < hostPos.size(); ++i)
        if (hostPos[i] != kWsolaUnset)                   // a position is below 2^41
            out_pos[map_offsets[0] + i] = hostPos[i];
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
        return reconstruct_wsola(ctx, s, idx, out_offsets, n_targets, frame_map, map_offsets, map_frames, pair_len, search,
                                 flags, out_pos, out_samples, out_pcm32);
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
        if (ctx && (!win_first || !win_len)) {
            ctx->err = "ssym_reconstruct_wsola_spans: win_first and win_len must not be NULL";
            return SSYM_E_INVALID;
        }
        SampleWindows wn;
        wn.first = win_first;
        wn.len = win_len;
        return reconstruct_wsola(ctx, s, idx, out_offsets, n_targets, frame_map, map_offsets, map_frames, pair_len, search,
                                 flags, out_pos, out_samples, out_pcm32, wn, "ssym_reconstruct_wsola_spans");
    });
}

}  // extern "C"
