// warp_common.hpp -- what the two resynthesis calls share (warp.hip: plain overlap-add along the frame map; wsola.hip: the
// same overlap-add from searched frame positions): the frame geometry, the window's bits, the 32-bit conversion, the one
// text of the synthesis kernel (warp_synth; warp_kernel and wsola_synth_kernel are its two wrappers) and the one host
// driver path (WarpCall: refusals, staging block, uploads, outputs).  A .hip file keeps its kernels' names, its launches
// and its timings; wsola.hip also the search and the positions.  One step of that search (wsola_step, with wsola_sums and
// wsola_beats) is here too: wsola_search_kernel and the live resynthesis (resynth.hip: resynth_search_kernel) both run it.
//
// Gather form: one thread per output sample, which no other thread writes.  One 256-thread workgroup per (target, 4096-sample chunk),
// as reconstruct_kernel.  Thread `tid` computes samples k = chunk + tid + 256 u, u = 0 .. 15; for a fixed u the whole
// workgroup shares k / 256, so its taps are the same four target frames and m = tid + 256 q, q = 3 .. 0: a thread
// only ever needs the window at tid, tid + 256, tid + 512 and tid + 768, which it keeps in registers.  The chunk touches
// target frames chunk / 256 - 3 ... chunk / 256 + 15: their 19 source positions sit in LDS (sLen for a frame outside
// [0, F): such a tap is never valid), every read of them a broadcast.
#pragma once
#include "ssym_internal.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace ssym {

constexpr int kWarpHop = SSYM_MFCC_HOP, kWarpBin = SSYM_MFCC_BIN;
constexpr int kWarpTaps = kWarpBin / kWarpHop;                    // 4 windows cover a sample
constexpr int kWarpChunk = 4096;                                  // samples per workgroup
constexpr int kWarpFrames = kWarpChunk / kWarpHop + kWarpTaps - 1;    // 19 target frames reach into a chunk
static_assert(kWarpHop == 256 && kWarpTaps == 4 && kWarpFrames == 19, "warp kernels: 256 threads, one hop each");

// (i32::max_value() as f64 * sample) as i32, as reconstruct_kernel: truncate toward zero, saturate, NaN -> 0
__device__ __forceinline__ int32_t warp_pcm32(double v)
{
    const double x = __dmul_rn(2147483647.0, v);
    if (x != x) return 0;
    if (x >= 2147483647.0) return 2147483647;
    if (x <= -2147483648.0) return (int32_t)0x80000000;
    return (int32_t)x;
}

// w[m] = 0.5 - 0.5 cos(2 pi m / 1024): the text of build_tables (mfcc_frame.hpp), so the bits of the MFCC window
inline const std::vector<double> &warp_window()
{
    static const std::vector<double> win = [] {
        const double PI = 3.14159265358979323846;
        std::vector<double> w(kWarpBin);
        for (int i = 0; i < kWarpBin; ++i)
            w[i] = 0.5 - 0.5 * std::cos(2.0 * PI * (double)i / (double)kWarpBin);
        return w;
    }();
    return win;
}

// ---- one step of WSOLA's search (wsola.hip's definition), shared by wsola_search_kernel and resynth_search_kernel ----
constexpr uint32_t kWsolaMaxSearch = 512;
constexpr int kWsolaMaxRounds = (2 * (int)kWsolaMaxSearch + 1 + 255) / 256;      // 5 lags per thread at most
constexpr int kWsolaNone = INT32_MIN;                                            // "no lag yet" in the argmax

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

// The LDS of a search workgroup (256 threads) and what a thread knows of its place in it.  sm: [BIN] template, then
// [BIN + 2 S] candidate span -- (2 BIN + 2 S) doubles of dynamic LDS.
struct WsolaStep {
    double *sT, *sC;
    double *wScore;              // [4]
    int *wLag;                   // [4]
    int tid, wave, S, L, rounds;
    __device__ __forceinline__ WsolaStep(double *sm, double *score, int *lagOut, uint32_t search)
        : sT(sm), sC(sm + kWarpBin), wScore(score), wLag(lagOut), tid((int)threadIdx.x), wave((int)threadIdx.x >> 6), S((int)search),
          L(2 * (int)search + 1)
    {
        // rounds in which this wave owns a lag: lags wave * 64 + 256 r < L
        rounds = L > wave * 64 ? (L - wave * 64 + 255) / 256 : 0;
    }
};

// d* of one step, the same in every thread of the workgroup: x[0 .. sLen) the sound, prev = pos[j-1], nom = map[j] * HOP
// (< 2^40).  The template (8 KiB) and the candidate span x[nom - S .. nom + S + BIN) (<= 16 KiB) go to LDS; thread tid owns
// the lags tid, tid + 256, ... and runs their sums in the defined order; the argmax is a butterfly over the wave and a pass
// over the four waves' winners -- the order (score, -|d|, -d) is total over distinct lags, so the tree's shape cannot
// change the winner.  Every thread of the workgroup calls it, S > 0 or not.
__device__ __forceinline__ int wsola_step(const WsolaStep &w, const double *__restrict__ x, uint64_t sLen, uint64_t prev, int64_t nom)
{
    const int tid = w.tid, S = w.S, L = w.L, rounds = w.rounds;
    double *sT = w.sT, *sC = w.sC;
    // admissible lags lo .. hi: 0 <= nom + d < sLen (sLen < 2^61: a store of doubles)
    const int64_t lo = nom < (int64_t)S ? -nom : -(int64_t)S;
    const int64_t hi = std::min<int64_t>((int64_t)S, (int64_t)sLen - 1 - nom);
    if (!(S > 0 && lo <= hi))                // the same for every thread of the workgroup
        return 0;
    __syncthreads();                         // the step before has read its template and span
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
            continue;                        // NaN never wins
        if (wsola_beats(sc, d, bs, bd)) {
            bs = sc;
            bd = d;
        }
    }
#pragma unroll
    for (int v = 32; v >= 1; v >>= 1) {
        const double os = __shfl_xor(bs, v, 64);
        const int od = __shfl_xor(bd, v, 64);
        if (wsola_beats(os, od, bs, bd)) {
            bs = os;
            bd = od;
        }
    }
    if ((tid & 63) == 0) {
        w.wScore[w.wave] = bs;
        w.wLag[w.wave] = bd;
    }
    __syncthreads();
    bs = w.wScore[0];
    bd = w.wLag[0];
#pragma unroll
    for (int v = 1; v < 4; ++v)
        if (wsola_beats(w.wScore[v], w.wLag[v], bs, bd)) {
            bs = w.wScore[v];
            bd = w.wLag[v];
        }
    return bd == kWsolaNone ? 0 : bd;
}

namespace {      // the including file's own, as the kernels that take these arguments: their mangled names stay

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

// The synthesis kernel's body.  framePos(o): the source position, in samples, of the target frame listed at map slot o
// (below 2^41, so nothing overflows here): warp_kernel's map[o] * HOP, wsola_synth_kernel's pos[o].
template <class FramePos>
__device__ __forceinline__ void warp_synth(const WarpArgs &a, FramePos framePos)
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
            pos = framePos(a.mapOff[t] + (uint64_t)j);
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

// The one staging block of a call, in ssym_reconstruct's scratch: [out offsets | map offsets | window | window table]
// f64 / u64, then [idx | map frames | pair_len] u32.  Byte offsets from the block's start (the out offsets are at 0): the
// host fill and the kernel arguments both go through at(), the one with the host copy, the other with the device block.
struct WarpLayout {
    size_t mapOff, win, table, idx, mapFrames, pairLen, bytes;
    WarpLayout(uint32_t nTargets, bool windows, bool lengths)
    {
        static_assert(sizeof(double) == sizeof(uint64_t), "one staging block");
        const size_t n = nTargets, words32 = n * (lengths ? 3 : 2);
        mapOff = (n + 1) * sizeof(uint64_t);
        win = 2 * mapOff;
        table = win + kWarpBin * sizeof(double);
        idx = table + (windows ? 2 * n * sizeof(uint64_t) : 0);
        mapFrames = idx + n * sizeof(uint32_t);
        pairLen = mapFrames + n * sizeof(uint32_t);
        bytes = idx + (words32 + 1) / 2 * sizeof(uint64_t);
    }
    template <class T>
    static T *at(void *block, size_t offset) { return reinterpret_cast<T *>((char *)block + offset); }
};

// the _spans entry points' first refusal, before any of the plain call's
inline int32_t warp_windows(ssym_ctx *ctx, const char *fn, const uint64_t *win_first, const uint64_t *win_len, SampleWindows &wn)
{
    if (ctx && (!win_first || !win_len)) {
        ctx->err = std::string(fn) + ": win_first and win_len must not be NULL";
        return SSYM_E_INVALID;
    }
    wn.first = win_first;
    wn.len = win_len;
    return SSYM_OK;
}

// One call of ssym_reconstruct_warped / _wsola or their _spans forms: the caller's arguments, then what the steps below find.
// The steps in the order a driver takes them: check_pointers, (WSOLA: its search width), check, idle, stage, its launches,
// finish.
struct WarpCall {
    ssym_ctx *ctx;
    const ssym_samples *s;
    const uint32_t *idx;
    const uint64_t *out_offsets;
    uint32_t n_targets;
    const uint32_t *frame_map;
    const uint64_t *map_offsets;
    const uint32_t *map_frames, *pair_len;
    uint32_t flags;
    double *out_samples;
    int32_t *out_pcm32;
    SampleWindows wn;                   // both NULL: whole sounds
    const char *fn;                     // the entry point's name, for the messages

    uint64_t maxLen = 0, total = 0, mapTotal = 0;      // longest target, all targets, map slots (check)
    bool anyMap = false;                               // a target has map frames (check)
    bool outDev = false, mapDev = false;               // the flags (stage)
    std::vector<uint64_t> host{};                      // the staging block: lives until finish's synchronisation
    double *dOut = nullptr;                            // where the kernel writes: the caller's device arrays or ctx->part
    int32_t *dPcm = nullptr;

    int32_t refuse(const std::string &what, int32_t rc = SSYM_E_INVALID)
    {
        ctx->err = fn + (": " + what);
        return rc;
    }

    int32_t check_pointers()
    {
        if (!ctx)
            return SSYM_E_INVALID;
        if (!s || !idx || !out_offsets || !map_offsets || !map_frames)
            return refuse("s, idx, out_offsets, map_offsets and map_frames must not be NULL");
        return SSYM_OK;
    }

    // the refusals after the NULL pointers, in their order: target t's offsets and index before its map room, all targets'
    // before the NULL map, the windows last
    int32_t check()
    {
        if (out_offsets[0] != 0)
            return refuse("out_offsets must start at 0");
        if (flags & ~(uint32_t)(SSYM_OUT_DEVICE | SSYM_WARP_MAP_DEVICE))
            return refuse("unknown flag bits");
        if (s->n == 0) {
            ctx->err = "empty dictionary";
            return SSYM_E_EMPTY_DICT;
        }
        for (uint32_t t = 0; t < n_targets; ++t) {
            if (out_offsets[t + 1] < out_offsets[t] || idx[t] >= s->n)
                return refuse("out_offsets decrease or an index is outside the sample store (target " + std::to_string(t) + ")");
            if (map_offsets[t + 1] < map_offsets[t] || map_offsets[t + 1] - map_offsets[t] < map_frames[t])
                return refuse("map_offsets decrease or leave less room than map_frames (target " + std::to_string(t) + ")");
            anyMap = anyMap || map_frames[t] > 0;
            maxLen = std::max<uint64_t>(maxLen, out_offsets[t + 1] - out_offsets[t]);
        }
        if (anyMap && !frame_map)
            return refuse("frame_map is NULL although a target has map frames");
        total = out_offsets[n_targets];
        mapTotal = map_offsets[n_targets] - map_offsets[0];
        return wn ? wn.check(ctx->err, fn, s, idx, n_targets) : SSYM_OK;
    }

    // nothing to do: SSYM_OK before any device work, ctx->timings left alone
    bool idle() const { return n_targets == 0 || total == 0 || (!out_samples && !out_pcm32); }

    // The staging block and (host map) the caller's map, uploaded in one copy each into ctx->best; behind them `extraBytes`
    // (8-byte aligned) for the driver, at *extra; the outputs; the arguments of the synthesis kernel.
    int32_t stage(WarpArgs &a, size_t extraBytes = 0, void **extra = nullptr)
    {
        SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        outDev = (flags & SSYM_OUT_DEVICE) != 0;
        mapDev = (flags & SSYM_WARP_MAP_DEVICE) != 0;
        const bool upLen = !mapDev && pair_len, upMap = !mapDev && anyMap && mapTotal;
        const size_t n1 = (size_t)n_targets + 1;
        const WarpLayout lay(n_targets, (bool)wn, upLen);
        host.assign(lay.bytes / sizeof(uint64_t), 0);
        std::copy(out_offsets, out_offsets + n1, host.data());
        for (size_t t = 0; t < n1; ++t)
            lay.at<uint64_t>(host.data(), lay.mapOff)[t] = map_offsets[t] - map_offsets[0];
        std::copy(warp_window().begin(), warp_window().end(), lay.at<double>(host.data(), lay.win));
        if (wn)
            wn.fill(s, idx, n_targets, lay.at<uint64_t>(host.data(), lay.table), lay.at<uint32_t>(host.data(), lay.idx));
        else
            std::copy(idx, idx + n_targets, lay.at<uint32_t>(host.data(), lay.idx));
        std::copy(map_frames, map_frames + n_targets, lay.at<uint32_t>(host.data(), lay.mapFrames));
        if (upLen)
            std::copy(pair_len, pair_len + n_targets, lay.at<uint32_t>(host.data(), lay.pairLen));
        const size_t mapBytes = upMap ? (((size_t)mapTotal * sizeof(uint32_t) + 7) & ~(size_t)7) : 0;
        int32_t rc = ensure(ctx, ctx->best, lay.bytes + mapBytes + extraBytes + 16);
        if (rc != SSYM_OK)
            return rc;
        void *dev = ctx->best.ptr;
        uint32_t *dMap = lay.at<uint32_t>(dev, lay.bytes);
        if (extra)
            *extra = lay.at<char>(dev, lay.bytes + mapBytes);
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dev, host.data(), lay.bytes, hipMemcpyHostToDevice, st));
        if (upMap)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dMap, frame_map + map_offsets[0], (size_t)mapTotal * sizeof(uint32_t),
                                               hipMemcpyHostToDevice, st));
        dOut = out_samples;
        dPcm = out_pcm32;
        if (!outDev) {
            rc = ensure(ctx, ctx->part, total * (sizeof(double) + sizeof(int32_t)));
            if (rc != SSYM_OK)
                return rc;
            dOut = out_samples ? (double *)ctx->part.ptr : nullptr;
            dPcm = out_pcm32 ? (int32_t *)((double *)ctx->part.ptr + total) : nullptr;
        }
        a.src = s->samples;
        a.srcOff = wn ? lay.at<uint64_t>(dev, lay.table) : s->off;
        a.nSounds = wn ? 2 * n_targets : s->n;
        a.idx = lay.at<uint32_t>(dev, lay.idx);
        a.outOff = lay.at<uint64_t>(dev, 0);
        a.map = mapDev ? (frame_map ? frame_map + map_offsets[0] : nullptr) : dMap;
        a.mapOff = lay.at<uint64_t>(dev, lay.mapOff);
        a.mapFrames = lay.at<uint32_t>(dev, lay.mapFrames);
        a.pairLen = mapDev ? pair_len : (upLen ? lay.at<uint32_t>(dev, lay.pairLen) : nullptr);
        a.win = lay.at<double>(dev, lay.win);
        a.out = dOut;
        a.pcm = dPcm;
        return SSYM_OK;
    }

    // the synthesis kernel's grid
    dim3 grid() const { return dim3((unsigned)((maxLen + kWarpChunk - 1) / kWarpChunk), n_targets); }

    // host outputs copied back from ctx->part, then the call's one synchronisation
    int32_t finish()
    {
        hipStream_t st = ctx->stream;
        if (!outDev && out_samples)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_samples, dOut, total * sizeof(double), hipMemcpyDeviceToHost, st));
        if (!outDev && out_pcm32)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_pcm32, dPcm, total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        return SSYM_OK;
    }
};

}  // namespace
}  // namespace ssym
