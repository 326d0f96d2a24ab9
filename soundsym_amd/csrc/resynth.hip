// resynth.hip -- live resynthesis: committed mosaic frames to audio, push by push (DESIGN.md 2 "Live resynthesis", 5.27; the
// header carries the definition, tests/live_resynth_ref.py restates it).
//
// Role on the path: reconstruct_mosaic renders whole pieces through ssym_reconstruct_warped_spans / _wsola_spans, whose sample
// window ends at (source_last + 1) * HOP -- not known while a piece is open.  A resynthesiser is the resumable form, lane by
// lane, as a mosaicker is ssym_dtw_mosaic's: it takes committed frames (from a mosaicker's frame log device to device, or
// from host arrays), releases every output hop as soon as its bits can no longer change, and from reset to flush its output
// is the offline render's, bit for bit.  Device state is a ring of 16 frames per lane.
//
// Definition.  HOP, BIN, w[], the taps / value / pcm rules, the pos[] chain and the window rule are those of "Warped
// reconstruction", "WSOLA" and "Spans", word for word.  One lane receives frames (src, frame, start) in column order.
//   tile     : starts at every frame with start = 1.  A sounding tile a...b has map[j] = frame_j, first = map[a], last = map[b];
//              within a tile map steps by 0, 1 or 2, never by 0 twice in a row.  src = SSYM_COVER_GAP: a gap frame, a tile of
//              its own.
//   output   : tile i owns (b - a + 1) * HOP samples, the last tile N - a * HOP (N: the flush's total_samples).  A sounding tile
//              is the _spans call's output for the window [min(first * HOP, n_src), min((last + 1) * HOP, n_src)) of sound src,
//              the map map - first, pos[0] = 0 at the tile's first frame.  A gap tile is +0.0; a lane without frames N zeros.
//              Hop j is samples [j * HOP, (j + 1) * HOP); its taps are frames max(a, j - 3) ... j of its own tile only.
//   release  : L = the map value of the latest frame of the open tile.  Hop j is released, in column order, when its tile is
//              closed (a later start has arrived, or the flush), when map[j] + R <= L (R = 2 for search = 0, else
//              floor((search + 1279) / 256)), or at once when it is a gap frame.  An open tile is rendered with the window end
//              (L + 1) * HOP, clipped to n_src.
//   why      : search = 0: a tap j' of hop j reads source hops up to map[j'] + (j - j'); two consecutive steps sum to 1 at
//              least, so that is at most map[j] + 2.  search > 0: the template reads up to pos[j-1] + HOP + BIN - 1 <=
//              map[j] * HOP + search + 1279; candidates, admissibility and taps reach less far.  Every read that decides a
//              released hop lies below (L + 1) * HOP: a later `last` cannot change it.  At most 2 R hops of a lane are held.
//   flush    : closes the open tile, releases the rest and the tail total_samples - frames * HOP; the lane has then ENDED.
//
// Mapping.
//   feed     resynth_feed_kernel, one thread per lane, serial over the lane's new frames: appends them to the ring (column j
//            at j mod 16: the unreleased frames and the three before them with their pos), closes tiles, applies the release
//            rule and writes one hop entry per released hop into the call's hop list -- where its window starts in the store,
//            the window's length, its nominal position and its tile -- behind three entries of history (tile and pos of the
//            three columns before).  A flush adds the tail's hops: entries that are no tap of anything.
//   search   resynth_search_kernel (search > 0), one 256-thread workgroup per lane, serial over the hops released in this
//            call: each step is wsola_step (warp_common.hpp), the one wsola_search_kernel runs; pos goes into the hop list and,
//            for the last three, back into the ring.
//   synth    resynth_synth_kernel: warp_synth's gather, one thread per output sample, one 256-thread workgroup per (lane, 16
//            hops).  The 19 entries that reach into the workgroup's hops sit in LDS; a tap counts only when its entry's tile
//            is the hop's and p < the window's length, tested before the load: no frame content reads outside the store.
// No workgroup waits on another; stream order is the only ordering between kernels.  No atomics.
// Host: check_handle, the lane limit, the lane check of flush / reset and the sample log (a LaneLog, one entry per sample) are
// lane_feed.hpp's.  One synchronisation per call: the released counts depend on device data and come back with it.
#include "lane_feed.hpp"
#include "warp_common.hpp"

namespace ssym {

constexpr uint32_t kResynthMaxLanes = 65535;                     // the synthesis grid's y
constexpr uint32_t kResynthRing = 16;                            // frames per lane on the device
constexpr uint32_t kResynthNone = 0xffffffffu;                   // "no tile", "no step"
constexpr int kResynthHops = 16;                                 // hops per synthesis workgroup
constexpr int kResynthEntries = kResynthHops + kWarpTaps - 1;    // 19 entries reach into them
static_assert(2 * ((kWsolaMaxSearch + 1279) / 256) + (kWarpTaps - 1) < kResynthRing, "the ring holds 2 R unreleased frames and 3 before");

// a lane's record on the device
struct RsLane {
    unsigned long long n;        // frames consumed
    unsigned long long rel;      // hops released
    unsigned long long hops;     // hops the last call released
    unsigned long long count;    // ... its tail hops included
    unsigned long long samples;  // samples the last call released
    uint32_t a;                  // the open tile: its first column,
    uint32_t src;                // its sound (or SSYM_COVER_GAP),
    uint32_t first;              // map at its first column,
    uint32_t last;               // L, map at its latest column,
    uint32_t step;               // the latest step (kResynthNone at the tile's first frame)
    uint32_t has;                // 0: no frame yet
};

// a ring slot: column j at j mod 16
struct RsFrame {
    uint32_t map, a;             // the frame's source frame and its tile's first column
    uint64_t pos;                // its position relative to the tile's window, once released
};

// one entry of a call's hop list
struct RsHop {
    uint64_t xoff;               // where the tile's window starts in the store
    uint64_t wlen;               // the window's length at the release: a tap is valid below it
    uint64_t pos;                // the frame's position in the window (the nominal one until the search has run)
    uint32_t a;                  // the frame's tile, as a tap (kResynthNone: no tap of anything)
    uint32_t tile;               // the tile whose taps the hop takes
};

// what one call does with a lane
struct RsStep {
    const uint32_t *src, *frame, *start;     // the new frames (DEVICE)
    uint64_t hopAt;              // the lane's stretch of the hop list: three entries of history, then the released hops
    uint64_t outAt;              // ... and of the samples
    uint64_t tail;               // flush: samples beyond the last frame's hop
    uint32_t m;                  // new frames
    uint32_t flush;
};

}  // namespace ssym

struct ssym_resynth {
    ssym_ctx *ctx = nullptr;
    const ssym_samples *store = nullptr;
    uint32_t nLanes = 0, search = 0, reach = 0;      // reach: R
    // host mirrors of the lanes
    std::vector<uint64_t> consumed, released, samples;
    std::vector<uint8_t> ended;
    std::vector<ssym::RsLane> state;
    // device
    ssym::RsLane *lanes = nullptr;           // [nLanes]
    ssym::RsFrame *ring = nullptr;           // [nLanes][16]
    ssym::RsStep *dSteps = nullptr;          // [nLanes]
    double *win = nullptr;                   // [1024]
    ssym::RsHop *hops = nullptr;             // the last call's hop list
    uint64_t hopCap = 0;
    // the sample log: the samples of the last push / take / flush, one entry per sample (cost: f64, word 0: pcm)
    ssym::LaneLog out{1};
    // the log taken last
    const ssym_mosaicker *tookFrom = nullptr;
    uint64_t tookCall = 0;
};

namespace ssym {
namespace {

constexpr const char *kNoun = "resynth";

__global__ __launch_bounds__(256) void resynth_init_kernel(RsLane *lanes, uint32_t lane0, uint32_t nLanes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nLanes)
        lanes[lane0 + i] = RsLane{0, 0, 0, 0, 0, kResynthNone, SSYM_COVER_GAP, 0, 0, kResynthNone, 0};
}

struct RsArgs {
    const RsStep *steps;
    RsLane *lanes;
    RsFrame *ring;
    RsHop *hops;
    const double *store;         // the store's samples
    const uint64_t *srcOff;      // [nSounds + 1]
    const double *win;           // [1024]
    double *out;
    int32_t *pcm;
    uint32_t nLanes, nSounds, search, reach;
};

__global__ __launch_bounds__(64) void resynth_feed_kernel(const RsArgs a)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.nLanes)
        return;
    const RsStep s = a.steps[l];
    if (s.m == 0 && !s.flush)
        return;
    RsLane st = a.lanes[l];
    RsFrame *ring = a.ring + (size_t)l * kResynthRing;
    RsHop *h = a.hops + s.hopAt;
    // history: tile and pos of the three columns before the first hop this call can release
    for (int i = 0; i < kWarpTaps - 1; ++i) {
        const long long col = (long long)st.rel - (kWarpTaps - 1) + i;
        RsHop o{0, 0, 0, kResynthNone, kResynthNone};
        if (col >= 0) {
            const RsFrame e = ring[(uint64_t)col % kResynthRing];
            o.pos = e.pos;
            o.a = e.a;
        }
        h[i] = o;
    }
    // the open tile's window as of now: [base, base + wlen) of the store; nothing for a gap, a sound outside the store or no tile
    auto window = [&](uint64_t &xoff, uint64_t &wlen) {
        xoff = wlen = 0;
        if (!st.has || st.src >= a.nSounds)
            return;
        const uint64_t s0 = a.srcOff[st.src], nSrc = a.srcOff[st.src + 1] - s0;
        const uint64_t base = std::min<uint64_t>((uint64_t)st.first * kWarpHop, nSrc);
        const uint64_t end = std::min<uint64_t>(((uint64_t)st.last + 1) * kWarpHop, nSrc);
        xoff = s0 + base;
        wlen = end > base ? end - base : 0;
    };
    uint64_t cnt = 0;
    // column st.rel leaves: it belongs to the open tile
    auto release = [&]() {
        RsFrame &e = ring[st.rel % kResynthRing];
        RsHop o;
        window(o.xoff, o.wlen);
        if (e.map < st.first)                    // (no frame a push accepts: the tile's maps do not decrease)
            o.wlen = 0;
        o.pos = (uint64_t)(e.map - st.first) * kWarpHop;
        o.a = o.tile = e.a;
        e.pos = o.pos;                           // search > 0: the search kernel puts the searched one there
        h[(kWarpTaps - 1) + cnt] = o;
        ++cnt;
        ++st.rel;
    };
    for (uint32_t k = 0; k < s.m; ++k) {
        const uint32_t src = s.src[k], f = s.frame[k];
        if (s.start[k] || !st.has) {
            while (st.rel < st.n)
                release();                       // the tile is closed
            st.a = (uint32_t)st.n;
            st.src = src;
            st.first = st.last = f;
            st.step = kResynthNone;
            st.has = 1;
        } else {
            st.step = f - st.last;
            st.last = f;
        }
        ring[st.n % kResynthRing] = RsFrame{f, st.a, 0};
        ++st.n;
        if (st.src == SSYM_COVER_GAP) {
            release();                           // a gap frame leaves at once
            continue;
        }
        while (st.rel < st.n && ((uint64_t)ring[st.rel % kResynthRing].map + a.reach <= st.last ||
                                 st.n - st.rel > kResynthRing - (kWarpTaps - 1)))       // (the latter: no paced map gets there)
            release();
    }
    if (s.flush)
        while (st.rel < st.n)
            release();
    st.hops = cnt;
    st.samples = cnt * kWarpHop + s.tail;
    if (s.flush) {
        // the tail's hops take the last tile's taps and are no tap themselves
        RsHop o;
        window(o.xoff, o.wlen);
        o.pos = 0;
        o.a = kResynthNone;
        o.tile = st.has ? st.a : kResynthNone;
        for (uint64_t t = 0; t < (s.tail + kWarpHop - 1) / kWarpHop; ++t)
            h[(kWarpTaps - 1) + cnt++] = o;
    }
    st.count = cnt;
    a.lanes[l] = st;
}

// the positions of the hops released in this call, lane by lane: WSOLA's chain, continued from the ring
__global__ __launch_bounds__(256) void resynth_search_kernel(const RsArgs a)
{
    extern __shared__ double sm[];               // [BIN] template, then [BIN + 2 S] candidate span
    __shared__ double wScore[4];
    __shared__ int wLag[4];
    const WsolaStep w(sm, wScore, wLag, a.search);
    const uint32_t l = blockIdx.x;
    const RsStep s = a.steps[l];
    if (s.m == 0 && !s.flush)
        return;
    const uint64_t hops = a.lanes[l].hops, col0 = a.lanes[l].rel - hops;
    RsHop *h = a.hops + s.hopAt;
    RsFrame *ring = a.ring + (size_t)l * kResynthRing;
    uint64_t prev = h[kWarpTaps - 2].pos;        // pos of the column before the first hop
    for (uint64_t r = 0; r < hops; ++r) {
        const RsHop e = h[(kWarpTaps - 1) + r];
        const uint64_t col = col0 + r;
        uint64_t pos = e.pos;                    // the tile's first frame: pos[0] = 0
        if ((uint64_t)e.a != col)
            pos = (uint64_t)((int64_t)e.pos + (int64_t)wsola_step(w, a.store + e.xoff, e.wlen, prev, (int64_t)e.pos));
        prev = pos;
        if (w.tid == 0) {
            h[(kWarpTaps - 1) + r].pos = pos;
            if (r + (kWarpTaps - 1) >= hops)     // the next call's history
                ring[col % kResynthRing].pos = pos;
        }
    }
}

// warp_synth's gather over a call's hop list: grid (16-hop groups, lanes)
__global__ __launch_bounds__(256) void resynth_synth_kernel(const RsArgs a)
{
    __shared__ RsHop sHop[kResynthEntries];
    const uint32_t l = blockIdx.y, tid = threadIdx.x;
    const RsStep s = a.steps[l];
    if (s.m == 0 && !s.flush)
        return;
    const uint64_t count = a.lanes[l].count, samples = a.lanes[l].samples;
    const uint64_t h0 = (uint64_t)blockIdx.x * kResynthHops;
    if (h0 >= count)
        return;                                  // the whole workgroup: no hop of this lane in the group
    if (tid < (uint32_t)kResynthEntries) {
        if (h0 + tid < count + (kWarpTaps - 1))
            sHop[tid] = a.hops[s.hopAt + h0 + tid];
        else
            sHop[tid] = RsHop{0, 0, 0, kResynthNone, kResynthNone};      // beyond the lane's hops: no tap of anything
    }
    // a thread only ever needs the window at tid, tid + 256, tid + 512 and tid + 768
    const double w0 = a.win[tid], w1 = a.win[tid + 256], w2 = a.win[tid + 512], w3 = a.win[tid + 768];
    __syncthreads();

    for (int u = 0; u < kResynthHops && h0 + (uint64_t)u < count; ++u) {
        const uint64_t k = (h0 + (uint64_t)u) * kWarpHop + tid;
        if (k >= samples)
            continue;                            // the last hop of a flush's tail
        const uint64_t wlen = sHop[u + kWarpTaps - 1].wlen;
        const uint32_t tile = sHop[u + kWarpTaps - 1].tile;
        const double *__restrict__ x = a.store + sHop[u + kWarpTaps - 1].xoff;
        double num = 0.0, den = 0.0;
        // tap i in ascending column: entry u + i, window quarter q = 3 - i
        auto tap = [&](int i, double wv) {
            const uint64_t p = sHop[u + i].pos + (uint64_t)(tid + 256 * (kWarpTaps - 1 - i));
            if (sHop[u + i].a == tile && p < wlen) {       // tested before the load: no frame content reads outside x
                num = __dadd_rn(num, __dmul_rn(wv, x[p]));
                den = __dadd_rn(den, wv);
            }
        };
        tap(0, w3);
        tap(1, w2);
        tap(2, w1);
        tap(3, w0);
        const double r = den > 0.0 ? __ddiv_rn(num, den) : 0.0;
        a.out[s.outAt + k] = r;
        a.pcm[s.outAt + k] = warp_pcm32(r);
    }
}

void resynth_free(ssym_ctx *ctx, ssym_resynth *rs)
{
    for (void *p : {(void *)rs->lanes, (void *)rs->ring, (void *)rs->dSteps, (void *)rs->win, (void *)rs->hops})
        if (p)
            dev_free(ctx, p);
    rs->out.free(ctx);
    delete rs;
}

LaneFeed feed_of(const ssym_resynth *rs)
{
    return LaneFeed{kNoun, "out_n_samples", rs->nLanes, 0, rs->consumed, &rs->ended, false, nullptr};
}

int32_t refuse(ssym_ctx *ctx, const char *fn, const std::string &what, int32_t rc = SSYM_E_INVALID)
{
    ctx->err = fn + (": " + what);
    return rc;
}

int32_t resynth_create(ssym_ctx *ctx, const ssym_samples *store, uint32_t n_lanes, uint32_t search, ssym_resynth **out)
{
    const char *fn = "ssym_resynth_create";
    if (!out)
        return refuse(ctx, fn, "out is NULL");
    *out = nullptr;
    if (!store || n_lanes == 0)
        return refuse(ctx, fn, "the sample store is NULL or n_lanes is 0");
    if (search > kWsolaMaxSearch)
        return refuse(ctx, fn, "search must not exceed 512 samples");
    if (store->n == 0)
        return refuse(ctx, fn, "empty sample store", SSYM_E_EMPTY_DICT);
    if (n_lanes > kResynthMaxLanes)
        return refuse(ctx, fn, "more than " + std::to_string(kResynthMaxLanes) + " lanes", SSYM_E_UNSUPPORTED);
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ssym_resynth *rs = new ssym_resynth;
    rs->ctx = ctx;
    rs->store = store;
    rs->nLanes = n_lanes;
    rs->search = search;
    rs->reach = search ? (search + 1279) / 256 : 2;
    rs->consumed.assign(n_lanes, 0);
    rs->released.assign(n_lanes, 0);
    rs->samples.assign(n_lanes, 0);
    rs->ended.assign(n_lanes, 0);
    rs->state.assign(n_lanes, RsLane{0, 0, 0, 0, 0, kResynthNone, SSYM_COVER_GAP, 0, 0, kResynthNone, 0});
    int32_t rc = alloc_n(ctx, &rs->lanes, (size_t)n_lanes);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &rs->ring, (size_t)n_lanes * kResynthRing);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &rs->dSteps, (size_t)n_lanes);
    if (rc == SSYM_OK)
        rc = alloc_n(ctx, &rs->win, (size_t)kWarpBin);
    if (rc != SSYM_OK) {
        resynth_free(ctx, rs);
        return rc;
    }
    hipError_t e = hipMemcpyAsync(rs->win, warp_window().data(), sizeof(double) * kWarpBin, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(rs->ring, 0, sizeof(RsFrame) * (size_t)n_lanes * kResynthRing, ctx->stream);
    if (e == hipSuccess) {
        resynth_init_kernel<<<(n_lanes + 255) / 256, 256, 0, ctx->stream>>>(rs->lanes, 0u, n_lanes);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->err = std::string(fn) + ": " + hipGetErrorString(e);
        resynth_free(ctx, rs);
        return SSYM_E_HIP;
    }
    *out = rs;
    return SSYM_OK;
}

// The body of push, take and flush.  src / frame / start: lane l's m[l] new frames from at[l] on (DEVICE); flushLane: the
// lane to flush (tail samples behind its frames), or kResynthNone.
int32_t resynth_run(ssym_ctx *ctx, ssym_resynth *rs, const uint32_t *src, const uint32_t *frame, const uint32_t *start,
                    const std::vector<uint64_t> &at, const std::vector<uint64_t> &m, uint32_t flushLane, uint64_t tail,
                    uint64_t *out_n_samples)
{
    const uint32_t nL = rs->nLanes;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    // room: a lane releases no more hops than it holds unreleased and receives, and the tail's
    std::vector<RsStep> steps(nL);
    uint64_t hopNeed = 0, outNeed = 0, maxHops = 0;
    rs->out.off.assign((size_t)nL + 1, 0);
    rs->out.count.assign(nL, 0);
    for (uint32_t l = 0; l < nL; ++l) {
        RsStep &s = steps[l];
        s = RsStep{nullptr, nullptr, nullptr, hopNeed, outNeed, 0, (uint32_t)m[l], l == flushLane ? 1u : 0u};
        rs->out.off[l] = outNeed;
        if (!s.m && !s.flush)
            continue;
        if (s.m) {
            s.src = src + at[l];
            s.frame = frame + at[l];
            s.start = start + at[l];
        }
        uint64_t room = rs->consumed[l] - rs->released[l] + m[l];
        if (s.flush) {
            s.tail = tail;
            room += (tail + kWarpHop - 1) / kWarpHop;
        }
        hopNeed += room + (kWarpTaps - 1);
        outNeed += room * kWarpHop;
        maxHops = std::max(maxHops, room);
    }
    rs->out.off[nL] = outNeed;
    if (hopNeed > rs->hopCap) {
        const uint64_t grown = pow2_at_least(std::max<uint64_t>(hopNeed, 256));
        RsHop *p = nullptr;
        const int32_t rc = alloc_n(ctx, &p, (size_t)grown);
        if (rc != SSYM_OK)
            return rc;
        if (rs->hops)
            dev_free(ctx, rs->hops);             // (every call ends synchronised: no kernel reads the old list)
        rs->hops = p;
        rs->hopCap = grown;
    }
    int32_t rc = rs->out.room(ctx, outNeed);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(rs->dSteps, steps.data(), sizeof(RsStep) * nL, hipMemcpyHostToDevice, st));
    RsArgs k{rs->dSteps, rs->lanes, rs->ring, rs->hops, rs->store->samples, rs->store->off, rs->win, rs->out.cost,
             (int32_t *)rs->out.word(0), nL, rs->store->n, rs->search, rs->reach};
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    resynth_feed_kernel<<<(nL + 63) / 64, 64, 0, st>>>(k);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    if (rs->search) {
        const size_t lds = (size_t)(2 * kWarpBin + 2 * rs->search) * sizeof(double);
        resynth_search_kernel<<<nL, 256, lds, st>>>(k);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    if (maxHops) {
        resynth_synth_kernel<<<dim3((unsigned)((maxHops + kResynthHops - 1) / kResynthHops), nL), 256, 0, st>>>(k);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    SSYM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
    std::vector<RsLane> state(nL);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(state.data(), rs->lanes, sizeof(RsLane) * nL, hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    uint64_t total = 0;
    for (uint32_t l = 0; l < nL; ++l) {
        if (!steps[l].m && !steps[l].flush)
            continue;
        rs->state[l] = state[l];
        rs->consumed[l] = state[l].n;
        rs->released[l] = state[l].rel;
        rs->samples[l] += state[l].samples;
        rs->out.count[l] = state[l].samples;
        total += state[l].samples;
    }
    if (flushLane != kResynthNone)
        rs->ended[flushLane] = 1;
    *out_n_samples = total;
    ssym_timings tm{};
    tm.main_ms = rs->search ? ev_ms(ev[1], ev[2]) : 0.f;                  // the search
    tm.reduce_ms = ev_ms(ev[0], ev[1]) + ev_ms(ev[2], ev[3]);             // staging and synthesis
    tm.total_ms = ev_ms(ev[0], ev[3]);
    tm.main_launches = rs->search ? 1 : 0;
    for (uint32_t l = 0; l < nL; ++l)
        tm.n_pairs += m[l];                                               // frames
    ctx->timings = tm;
    return SSYM_OK;
}

int32_t resynth_push(ssym_ctx *ctx, ssym_resynth *rs, const uint32_t *lane, const uint32_t *column, const uint32_t *src,
                     const uint32_t *frame, const uint32_t *start, uint64_t n_frames, uint64_t *out_n_samples)
{
    const char *fn = "ssym_resynth_push";
    int32_t rc = check_handle(ctx, rs, kNoun, fn);
    if (rc != SSYM_OK)
        return rc;
    if (!out_n_samples || (n_frames && (!lane || !column || !src || !frame || !start)))
        return refuse(ctx, fn, "lane, column, src, frame, start and out_n_samples must not be NULL");
    const uint32_t nL = rs->nLanes;
    const LaneFeed feed = feed_of(rs);
    std::vector<uint64_t> at(nL, 0), m(nL, 0);
    // the frames against a copy of the lanes' records: a refused push consumes nothing
    std::vector<RsLane> walk;
    uint32_t cur = kResynthNone;
    RsLane w{};
    for (uint64_t k = 0; k < n_frames; ++k) {
        const uint32_t l = lane[k];
        const std::string where = " (entry " + std::to_string(k) + ")";
        if (l >= nL || (cur != kResynthNone && l < cur))
            return refuse(ctx, fn, "a lane is outside the resynthesiser's lanes or the entries are not ordered by (lane, column)" + where);
        if (l != cur) {
            cur = l;
            w = rs->state[l];
            at[l] = k;
        }
        if ((uint64_t)column[k] != w.n)
            return refuse(ctx, fn, "lane " + std::to_string(l) + " has consumed " + std::to_string(w.n) + " frames, and column " +
                                       std::to_string(column[k]) + " does not continue them" + where);
        if (rs->ended[l])
            return refuse(ctx, fn, "lane " + std::to_string(l) + " was flushed and has ended; call ssym_resynth_reset");
        if (!w.has && !start[k])
            return refuse(ctx, fn, "the first frame of lane " + std::to_string(l) + " starts no tile" + where);
        if (src[k] != SSYM_COVER_GAP && src[k] >= rs->store->n)
            return refuse(ctx, fn, "src is neither a sound of the store nor SSYM_COVER_GAP" + where);
        if (start[k]) {
            w.src = src[k];
            w.first = w.last = frame[k];
            w.step = kResynthNone;
            w.has = 1;
        } else {
            const uint32_t step = frame[k] - w.last;
            if (w.src == SSYM_COVER_GAP || src[k] != w.src || frame[k] < w.last || step > 2 || (step == 0 && w.step == 0))
                return refuse(ctx, fn, "within a tile the frames name one sound and step by 0, 1 or 2, never by 0 twice in a row; a gap frame starts a tile" + where);
            w.step = step;
            w.last = frame[k];
        }
        ++w.n;
        ++m[l];
        rc = feed.check_lane_room(ctx, fn, l, rs->consumed[l], m[l]);
        if (rc != SSYM_OK)
            return rc;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    Blocks bl(ctx);
    uint32_t *dev = nullptr;
    if (n_frames) {
        rc = bl.get(&dev, (size_t)n_frames * 3);
        if (rc != SSYM_OK)
            return rc;
        const uint32_t *from[3] = {src, frame, start};
        for (int i = 0; i < 3; ++i)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dev + (size_t)i * n_frames, from[i], sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice,
                                               ctx->stream));
    }
    return resynth_run(ctx, rs, dev, dev + n_frames, dev + 2 * n_frames, at, m, kResynthNone, 0, out_n_samples);
}

int32_t resynth_take(ssym_ctx *ctx, ssym_resynth *rs, const ssym_mosaicker *mk, uint64_t *out_n_samples)
{
    const char *fn = "ssym_resynth_take";
    int32_t rc = check_handle(ctx, rs, kNoun, fn);
    if (rc != SSYM_OK)
        return rc;
    if (!mk || !out_n_samples)
        return refuse(ctx, fn, "the mosaicker and out_n_samples must not be NULL");
    const MosaickerLog log = mosaicker_log(mk);
    if (log.ctx != ctx)
        return refuse(ctx, fn, "the mosaicker belongs to another context");
    const uint32_t nL = rs->nLanes;
    if (log.nLanes != nL)
        return refuse(ctx, fn, "the mosaicker has " + std::to_string(log.nLanes) + " lanes, the resynthesiser " + std::to_string(nL));
    if (rs->tookFrom == mk && rs->tookCall == log.calls)
        return refuse(ctx, fn, "the mosaicker's last frame log was taken already");
    if (log.calls == 0 || log.log->count.size() != nL)
        return refuse(ctx, fn, "the mosaicker has no frame log yet");
    const LaneFeed feed = feed_of(rs);
    std::vector<uint64_t> at(nL, 0), m(nL, 0);
    for (uint32_t l = 0; l < nL; ++l) {
        m[l] = log.log->count[l];
        at[l] = log.log->off[l];
        if (!m[l])
            continue;
        const int64_t first = (*log.done)[l] + 1 - (int64_t)m[l];
        if (first < 0 || (uint64_t)first != rs->consumed[l])
            return refuse(ctx, fn, "lane " + std::to_string(l) + " has consumed " + std::to_string(rs->consumed[l]) +
                                       " frames, and the log's column " + std::to_string(first) + " does not continue them");
        if (rs->ended[l])
            return refuse(ctx, fn, "lane " + std::to_string(l) + " was flushed and has ended; call ssym_resynth_reset");
        rc = feed.check_lane_room(ctx, fn, l, rs->consumed[l], m[l]);
        if (rc != SSYM_OK)
            return rc;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    rc = resynth_run(ctx, rs, log.log->word(2), log.log->word(3), log.log->word(4), at, m, kResynthNone, 0, out_n_samples);
    if (rc == SSYM_OK) {
        rs->tookFrom = mk;
        rs->tookCall = log.calls;
    }
    return rc;
}

int32_t resynth_flush(ssym_ctx *ctx, ssym_resynth *rs, uint32_t lane, uint64_t total_samples, uint64_t *out_n_samples)
{
    const char *fn = "ssym_resynth_flush";
    int32_t rc = check_handle(ctx, rs, kNoun, fn);
    if (rc == SSYM_OK)
        rc = feed_of(rs).lane(ctx, fn, lane, true, out_n_samples);
    if (rc != SSYM_OK)
        return rc;
    if (rs->ended[lane])
        return refuse(ctx, fn, "lane " + std::to_string(lane) + " was flushed and has ended; call ssym_resynth_reset");
    if (total_samples < rs->consumed[lane] * kWarpHop)
        return refuse(ctx, fn, "total_samples is less than the lane's frames x 256");
    const std::vector<uint64_t> none(rs->nLanes, 0);
    return resynth_run(ctx, rs, nullptr, nullptr, nullptr, none, none, lane, total_samples - rs->consumed[lane] * kWarpHop,
                       out_n_samples);
}

int32_t resynth_reset(ssym_ctx *ctx, ssym_resynth *rs, uint32_t lane)
{
    const char *fn = "ssym_resynth_reset";
    int32_t rc = check_handle(ctx, rs, kNoun, fn);
    if (rc == SSYM_OK)
        rc = feed_of(rs).lane(ctx, fn, lane, false, nullptr);
    if (rc != SSYM_OK)
        return rc;
    resynth_init_kernel<<<1, 256, 0, ctx->stream>>>(rs->lanes, lane, 1u);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    rs->state[lane] = RsLane{0, 0, 0, 0, 0, kResynthNone, SSYM_COVER_GAP, 0, 0, kResynthNone, 0};
    rs->consumed[lane] = rs->released[lane] = rs->samples[lane] = 0;
    rs->ended[lane] = 0;
    return SSYM_OK;
}

int32_t resynth_samples(ssym_ctx *ctx, const ssym_resynth *rs, uint64_t *out_lane_offsets, double *out_samples, int32_t *out_pcm32,
                        uint32_t flags)
{
    const char *fn = "ssym_resynth_samples";
    int32_t rc = check_handle(ctx, rs, kNoun, fn);
    if (rc != SSYM_OK)
        return rc;
    if (flags & ~(uint32_t)SSYM_OUT_DEVICE)
        return refuse(ctx, fn, "unknown flag bits");
    if (out_lane_offsets) {
        uint64_t to = 0;
        for (uint32_t l = 0; l < rs->nLanes; ++l) {
            out_lane_offsets[l] = to;
            to += l < rs->out.count.size() ? rs->out.count[l] : 0;
        }
        out_lane_offsets[rs->nLanes] = to;
    }
    if (!out_samples && !out_pcm32)
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint32_t *const outs[1] = {(uint32_t *)out_pcm32};
    return rs->out.copy(ctx, out_samples, outs, (flags & SSYM_OUT_DEVICE) != 0);
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_resynth_create(ssym_ctx *ctx, const ssym_samples *store, uint32_t n_lanes, uint32_t search, ssym_resynth **out)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return resynth_create(ctx, store, n_lanes, search, out); });
}

int32_t ssym_resynth_destroy(ssym_ctx *ctx, ssym_resynth *rs)
{
    return lane_destroy(ctx, rs, resynth_free);
}

int32_t ssym_resynth_push(ssym_ctx *ctx, ssym_resynth *rs, const uint32_t *lane, const uint32_t *column, const uint32_t *src,
                          const uint32_t *frame, const uint32_t *start, uint64_t n_frames, uint64_t *out_n_samples)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return resynth_push(ctx, rs, lane, column, src, frame, start, n_frames, out_n_samples); });
}

int32_t ssym_resynth_take(ssym_ctx *ctx, ssym_resynth *rs, const ssym_mosaicker *mk, uint64_t *out_n_samples)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return resynth_take(ctx, rs, mk, out_n_samples); });
}

int32_t ssym_resynth_samples(ssym_ctx *ctx, const ssym_resynth *rs, uint64_t *out_lane_offsets, double *out_samples,
                             int32_t *out_pcm32, uint32_t flags)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return resynth_samples(ctx, rs, out_lane_offsets, out_samples, out_pcm32, flags); });
}

int32_t ssym_resynth_flush(ssym_ctx *ctx, ssym_resynth *rs, uint32_t lane, uint64_t total_samples, uint64_t *out_n_samples)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return resynth_flush(ctx, rs, lane, total_samples, out_n_samples); });
}

int32_t ssym_resynth_counts(const ssym_resynth *rs, uint64_t *out_frames, uint64_t *out_samples)
{
    if (!rs)
        return SSYM_E_INVALID;
    if (out_frames)
        std::copy(rs->consumed.begin(), rs->consumed.end(), out_frames);
    if (out_samples)
        std::copy(rs->samples.begin(), rs->samples.end(), out_samples);
    return SSYM_OK;
}

int32_t ssym_resynth_reset(ssym_ctx *ctx, ssym_resynth *rs, uint32_t lane)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t { return resynth_reset(ctx, rs, lane); });
}

}  // extern "C"
