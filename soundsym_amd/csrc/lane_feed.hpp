// lane_feed.hpp -- what the lane-fed objects share on the host: the spotter (dtw_spotter.hip), the coverer
// (dtw_coverer.hip) and the mosaicker (dtw_mosaicker.hip) consume growing sounds lane by lane, in pushes of host frames or
// by following a stream's resident frames, and flush or reset one lane.  The checks of those calls, their order, their
// messages and the upload of a push are here once (LaneFeed), and so are the bodies of the four entry points and of destroy
// (lane_push, lane_follow, lane_flush, lane_reset, lane_destroy): an object hands in its feed and what it does with the
// frames (spotter_run; the coverer's and the mosaicker's runs are one loop too, lane_tiling.hpp's tiling_run).  Here as
// well: the log of a call's results that the coverer and the mosaicker keep (LaneLog: its room, its layout at the start of a
// call and the copy out; the spotter's event log keeps its contents while it grows and is sorted, and stays with the
// spotter), and pow2_at_least.  The resynthesiser (resynth.hip) is lane-fed too, with committed frames instead of features:
// it takes check_handle, the lane limit and the lane check of flush / reset from here, keeps its released samples in a
// LaneLog (one entry per sample) and reads the mosaicker's (MosaickerLog); it and the follower (follower.hip) are destroyed
// by lane_destroy.
//
// The order of the refusals is part of the interface ("the earlier of two faults is the one reported"):
//   push   : frame_offsets / count NULL | the object's own check | lane by lane: offsets decrease, the lane has ended,
//            the lane limit | feats NULL | hipSetDevice, upload
//   follow : stream / count NULL | the object's own check | the stream's context | the stream's shape | lane by lane: holds
//            fewer than consumed, the lane limit | hipSetDevice
//   lane   : lane outside the lanes (flush: or count NULL) | hipSetDevice
// and check_handle comes before each of them; the object's run comes behind them.
#pragma once

#include "ssym_internal.hpp"

#include <algorithm>
#include <functional>

namespace ssym {

// frames a lane may consume: its row numbers, ends and cut points are reported as u32, and 0xffffffff means none
constexpr uint64_t kLaneMaxFrames = 2147483647;          // 2^31 - 1
constexpr uint32_t kLaneNone = 0xffffffffu;              // the lane to flush of a call that flushes none

template <class T>
int32_t alloc_n(ssym_ctx *ctx, T **p, size_t count)
{
    return dev_alloc(ctx, (void **)p, std::max<size_t>(count * sizeof(T), 8));
}

// n values of T from device memory to an output that is host memory, or device memory with SSYM_OUT_DEVICE
template <class T>
int32_t copy_out(ssym_ctx *ctx, T *out, const T *dev, size_t n, bool outDev)
{
    if (out && n)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out, dev, sizeof(T) * n, outDev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                           ctx->stream));
    return SSYM_OK;
}

inline uint64_t pow2_at_least(uint64_t x)
{
    uint64_t p = 1;
    while (p < x)
        p <<= 1;
    return p;
}

// The log of a call (the coverer's pieces, the mosaicker's frames): what the last push / follow / flush emitted, one f64
// array and nWords u32 arrays of `cap` entries each, lane l's entries from off[l] on, count[l] of them.  The commit kernels
// fill it; the call that reads it copies the lanes' stretches out one behind the other.
struct LaneLog {
    uint32_t nWords;
    double *cost = nullptr;                              // [cap]
    uint32_t *words = nullptr;                           // [nWords][cap]
    uint64_t cap = 0;
    std::vector<uint64_t> off, count;                    // [nLanes + 1], [nLanes]

    explicit LaneLog(uint32_t n) : nWords(n) {}
    uint32_t *word(uint32_t w) const { return words + w * cap; }

    // room for `need` entries; what the log held is dropped (a call's log starts empty)
    int32_t room(ssym_ctx *ctx, uint64_t need)
    {
        if (need <= cap)
            return SSYM_OK;
        const uint64_t grown = pow2_at_least(std::max<uint64_t>(need, 256));
        double *c = nullptr;
        uint32_t *w = nullptr;
        int32_t rc = alloc_n(ctx, &c, (size_t)grown);
        if (rc == SSYM_OK)
            rc = alloc_n(ctx, &w, nWords * (size_t)grown);
        if (rc != SSYM_OK) {
            if (c)
                dev_free(ctx, c);
            return rc;
        }
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        free(ctx);
        cost = c;
        words = w;
        cap = grown;
        return SSYM_OK;
    }

    // a call begins: lane l with new frames (m[l]) or the flush has room for an entry per frame beyond done[l] -- an entry
    // has a frame at least, so a lane emits no more
    int32_t begin(ssym_ctx *ctx, const std::vector<uint64_t> &consumed, const std::vector<int64_t> &done,
                  const std::vector<uint64_t> &m, uint32_t flushLane)
    {
        const uint32_t nL = (uint32_t)m.size();
        off.assign((size_t)nL + 1, 0);
        count.assign(nL, 0);
        uint64_t need = 0;
        for (uint32_t l = 0; l < nL; ++l) {
            off[l] = need;
            if (m[l] || l == flushLane)
                need += consumed[l] + m[l] - (uint64_t)(done[l] + 1);
        }
        off[nL] = need;
        return room(ctx, need);
    }

    uint64_t total() const
    {
        uint64_t n = 0;
        for (const uint64_t c : count)
            n += c;
        return n;
    }

    // the lanes' stretches, one behind the other, into the outputs that are not NULL (outs: nWords of them); synchronises
    int32_t copy(ssym_ctx *ctx, double *out_cost, uint32_t *const *outs, bool outDev) const
    {
        size_t to = 0;
        for (size_t l = 0; l < count.size(); ++l) {
            const size_t from = off[l], n = count[l];
            int32_t rc = copy_out(ctx, out_cost ? out_cost + to : nullptr, (const double *)cost + from, n, outDev);
            for (uint32_t w = 0; w < nWords && rc == SSYM_OK; ++w)
                rc = copy_out(ctx, outs[w] ? outs[w] + to : nullptr, (const uint32_t *)word(w) + from, n, outDev);
            if (rc != SSYM_OK)
                return rc;
            to += n;
        }
        if (to)
            SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return SSYM_OK;
    }

    void free(ssym_ctx *ctx)
    {
        for (void *p : {(void *)cost, (void *)words})
            if (p)
                dev_free(ctx, p);
        cost = nullptr;
        words = nullptr;
        cap = 0;
    }
};

// The mosaicker's last frame log where it lies (dtw_mosaicker.hip): what the resynthesiser (resynth.hip) takes device to
// device.  Words 2, 3 and 4 are src, frame and start; lane l's first entry is column (*done)[l] + 1 - log->count[l]; `calls`
// names the log (it counts the calls that began one).
struct MosaickerLog {
    const ssym_ctx *ctx;
    uint32_t nLanes;
    const LaneLog *log;
    const std::vector<int64_t> *done;
    uint64_t calls;
};
MosaickerLog mosaicker_log(const ssym_mosaicker *mk);

// what every call refuses before anything else; noun: "spotter", "coverer", "mosaicker", "resynthesiser"
template <class Handle>
int32_t check_handle(ssym_ctx *ctx, const Handle *h, const char *noun, const char *fn)
{
    if (!h) {
        ctx->err = std::string(fn) + ": the " + noun + " handle is NULL";
        return SSYM_E_INVALID;
    }
    if (h->ctx != ctx) {
        ctx->err = std::string(fn) + ": the " + noun + " belongs to another context";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

// what is fed: a view of an object whose handle has been checked
struct LaneFeed {
    const char *noun;                                    // "spotter", "coverer", "mosaicker"
    const char *count;                                   // the name of the count output: "out_n_events", "out_n_pieces", "out_n_frames"
    uint32_t nLanes, dim;
    const std::vector<uint64_t> &consumed;               // frames per lane
    const std::vector<uint8_t> *ended;                   // NULL: lanes never end
    bool upload;                                         // false: the object has no use for the frames of a push
    std::function<int32_t(const char *fn)> own;          // the object's own check behind the NULL checks of push and follow

    // m frames more on a lane that has consumed n
    int32_t check_lane_room(ssym_ctx *ctx, const char *fn, uint32_t lane, uint64_t n, uint64_t m) const
    {
        if (m > kLaneMaxFrames || n + m > kLaneMaxFrames) {
            ctx->err = std::string(fn) + ": lane " + std::to_string(lane) + " would consume more than 2^31 - 1 = " +
                       std::to_string(kLaneMaxFrames) + " frames";
            return SSYM_E_UNSUPPORTED;
        }
        return SSYM_OK;
    }

    // lane l consumes the host frames feats[frame_offsets[l] ... frame_offsets[l + 1]): m[l] frames at rows[l], uploaded into a
    // block of bl (enqueued on ctx's stream; bl outlives the object's run)
    int32_t push(ssym_ctx *ctx, const char *fn, const double *feats, const uint64_t *frame_offsets, const uint64_t *out_n,
                 Blocks &bl, std::vector<const double *> &rows, std::vector<uint64_t> &m) const
    {
        if (!frame_offsets || !out_n) {
            ctx->err = std::string(fn) + ": frame_offsets and " + count + " must not be NULL";
            return SSYM_E_INVALID;
        }
        int32_t rc = own ? own(fn) : SSYM_OK;
        if (rc != SSYM_OK)
            return rc;
        m.assign(nLanes, 0);
        rows.assign(nLanes, nullptr);
        for (uint32_t l = 0; l < nLanes; ++l) {
            if (frame_offsets[l + 1] < frame_offsets[l]) {
                ctx->err = std::string(fn) + ": frame_offsets decrease";
                return SSYM_E_INVALID;
            }
            m[l] = frame_offsets[l + 1] - frame_offsets[l];
            if (m[l] && ended && (*ended)[l]) {
                ctx->err = std::string(fn) + ": lane " + std::to_string(l) + " was flushed and has ended; call ssym_" + noun + "_reset";
                return SSYM_E_INVALID;
            }
            rc = check_lane_room(ctx, fn, l, consumed[l], m[l]);
            if (rc != SSYM_OK)
                return rc;
        }
        const uint64_t total = frame_offsets[nLanes] - frame_offsets[0];
        if (total && !feats) {
            ctx->err = std::string(fn) + ": feats is NULL";
            return SSYM_E_INVALID;
        }
        SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        if (total && upload) {
            double *block = nullptr;
            rc = bl.get(&block, (size_t)total * dim);
            if (rc != SSYM_OK)
                return rc;
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(block, feats + frame_offsets[0] * dim, sizeof(double) * total * dim,
                                               hipMemcpyHostToDevice, ctx->stream));
            for (uint32_t l = 0; l < nLanes; ++l)
                rows[l] = block + (frame_offsets[l] - frame_offsets[0]) * dim;
        }
        return SSYM_OK;
    }

    // every lane consumes, in place, what the stream's lane holds beyond the frames consumed; a lane that has ended is skipped
    int32_t follow(ssym_ctx *ctx, const char *fn, const ssym_stream *stream, const uint64_t *out_n,
                   std::vector<const double *> &rows, std::vector<uint64_t> &m) const
    {
        if (!stream || !out_n) {
            ctx->err = std::string(fn) + ": stream and " + count + " must not be NULL";
            return SSYM_E_INVALID;
        }
        int32_t rc = own ? own(fn) : SSYM_OK;
        if (rc != SSYM_OK)
            return rc;
        uint32_t lanes = 0, nc = 0;
        const ssym_ctx *owner = nullptr;
        stream_shape(stream, &lanes, &nc, &owner);
        if (owner != ctx) {
            ctx->err = std::string(fn) + ": the stream belongs to another context";
            return SSYM_E_INVALID;
        }
        if (lanes != nLanes || nc != dim) {
            ctx->err = std::string(fn) + ": the stream has " + std::to_string(lanes) + " lanes of " + std::to_string(nc) +
                       " coefficients, the " + noun + " " + std::to_string(nLanes) + " lanes of " + std::to_string(dim) + " values";
            return SSYM_E_INVALID;
        }
        m.assign(nLanes, 0);
        rows.assign(nLanes, nullptr);
        for (uint32_t l = 0; l < nLanes; ++l) {
            const double *frames = nullptr;
            uint64_t held = 0;
            if (ssym_stream_frames_device(stream, l, &frames, &held) != SSYM_OK) {
                ctx->err = std::string(fn) + ": the stream does not answer for lane " + std::to_string(l);
                return SSYM_E_INVALID;
            }
            if (held < consumed[l]) {
                ctx->err = std::string(fn) + ": lane " + std::to_string(l) + " of the stream holds " + std::to_string(held) +
                           " frames, fewer than the " + std::to_string(consumed[l]) + " consumed: after ssym_stream_reset call ssym_" +
                           noun + "_reset";
                return SSYM_E_INVALID;
            }
            m[l] = ended && (*ended)[l] ? 0 : held - consumed[l];
            rc = check_lane_room(ctx, fn, l, consumed[l], m[l]);
            if (rc != SSYM_OK)
                return rc;
            rows[l] = m[l] ? frames + consumed[l] * dim : nullptr;           // read in place: no copy
        }
        SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        return SSYM_OK;
    }

    // the lane of a flush (wantCount: its count output too) or of a reset
    int32_t lane(ssym_ctx *ctx, const char *fn, uint32_t lane, bool wantCount, const uint64_t *out_n) const
    {
        if (lane >= nLanes || (wantCount && !out_n)) {
            ctx->err = std::string(fn) + ": lane outside the " + noun + "'s lanes";
            if (wantCount)
                ctx->err += std::string(", or ") + count + " is NULL";
            return SSYM_E_INVALID;
        }
        SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        return SSYM_OK;
    }
};

// The bodies of ssym_<noun>_push / _follow / _flush / _reset, from the extern "C" function's first line on: a NULL context
// is refused without a message and no exception leaves (guarded, ssym_internal.hpp); check_handle; the feed's checks; the
// object's part.
//   feed(ctx, h)                   : the object's LaneFeed (asked for once the handle is checked)
//   run(fn, rows, m, flushLane)    : consume m[l] frames at rows[l] (DEVICE) on every lane, then flush flushLane (kLaneNone:
//                                    none); whatever else the entry point takes rides in the callable
//   own()                          : reset's part of the object -- its init kernel and its mirrors of the lane

template <class Handle, class Body>
int32_t lane_entry(ssym_ctx *ctx, Handle *h, const char *noun, const char *fn, Body body)
{
    if (!ctx)
        return SSYM_E_INVALID;
    return guarded(ctx, [&]() -> int32_t {
        const int32_t rc = check_handle(ctx, h, noun, fn);
        return rc == SSYM_OK ? body() : rc;
    });
}

template <class Handle, class Feed, class Run>
int32_t lane_push(ssym_ctx *ctx, Handle *h, const char *noun, const char *fn, Feed feed, const double *feats,
                  const uint64_t *frame_offsets, const uint64_t *out_n, Run run)
{
    return lane_entry(ctx, h, noun, fn, [&]() -> int32_t {
        Blocks bl(ctx);                                  // the uploaded frames: they outlive the run
        std::vector<const double *> rows;
        std::vector<uint64_t> m;
        const int32_t rc = feed(ctx, h).push(ctx, fn, feats, frame_offsets, out_n, bl, rows, m);
        return rc == SSYM_OK ? run(fn, rows, m, kLaneNone) : rc;
    });
}

template <class Handle, class Feed, class Run>
int32_t lane_follow(ssym_ctx *ctx, Handle *h, const char *noun, const char *fn, Feed feed, const ssym_stream *stream,
                    const uint64_t *out_n, Run run)
{
    return lane_entry(ctx, h, noun, fn, [&]() -> int32_t {
        std::vector<const double *> rows;
        std::vector<uint64_t> m;
        const int32_t rc = feed(ctx, h).follow(ctx, fn, stream, out_n, rows, m);
        return rc == SSYM_OK ? run(fn, rows, m, kLaneNone) : rc;
    });
}

template <class Handle, class Feed, class Run>
int32_t lane_flush(ssym_ctx *ctx, Handle *h, const char *noun, const char *fn, Feed feed, uint32_t lane, const uint64_t *out_n,
                   Run run)
{
    return lane_entry(ctx, h, noun, fn, [&]() -> int32_t {
        const int32_t rc = feed(ctx, h).lane(ctx, fn, lane, true, out_n);
        if (rc != SSYM_OK)
            return rc;
        const std::vector<const double *> rows(h->nLanes, nullptr);
        const std::vector<uint64_t> m(h->nLanes, 0);
        return run(fn, rows, m, lane);
    });
}

template <class Handle, class Feed, class Own>
int32_t lane_reset(ssym_ctx *ctx, Handle *h, const char *noun, const char *fn, Feed feed, uint32_t lane, Own own)
{
    return lane_entry(ctx, h, noun, fn, [&]() -> int32_t {
        const int32_t rc = feed(ctx, h).lane(ctx, fn, lane, false, nullptr);
        return rc == SSYM_OK ? own() : rc;
    });
}

// ssym_<noun>_destroy: NULL is destroyed already; the stream has done with the object's memory before release(ctx, h) frees it
template <class Handle, class Release>
int32_t lane_destroy(ssym_ctx *ctx, Handle *h, Release release)
{
    if (!h)
        return SSYM_OK;
    if (!ctx || h->ctx != ctx)
        return SSYM_E_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    release(ctx, h);
    return SSYM_OK;
}

}  // namespace ssym
