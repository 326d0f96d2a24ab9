// lane_tiling.hpp -- the host side of the two live tilings: the coverer (dtw_coverer.hip) and the mosaicker
// (dtw_mosaicker.hip) tile growing targets from one resident dictionary and report, call by call, what has become final.
// What they hold under the same names is LaneTiling; against it there is one of each of: the dictionary check and the feed
// (check_dict, feed_of), the first refusals of create (tiling_create_checks), the host body of best (tiling_best), the loop
// of push / follow / flush (tiling_run) and the hand-over of a grown ring store (ring_swap).  The kernels, the lane and step
// records and the plan of a slice are each object's own.
#pragma once

#include "dtw_wave.hpp"
#include "lane_feed.hpp"

namespace ssym {

struct LaneTiling {
    ssym_ctx *ctx = nullptr;
    const ssym_dict *dict = nullptr;
    uint32_t nLanes = 0, dim = 0;
    uint32_t dictN = 0;                      // the dictionary as it was at creation
    uint64_t dictFrames = 0;
    double penalty = 0.0, gapCost = 0.0;     // gapCost +inf: no gaps
    // host mirrors of the lanes
    std::vector<uint64_t> consumed;
    std::vector<int64_t> done;               // the last committed frame, -1 at first
    std::vector<uint8_t> ended;
    LaneLog log;                             // what the last push / follow / flush emitted
    uint64_t calls = 0;                      // push / follow / flush calls that began a log (host only): names a log to its reader

    explicit LaneTiling(uint32_t logWords) : log(logWords) {}

    void bind(ssym_ctx *c, const ssym_dict *d, uint32_t n_lanes, double piece_penalty, double gap_cost)
    {
        ctx = c;
        dict = d;
        nLanes = n_lanes;
        dim = d->set.dim;
        dictN = d->set.n;
        dictFrames = d->set.total_frames;
        penalty = piece_penalty;
        gapCost = gap_cost;
        consumed.assign(n_lanes, 0);
        done.assign(n_lanes, -1);
        ended.assign(n_lanes, 0);
    }
};

// what a call that reads the dictionary refuses
inline int32_t check_dict(ssym_ctx *ctx, const LaneTiling *t, const char *noun, const char *fn)
{
    if (t->dict->set.n != t->dictN || t->dict->set.total_frames != t->dictFrames) {
        ctx->err = std::string(fn) + ": the dictionary was appended to after the " + noun + " was created; create a new " + noun;
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

// a tiling as the lane feed (lane_feed.hpp) sees it: a flushed lane has ended, and push and follow read the dictionary
inline LaneFeed feed_of(ssym_ctx *ctx, const LaneTiling *t, const char *noun, const char *count)
{
    return LaneFeed{noun, count, t->nLanes, t->dim, t->consumed, &t->ended, true,
                    [ctx, t, noun](const char *fn) { return check_dict(ctx, t, noun, fn); }};
}

// what ssym_coverer_create* and ssym_mosaicker_create refuse first, in this order; *out is NULL from here on
template <class Handle>
int32_t tiling_create_checks(ssym_ctx *ctx, const char *fn, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty,
                             double gap_cost, Handle **out)
{
    if (!out) {
        ctx->err = std::string(fn) + ": out is NULL";
        return SSYM_E_INVALID;
    }
    *out = nullptr;
    int32_t rc = check_cover_ctx(ctx, fn);
    if (rc != SSYM_OK)
        return rc;
    if (!dict || n_lanes == 0) {
        ctx->err = std::string(fn) + ": the dictionary handle is NULL or n_lanes is 0";
        return SSYM_E_INVALID;
    }
    rc = check_cover_prices(ctx, fn, piece_penalty, gap_cost);
    if (rc != SSYM_OK)
        return rc;
    if (dict->set.n == 0) {
        ctx->err = std::string(fn) + ": empty dictionary";
        return SSYM_E_EMPTY_DICT;
    }
    return SSYM_OK;
}

// ssym_<noun>_best: launch(total, covered, committed) starts the object's best kernel on arrays of nLanes (NULL: not asked for)
template <class Launch>
int32_t tiling_best(ssym_ctx *ctx, const LaneTiling *t, const char *noun, const char *fn, double *out_total, uint32_t *out_covered,
                    uint32_t *out_committed, uint32_t flags, Launch launch)
{
    int32_t rc = check_handle(ctx, t, noun, fn);
    if (rc != SSYM_OK)
        return rc;
    if (!out_total && !out_covered && !out_committed)
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t nL = t->nLanes;
    // the caller's device arrays in place, or one f64 and one u32 block copied back
    StagedOut out(flags, {{out_total, nL}}, {{out_covered, nL}, {out_committed, nL}});
    Blocks bl(ctx);
    rc = out.alloc(bl);
    if (rc != SSYM_OK)
        return rc;
    launch(out.f64[0], out.u32[0], out.u32[1]);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return out.finish(ctx);
}

// A ring store grows.  fresh: the new arrays, allocated by the object one after the other until one failed (`allocated`
// says how; the rest are NULL); old: the arrays they replace (`had`: there are some); regrow(): launches the kernel that
// moves what the old arrays still hold; adopt(): the object's slots take the fresh arrays.  All or nothing: on any failure
// the fresh arrays are freed and the slots stay; else the stream has done with the old arrays before they are freed, and
// the slots change hands last.
template <size_t N, class Regrow, class Adopt>
int32_t ring_swap(ssym_ctx *ctx, const char *noun, int32_t allocated, void *const (&old)[N], void *const (&fresh)[N], bool had,
                  Regrow regrow, Adopt adopt)
{
    hipError_t e = hipSuccess;
    if (allocated == SSYM_OK && had) {
        regrow();
        e = hipGetLastError();
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);
        e = e != hipSuccess ? e : e2;
    }
    if (allocated != SSYM_OK || e != hipSuccess) {
        for (void *p : fresh)
            if (p)
                dev_free(ctx, p);
        if (allocated != SSYM_OK)
            return allocated;
        ctx->err = std::string(noun) + ": " + hipGetErrorString(e);
        return SSYM_E_HIP;
    }
    if (had)
        for (void *p : old)
            dev_free(ctx, p);
    adopt();
    return SSYM_OK;
}

// a call of tiling_run as the plan of a slice sees it: the frames and how many of them each lane has taken
struct TilingCall {
    const char *fn;
    const std::vector<const double *> &rows;
    const std::vector<uint64_t> &m;
    uint32_t flushLane;
    std::vector<uint64_t> at;
};

// the fields every step record has, for a slice of at most `slice` frames per lane; gives the lane's frames in it
template <class Step>
uint64_t tiling_step(const LaneTiling *t, const TilingCall &c, uint32_t l, uint64_t slice, Step *s)
{
    const uint64_t ml = std::min(slice, c.m[l] - c.at[l]);
    s->rows = ml ? c.rows[l] + c.at[l] * t->dim : nullptr;
    s->logAt = t->log.off[l] + t->log.count[l];
    s->m = (uint32_t)ml;
    s->flush = l == c.flushLane;
    return ml;
}

// something more that goes up with every slice's steps (the coverer's bufOff)
struct Upload {
    void *dev = nullptr;
    const void *host = nullptr;
    size_t bytes = 0;
};

// The body of push, follow and flush.  rows[l]: lane l's m[l] new frames (DEVICE); flushLane: the lane to flush, or
// kLaneNone.  The frames go through in slices with a commit after each; the host reads the lanes' records back after every
// slice, which is also the slice's synchronisation.  cells: cells per frame, for the timings.  The object `o` gives
//   plan(call, steps, &left, &need) : the next slice -- the step records (DEVICE copy: dSteps), the frames in it, the ring
//                                     room it needs; it may refuse
//   grow(need)                      : that room
//   forward(left != 0)              : what ev[0] ... ev[1] times (main_ms)
//   commit(left != 0)               : what ev[1] ... ev[2] times (reduce_ms)
//   fold(l, lane)                   : its own mirrors of lane l from the lane's record (DEVICE: dLanes)
// A refusal or failure inside a slice leaves through the epilogue: the count output says what the earlier slices logged (the
// mirrors and the log stand at the last slice that ran whole), the timings are stored, and a flushed lane has not ended.
template <class Step, class Lane, class Obj>
int32_t tiling_run(ssym_ctx *ctx, LaneTiling *t, Obj &o, Step *dSteps, const Lane *dLanes, uint64_t cells, const char *fn,
                   const std::vector<const double *> &rows, const std::vector<uint64_t> &m, uint32_t flushLane, uint64_t *out_n,
                   Upload more = {})
{
    const uint32_t nL = t->nLanes;
    hipStream_t st = ctx->stream;
    hipEvent_t *ev = ctx->ev;
    ssym_timings tm{};
    int32_t rc = t->log.begin(ctx, t->consumed, t->done, m, flushLane);
    if (rc != SSYM_OK)
        return rc;
    ++t->calls;
    for (uint32_t l = 0; l < nL; ++l)
        tm.n_pairs += cells * m[l];
    TilingCall call{fn, rows, m, flushLane, std::vector<uint64_t>(nL, 0)};
    std::vector<Step> steps(nL);
    std::vector<Lane> state(nL);
    const bool flush = flushLane != kLaneNone;
    for (;;) {
        uint64_t left = 0, need = 0;
        rc = o.plan(call, steps, &left, &need);
        if (rc != SSYM_OK || (left == 0 && !flush))
            break;
        rc = [&]() -> int32_t {
            int32_t r = o.grow(need);
            if (r != SSYM_OK)
                return r;
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dSteps, steps.data(), sizeof(Step) * nL, hipMemcpyHostToDevice, st));
            if (more.bytes)
                SSYM_HIP_CHECK(ctx, hipMemcpyAsync(more.dev, more.host, more.bytes, hipMemcpyHostToDevice, st));
            SSYM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
            r = o.forward(left != 0);
            if (r != SSYM_OK)
                return r;
            SSYM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
            r = o.commit(left != 0);
            if (r != SSYM_OK)
                return r;
            SSYM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(state.data(), dLanes, sizeof(Lane) * nL, hipMemcpyDeviceToHost, st));
            SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
            return SSYM_OK;
        }();
        if (rc != SSYM_OK)
            break;
        for (uint32_t l = 0; l < nL; ++l) {
            if (steps[l].m == 0 && !steps[l].flush)
                continue;
            t->consumed[l] = (uint64_t)state[l].n;
            t->done[l] = state[l].done;
            t->log.count[l] += state[l].count;
            call.at[l] += steps[l].m;
            o.fold(l, state[l]);
        }
        tm.main_ms += ev_ms(ev[0], ev[1]);
        tm.reduce_ms += ev_ms(ev[1], ev[2]);
        tm.total_ms += ev_ms(ev[0], ev[2]);
        tm.main_launches += left ? 1 : 0;
        if (flush)
            break;
    }
    if (flush && rc == SSYM_OK)
        t->ended[flushLane] = 1;
    *out_n = t->log.total();
    ctx->timings = tm;
    return rc;
}

}  // namespace ssym
