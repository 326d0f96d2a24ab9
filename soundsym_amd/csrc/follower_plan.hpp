// follower_plan.hpp -- the plan of one call of the live envelope follower (follower.hip; DESIGN.md 2 "Live envelope
// following", 5.29): what a push or a flush consumes, settles and releases, lane by lane.
//
// Host only, standard library only: follower.hip runs the plan, tests/cpp/follower_plan_dump.cpp prints it for the CPU
// tests, which hold it against its restatement in tests/live_follow_ref.py.  Everything here is arithmetic on how much the
// lanes have consumed -- never on a sample's value, never on how the samples were cut into pushes: with
// h = floor(min(ny, nx) / HOP), before the flush boundary b is settled when (b + 2) HOP <= min(ny, nx), max(0, h - 1) of
// them, and hop j is released when boundaries j and j + 1 are settled, max(0, h - 2) of them; the flush settles every
// boundary up to J = ceil(ny / HOP) and releases the rest of y.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ssym {

constexpr uint64_t kFollowerHop = 256;                   // HOP
constexpr uint64_t kFollowerLook = 2;                    // hops of look-ahead behind a boundary
constexpr uint32_t kFollowerBlock = 32;                  // boundaries per entry of the block table
constexpr uint64_t kFollowerRingMin = 2048;              // samples per lane and signal, at least
constexpr uint64_t kFollowerRingBytes = 512ull << 20;    // both rings of an object, at most
constexpr uint32_t kFollowerMaxLanes = (uint32_t)(kFollowerRingBytes / (2 * sizeof(double) * kFollowerRingMin));      // 16 384
constexpr uint64_t kFollowerMaxLen = 1ull << 40;         // a lane consumes fewer samples per signal
constexpr uint32_t kFollowerNoLane = 0xffffffffu;
static_assert(kFollowerMaxLanes == 16384, "the rings of the most lanes at the least capacity fill the budget");

// a lane since its reset
struct FollowerLane {
    uint64_t ny = 0, nx = 0;     // samples of y and of x consumed
    uint64_t released = 0;       // samples of y released
    uint8_t ended = 0;           // flushed
};

// boundaries settled and hops released before the flush, from the counts alone
inline uint64_t follower_settled(uint64_t ny, uint64_t nx)
{
    const uint64_t h = std::min(ny, nx) / kFollowerHop;
    return h > 1 ? h - 1 : 0;
}
inline uint64_t follower_released_hops(uint64_t ny, uint64_t nx)
{
    const uint64_t h = std::min(ny, nx) / kFollowerHop;
    return h > 2 ? h - 2 : 0;
}
// boundaries of a lane that ends with n samples
inline uint64_t follower_boundaries(uint64_t n) { return n ? (n + kFollowerHop - 1) / kFollowerHop + 1 : 0; }
// the first sample a lane still holds: two hops below the first unreleased one
inline uint64_t follower_held_from(const FollowerLane &l)
{
    const uint64_t r = l.released / kFollowerHop;
    return (r > kFollowerLook ? r - kFollowerLook : 0) * kFollowerHop;
}

// what one call does with a lane (the device reads it as it stands: 8-byte fields only)
struct FollowerStep {
    uint64_t ny, nx;             // the counts after the call
    uint64_t my, mx;             // samples appended
    uint64_t yAt, xAt;           // where they start in the call's arrays
    uint64_t setFirst, setCount; // the boundaries the call settles
    uint64_t relFirst, relCount; // the samples the call releases
    uint64_t outAt, gainAt;      // the lane's stretch of the call's sample log and gain log
};

// an entry of the gain kernel's block table
struct FollowerBlockEntry {
    uint32_t lane, first, count, pad;
};

struct FollowerPlan {
    std::vector<FollowerStep> steps;         // [nLanes]
    std::vector<FollowerBlockEntry> table;
    uint64_t samples = 0, gains = 0;         // the call's totals: released samples, settled boundaries
    uint64_t maxAppend = 0;                  // the most samples one lane appends to one ring
    uint64_t maxReleased = 0;                // the most samples one lane releases
    uint32_t maxBlock = 0;                   // the largest count in the table
    uint64_t ringCap = kFollowerRingMin;     // the capacity the rings need: a power of two
    bool work = false;                       // a lane appends, settles or releases
};

inline uint64_t follower_pow2_at_least(uint64_t x)
{
    uint64_t p = 1;
    while (p < x)
        p <<= 1;
    return p;
}

// The plan of a push (yOff / xOff: [nLanes + 1] offsets into the call's arrays, checked by the caller; flushLane =
// kFollowerNoLane) or of a flush (yOff = xOff = NULL).  Lanes that have ended take no part.
inline FollowerPlan follower_plan(const std::vector<FollowerLane> &lanes, const uint64_t *yOff, const uint64_t *xOff, uint32_t flushLane)
{
    FollowerPlan p;
    const uint32_t nL = (uint32_t)lanes.size();
    p.steps.assign(nL, FollowerStep{});
    uint64_t held = 0;
    for (uint32_t l = 0; l < nL; ++l) {
        const FollowerLane &ln = lanes[l];
        FollowerStep &s = p.steps[l];
        s.my = yOff ? yOff[l + 1] - yOff[l] : 0;
        s.mx = xOff ? xOff[l + 1] - xOff[l] : 0;
        s.yAt = yOff ? yOff[l] : 0;
        s.xAt = xOff ? xOff[l] : 0;
        s.ny = ln.ny + s.my;
        s.nx = ln.nx + s.mx;
        s.outAt = p.samples;
        s.gainAt = p.gains;
        if (ln.ended) {
            s.setFirst = follower_boundaries(ln.ny);
            s.relFirst = ln.released;
            continue;
        }
        s.setFirst = follower_settled(ln.ny, ln.nx);
        s.relFirst = ln.released;
        uint64_t setEnd = follower_settled(s.ny, s.nx), relEnd = follower_released_hops(s.ny, s.nx) * kFollowerHop;
        if (l == flushLane) {
            setEnd = follower_boundaries(s.ny);
            relEnd = s.ny;
        }
        s.setCount = setEnd - s.setFirst;
        s.relCount = relEnd - s.relFirst;
        for (uint64_t b = 0; b < s.setCount; b += kFollowerBlock) {
            const uint32_t count = (uint32_t)std::min<uint64_t>(kFollowerBlock, s.setCount - b);
            p.table.push_back(FollowerBlockEntry{l, (uint32_t)(s.setFirst + b), count, 0});
            p.maxBlock = std::max(p.maxBlock, count);
        }
        p.samples += s.relCount;
        p.gains += s.setCount;
        p.maxAppend = std::max(p.maxAppend, std::max(s.my, s.mx));
        p.maxReleased = std::max(p.maxReleased, s.relCount);
        p.work = p.work || s.my || s.mx || s.setCount || s.relCount;
        // the ring holds the lane from two hops below its first unreleased hop up to everything consumed
        held = std::max(held, std::max(s.ny, s.nx) - follower_held_from(ln));
    }
    p.ringCap = follower_pow2_at_least(std::max(held, kFollowerRingMin));
    return p;
}

// do rings of this capacity stay within the object's budget?
inline bool follower_ring_fits(uint64_t cap, uint32_t nLanes)
{
    return cap <= kFollowerRingBytes / (2 * sizeof(double)) / nLanes;
}

// the lanes after the call
inline void follower_commit(std::vector<FollowerLane> &lanes, const FollowerPlan &p, uint32_t flushLane)
{
    for (size_t l = 0; l < lanes.size(); ++l) {
        if (lanes[l].ended)
            continue;
        lanes[l].ny = p.steps[l].ny;
        lanes[l].nx = p.steps[l].nx;
        lanes[l].released = p.steps[l].relFirst + p.steps[l].relCount;
    }
    if (flushLane != kFollowerNoLane)
        lanes[flushLane].ended = 1;
}

}  // namespace ssym
