// The plan of the live envelope follower's calls (soundsym_amd/csrc/follower_plan.hpp), printed for tests/test_follower_plan.py:
// a host program over the plan's header alone, no HIP and no library.
//
//   follower_plan_dump <cases>      the file holds one call per line:
//     call <id> <lanes> <flush lane, or -1 for a push> then per lane: <ny> <nx> <released> <ended> <my> <mx>
// Output: a line of constants, then one JSON object per call.
#include "follower_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

using namespace ssym;

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <cases>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::printf("{\"kFollowerHop\": %" PRIu64 ", \"kFollowerBlock\": %u, \"kFollowerRingMin\": %" PRIu64 ", \"kFollowerRingBytes\": %" PRIu64
                ", \"kFollowerMaxLanes\": %u, \"kFollowerMaxLen\": %" PRIu64 ", \"kFollowerNoLane\": %u}\n",
                kFollowerHop, kFollowerBlock, kFollowerRingMin, kFollowerRingBytes, kFollowerMaxLanes, kFollowerMaxLen, kFollowerNoLane);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string word, id;
        uint32_t nL = 0;
        long long flush = -1;
        if (!(ss >> word >> id >> nL >> flush) || word != "call" || nL == 0) {
            std::fprintf(stderr, "bad line: %s\n", line.c_str());
            return 2;
        }
        std::vector<FollowerLane> lanes(nL);
        std::vector<uint64_t> yOff(nL + 1, 0), xOff(nL + 1, 0);
        for (uint32_t l = 0; l < nL; ++l) {
            uint64_t my = 0, mx = 0;
            unsigned ended = 0;
            if (!(ss >> lanes[l].ny >> lanes[l].nx >> lanes[l].released >> ended >> my >> mx)) {
                std::fprintf(stderr, "bad lane %u: %s\n", l, line.c_str());
                return 2;
            }
            lanes[l].ended = (uint8_t)ended;
            yOff[l + 1] = yOff[l] + my;
            xOff[l + 1] = xOff[l] + mx;
        }
        const uint32_t flushLane = flush < 0 ? kFollowerNoLane : (uint32_t)flush;
        const bool push = flush < 0;
        const FollowerPlan p = follower_plan(lanes, push ? yOff.data() : nullptr, push ? xOff.data() : nullptr, flushLane);
        std::printf("{\"id\": \"%s\", \"steps\": [", id.c_str());
        for (uint32_t l = 0; l < nL; ++l) {
            const FollowerStep &s = p.steps[l];
            std::printf("%s{\"ny\": %" PRIu64 ", \"nx\": %" PRIu64 ", \"my\": %" PRIu64 ", \"mx\": %" PRIu64 ", \"yAt\": %" PRIu64 ", \"xAt\": %" PRIu64
                        ", \"setFirst\": %" PRIu64 ", \"setCount\": %" PRIu64 ", \"relFirst\": %" PRIu64 ", \"relCount\": %" PRIu64
                        ", \"outAt\": %" PRIu64 ", \"gainAt\": %" PRIu64 "}",
                        l ? ", " : "", s.ny, s.nx, s.my, s.mx, s.yAt, s.xAt, s.setFirst, s.setCount, s.relFirst, s.relCount, s.outAt, s.gainAt);
        }
        std::printf("], \"table\": [");
        for (size_t i = 0; i < p.table.size(); ++i)
            std::printf("%s[%u, %u, %u]", i ? ", " : "", p.table[i].lane, p.table[i].first, p.table[i].count);
        std::printf("], \"samples\": %" PRIu64 ", \"gains\": %" PRIu64 ", \"maxAppend\": %" PRIu64 ", \"maxReleased\": %" PRIu64
                    ", \"maxBlock\": %u, \"ringCap\": %" PRIu64 ", \"fits\": %s, \"after\": [",
                    p.samples, p.gains, p.maxAppend, p.maxReleased, p.maxBlock, p.ringCap, follower_ring_fits(p.ringCap, nL) ? "true" : "false");
        follower_commit(lanes, p, flushLane);
        for (uint32_t l = 0; l < nL; ++l)
            std::printf("%s[%" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %u]", l ? ", " : "", lanes[l].ny, lanes[l].nx, lanes[l].released,
                        (unsigned)lanes[l].ended);
        std::printf("]}\n");
    }
    return 0;
}
