// filter_plan_dump -- prints what plan_filter (soundsym_amd/csrc/dtw_filter_plan.hpp) plans, for tests/test_filter_plan.py to
// hold against tests/filter_plan.py.  A host program over that one header: no HIP, no library.
//
//   filter_plan_dump CASES > plans.jsonl
//
// CASES, one record per line:
//   set NSRC len... NTGT len...                    segment lengths, in any order
//   run ID DIM CUS ABANDON SWEPT  PK SP MULTIPAIR PAIRBLOCK WG SKIP0 NT8 ONE_LAUNCH LONG_CLASSES PRUNE_NT
//                                                   one filter call over the last set: the FilterKnobs fields in their order
// Output: first the constants, then per run {"id": ID, "launches": [every field of every FilterLaunch]}.
#include "dtw_filter_plan.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

using namespace ssym;

static const char *kind_name(FilterKernel k)
{
    switch (k) {
    case FilterKernel::Mp: return "Mp";
    case FilterKernel::Sp: return "Sp";
    case FilterKernel::Generic: return "Generic";
    case FilterKernel::GenericSkip0: return "GenericSkip0";
    case FilterKernel::GenericPrune: return "GenericPrune";
    case FilterKernel::Wg: return "Wg";
    case FilterKernel::Pk: return "Pk";
    }
    return "?";
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: filter_plan_dump CASES\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    if (!f) {
        std::fprintf(stderr, "filter_plan_dump: cannot read %s\n", argv[1]);
        return 2;
    }
    std::printf("{\"kMaxClasses\": %d, \"kSmallClass\": %d, \"kSpRowBlock\": %d, \"kSpRing\": %d, \"kFilterRecHalfs\": %d, "
                "\"kFilterWavesPerBlock\": %d, \"kFilterMaxFrames\": %d, \"SSYM_SP_OCC_NT2\": %d}\n",
                kMaxClasses, kSmallClass, kSpRowBlock, kSpRing, kFilterRecHalfs, kFilterWavesPerBlock, kFilterMaxFrames,
                SSYM_SP_OCC_NT2);
    std::vector<uint32_t> ls, lt;       // the last set's lengths, ascending: record slots are ordered by length
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what))
            continue;
        if (what == "set") {
            size_t n = 0, m = 0;
            in >> n;
            ls.assign(n, 0u);
            for (uint32_t &x : ls)
                in >> x;
            in >> m;
            lt.assign(m, 0u);
            for (uint32_t &x : lt)
                in >> x;
            if (!in || n == 0 || m == 0) {
                std::fprintf(stderr, "filter_plan_dump: bad set: %.60s\n", line.c_str());
                return 1;
            }
            std::sort(ls.begin(), ls.end());
            std::sort(lt.begin(), lt.end());
            continue;
        }
        std::string id;
        int dim = 0, abandon = 0, k[10] = {0};
        FilterPlanInput p;
        in >> id >> dim >> p.numCus >> abandon >> p.pruneSwept;
        for (int &x : k)
            in >> x;
        if (what != "run" || !in || ls.empty()) {
            std::fprintf(stderr, "filter_plan_dump: bad run: %.60s\n", line.c_str());
            return 1;
        }
        p.knobs.pk = k[0], p.knobs.sp = k[1], p.knobs.spMultipair = k[2], p.knobs.spPairBlock = k[3], p.knobs.wg = k[4];
        p.knobs.skip0 = k[5], p.knobs.nt8 = k[6], p.knobs.oneLaunch = k[7], p.knobs.longClasses = k[8], p.knobs.pruneNt = k[9];
        p.abandon = abandon != 0;
        const FilterShape shape = filter_shape((int)std::max<uint32_t>(ls.back(), 1u));
        if (shape.nt == 0) {
            std::printf("{\"id\": \"%s\", \"launches\": null}\n", id.c_str());       // beyond the filter's reach
            continue;
        }
        // the sets as pack pads them: sources and targets to multiples of 32 slots, rows to the set's shape
        p.srcN = (uint32_t)ls.size(), p.srcNPad = (p.srcN + 31) / 32 * 32, p.framesPad = (uint32_t)shape.rows();
        p.tgtN = (uint32_t)lt.size();
        std::vector<uint32_t> pairLen(p.srcNPad / 2, 0u), groupCols((p.tgtN + 31) / 32, 0u);
        for (uint32_t s = 0; s < p.srcN; ++s)
            pairLen[s / 2] = std::max(pairLen[s / 2], ls[s]);
        for (uint32_t t = 0; t < p.tgtN; ++t) {
            groupCols[t / 32] = std::max(groupCols[t / 32], lt[t]);
            p.tgtTotalFrames += lt[t];
        }
        p.pairLen = pairLen.data(), p.groupCols = groupCols.data(), p.tgtGroups = (uint32_t)groupCols.size();
        // operand planes: the default record layouts (filter_pieces: layout 3 up to 13 values, layout 1 beyond)
        const int dimUse = filter_dim_used(dim);
        p.ku = filter_mfmas(dimUse > 13 ? 1 : 3, dimUse);
        std::printf("{\"id\": \"%s\", \"launches\": [", id.c_str());
        const std::vector<FilterLaunch> plan = plan_filter(p);
        for (size_t i = 0; i < plan.size(); ++i) {
            const FilterLaunch &l = plan[i];
            std::printf("%s{\"kind\": \"%s\", \"nt\": %d, \"passes\": %d, \"origin\": %d, \"lo\": %d, \"hi\": %d, \"grid\": %d, "
                        "\"taskChunk\": %d, \"pairBlock\": %d, \"taskPairs\": %d, \"occ\": %d, \"ctrSet\": %d, \"cells\": %llu}",
                        i ? ", " : "", kind_name(l.kind), l.nt, l.passes, l.origin, l.lo, l.hi, l.grid, l.taskChunk, l.pairBlock,
                        l.taskPairs, l.occ, l.ctrSet, l.cells);
        }
        std::printf("]}\n");
    }
    return 0;
}
