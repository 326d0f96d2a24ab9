// dtw_filter.hip -- all-pairs DTW cost fill on the f16 matrix pipe (gfx950), one pair per lane.
//
// Role on the path: replaces the N x M evaluations of the reference's inner loop
// (SoundDictionary::at_distance, src/sound.rs:352-359, called once per target by
// clone_from_dictionary, src/sound.rs:453-454) for the dtw metric.  Output is the f32 cost of every
// (source, target) pair; select.hip picks candidates from it and dtw_exact.hip re-scores them.
// The kernels are in dtw_filter_kernel.hpp and its siblings; this file builds their operand records and runs the launches
// that plan_filter (dtw_filter_plan.hpp) plans from the segment lengths.
//
// Numerics: operands are scaled by a common power of two s so that max |s v| < 64 and split into f16
// pieces (three record layouts, filter_pieces() in ssym_internal.hpp: up to 13 values per frame the
// source in two pieces and the target in one, K = 32; wider frames one piece on both sides, K = 48);
// the squared norms of the REPRESENTED frames ride along in two or three pieces, products are exact in
// the f32 accumulator.  The filter's error bound is derived in select.hip; returned costs and indices
// always come from the exact f64 kernel.
#include "ssym_internal.hpp"
#include "dtw_filter_kernel.hpp"
#include "dtw_filter_wg_kernel.hpp"
#include "dtw_filter_wg2_kernel.hpp"
#include "dtw_filter_pk_kernel.hpp"
#include "dtw_filter_sp_kernel.hpp"
#include "dtw_band_kernel.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

namespace ssym {

// launches of dtw_filter_wg_kernel in this process (run_kernel; read by ssym_debug_filter_wg_launches below: the tests'
// proof of which kernel ran)
static std::atomic<unsigned long long> g_filter_wg_launches{0};
// ... and those of them that took dtw_filter_wg2_kernel, the two-pass sibling (ssym_debug_filter_wg2_launches)
static std::atomic<unsigned long long> g_filter_wg2_launches{0};
// SSYM_FILTER_WG2=0 (under SSYM_TEST_HOOKS, read per filter call by read_filter_knobs): two-pass launches of the plan's Wg
// kind stay on dtw_filter_wg_kernel -- A/B runs from one library.  Not a knob of the plan: the plan is the same either way.
static std::atomic<bool> g_filter_wg2{true};
// ... and those of the wg2 launches that took its uniform-length instantiation (ssym_debug_filter_wg2u_launches)
static std::atomic<unsigned long long> g_filter_wg2u_launches{0};
// SSYM_FILTER_WG2U=0 (under SSYM_TEST_HOOKS, read beside SSYM_FILTER_WG2): uniform sets keep the general wg2 kernel
static std::atomic<bool> g_filter_wg2u{true};

int filter_pieces(int dim)
{
    static const bool k48 = ssym_knob("SSYM_FILTER_K48") != nullptr;      // measurements: the symmetric K = 48 layout
    return dim > kFilterMaxDim2 ? 1 : (k48 ? 2 : 3);
}

// One thread per (segment, record slot).  Frame f of a segment with nf frames goes to slot
// lead + f (lead = -1: END-ALIGNED, slot frames_pad - nf + f, the unbanded kernel's source layout).
// Source slots that hold no frame (and all slots of padding segments) get |a|^2 = +inf so that
// their DP cells stay at +inf; empty target slots are all-zero records.
__global__ void build_filter_records_kernel(const double *__restrict__ raw, const uint64_t *__restrict__ off,
                                            const uint32_t *__restrict__ perm, uint32_t n, uint32_t dim,
                                            uint32_t dimUse, uint32_t frames_pad, int is_source,
                                            int lead, int pieces, double scale, _Float16 *__restrict__ rec,
                                            unsigned *__restrict__ resid)
{
    const uint32_t s = blockIdx.y;                              // record slot of the segment, < n_pad
    const uint32_t seg = perm[s];                               // the segment it holds (0xffffffff: none)
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= frames_pad)
        return;
    _Float16 out[kFilterRecHalfs];
#pragma unroll
    for (int i = 0; i < kFilterRecHalfs; ++i)
        out[i] = (_Float16)0.0f;
    const uint32_t nf = seg < n ? (uint32_t)(off[seg + 1] - off[seg]) : 0u;
    const uint32_t first = lead < 0 ? frames_pad - nf : (uint32_t)lead;
    const bool real = slot >= first && slot < first + nf;
    const uint32_t f = slot - first;
    // slot of the first |a|^2 piece: behind the product slots (layout 3: fixed at 28, K = 32)
    const int nbase = pieces == 3 ? 28 : (pieces == 2 ? 3 : 1) * (int)dimUse;
    const int npieces = pieces == 3 ? 2 : 3;                       // f16 pieces per squared norm
    if (!real && is_source)
        out[filter_slot_offset(nbase)] = (_Float16)__builtin_inff();   // |a|^2 = +inf
    if (real) {
        const double *p = raw + (off[seg] + f) * dim;
        double nrm = 0.0, res2 = 0.0;
        for (uint32_t e = 0; e < dimUse; ++e) {                  // frames wider than 42 values: the first 42
            const double v = p[e] * scale;                       // exact: scale is a power of two
            const _Float16 h1 = (_Float16)v;
            // second piece: both sides in layout 2; in layout 3 the source, and the target's first two values
            const bool two = pieces == 2 || (pieces == 3 && (is_source || e < 2));
            const _Float16 h2 = two ? (_Float16)(v - (double)h1) : (_Float16)0.0f;
            const double vh = (double)h1 + (double)h2;           // the value the MFMA will see
            nrm += vh * vh;                                      // norms of the REPRESENTED frame
            res2 += (v - vh) * (v - vh);                         // ... and how far it lies from the frame itself
            const _Float16 m1 = (_Float16)(-2.0f * (float)h1), m2 = (_Float16)(-2.0f * (float)h2);
            if (pieces == 2) {
                out[filter_slot_offset(3 * e + 0)] = is_source ? m1 : h1;
                out[filter_slot_offset(3 * e + 1)] = is_source ? m1 : h2;
                out[filter_slot_offset(3 * e + 2)] = is_source ? m2 : h1;
            } else if (pieces == 3) {
                // a . b~ = (a1 + a2) b1 for every value, + a1 b2 for the first two: b~ = b1 (+ b2), exactly the
                // frame whose norm rides along, so the accumulator is |a~ - b~|^2 with no cancellation error
                out[filter_slot_offset(2 * e + 0)] = is_source ? m1 : h1;
                out[filter_slot_offset(2 * e + 1)] = is_source ? m2 : h1;
                if (e < 2)
                    out[filter_slot_offset(26 + e)] = is_source ? m1 : h2;
            } else {
                out[filter_slot_offset(e)] = is_source ? m1 : h1;
            }
        }
        // |frame - represented frame|, unscaled, rounded up: a local cost of this frame moves by at most that much when the
        // record stands in for the frame (the margin's rounding term, dtw_margin.hpp); the slot keeps its frames' maximum
        const float r = __double2float_ru(sqrt(res2) / scale * 1.0000001);
        if (r > 0.0f)
            atomicMax(&resid[s], __float_as_uint(r));
        const _Float16 p1 = (_Float16)nrm;
        const _Float16 p2 = (_Float16)(nrm - (double)p1);
        const _Float16 p3 = (_Float16)(nrm - (double)p1 - (double)p2);
        const int mine = nbase + (is_source ? 0 : npieces), other = nbase + (is_source ? npieces : 0);
        out[filter_slot_offset(mine + 0)] = p1;
        out[filter_slot_offset(mine + 1)] = p2;
        out[filter_slot_offset(other + 0)] = (_Float16)1.0f;
        out[filter_slot_offset(other + 1)] = (_Float16)1.0f;
        if (npieces == 3) {
            out[filter_slot_offset(mine + 2)] = p3;
            out[filter_slot_offset(other + 2)] = (_Float16)1.0f;
        }
    }
    if (is_source) {
        _Float16 *dst = rec + ((size_t)s * frames_pad + slot) * kFilterRecHalfs;
#pragma unroll
        for (int i = 0; i < kFilterRecHalfs; ++i)
            dst[i] = out[i];
    } else {
        // group-major target layout (dtw_filter_kernel.hpp, tgt_rec_offset); n_pad is a multiple of 32
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int m = 0; m < kFilterKM; ++m) {
                _Float16 *dst = rec + tgt_rec_offset(s, frames_pad, slot, m, h);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    dst[i] = out[h * 24 + m * 8 + i];
            }
    }
}

// banded layout: slot s of a source holds frame s - r; tile T of column j reads slots j + 16T .. +15
static uint32_t band_slots(int radius, const SegmentSet &src, const SegmentSet &tgt)
{
    const uint32_t kb = (uint32_t)(2 * radius + 1 + 15) / 16 * 16;
    return std::max<uint32_t>(radius + src.max_frames, std::max<uint32_t>(tgt.max_frames, 1) + kb) + 1;
}
static size_t band_lds_bytes(int radius, const SegmentSet &src, const SegmentSet &tgt)
{
    return ((size_t)2 * band_slots(radius, src, tgt) * kFilterRecHalfs + kBandImagePad) * sizeof(_Float16);
}

// A Sakoe-Chiba band the banded kernel cannot take -- more than 6 tiles of diagonals (r > 47), or a source pair that
// does not fit the LDS -- is served by the UNBANDED filter: a band only removes paths, so the unbanded cost bounds the
// banded one from below, and the lower-bound cascade (select.hip, "wide frames") with the banded exact kernel does
// the rest.
bool filter_band_as_bound(const ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt)
{
    if (ctx->band < 0)
        return false;
    return 2 * ctx->band + 1 > 6 * 16 || band_lds_bytes(ctx->band, src, tgt) > 160 * 1024 - 64;   // (+ the kernel's few static bytes)
}

bool filter_supported(const ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt)
{
    if (src.light || tgt.light)
        return false;   // packed for the exact kernels only
    if (src.dim != tgt.dim)
        return false;   // (frames wider than 42 values: match.hip decides, the filter is then a lower bound only)
    if ((ctx->band < 0 || filter_band_as_bound(ctx, src, tgt)) && filter_shape((int)src.max_frames).nt == 0)
        return false;   // more than 4096 source frames
    if (!std::isfinite(src.max_abs) || !std::isfinite(tgt.max_abs))
        return false;   // inf / NaN features: exact kernel keeps IEEE semantics
    if (!std::isfinite(src.max_sqnorm_all) || !std::isfinite(tgt.max_sqnorm_all))
        return false;   // squared frame norms beyond f32: no common scale serves values and norms
    return src.n > 0 && tgt.n > 0;
}

// Common power-of-two scale s: max |s v| < 64 (in [32, 64) unless the norms below ask for less; 1 when
// everything is zero), AND every scaled squared frame norm below the f16 maximum -- the records carry
// |a|^2 as three f16 pieces, and from 17 values per frame on 64^2 * dim passes 65504: the first piece
// would be +inf, the third NaN, and the pair would silently drop out of the search.  A smaller s keeps
// every assumption of the error model (|s v| < 64 is an upper bound; its absolute terms are priced
// through 1 / s^2, dtw_margin.hpp).  max_sqnorm is rounded up and the records' norms are those of the
// f16-rounded frames (<= (1 + 2^-11)^2 larger), hence the slack.
static double common_scale(const SegmentSet &src, const SegmentSet &tgt)
{
    const double m = std::max(src.max_abs, tgt.max_abs);
    if (!(m > 0.0))
        return 1.0;
    int e = 0;
    (void)std::frexp(m, &e);          // m = f * 2^e, f in [0.5, 1)
    e = std::min(std::max(6 - e, -100), 100);
    const double sq = std::max(src.max_sqnorm_all, tgt.max_sqnorm_all);
    while (e > -200 && sq * std::ldexp(1.0, 2 * e) * 1.01 >= 65000.0)
        --e;
    const double ideal = std::ldexp(1.0, e);
    // The dictionary's records are cached on the scale they were built with.  A batch of quieter targets would ask
    // for a larger scale and the next louder one for the smaller again -- a full pass over the dictionary per call,
    // its time depending on the previous call.  A smaller scale than the ideal one is always admissible (|s v| < 64
    // and the norm bound only get easier; the error model prices the scale through 1 / s^2), so the cached scale is
    // kept while it is at most 16 times smaller than the ideal: four bits of the f16 pieces' headroom, not a rebuild.
    if (src.rec && src.rec_scale > 0.0 && src.rec_scale <= ideal && src.rec_scale * 16.0 >= ideal)
        return src.rec_scale;
    return ideal;
}

static int32_t ensure_records(ssym_ctx *ctx, const SegmentSet &set, double scale, uint32_t slots, int lead)
{
    const size_t bytes = (size_t)set.n_pad * slots * kFilterRecHalfs * sizeof(_Float16);
    if (set.rec && set.rec_scale == scale && set.rec_bytes == bytes && set.rec_slots == slots &&
        set.rec_lead == lead)
        return SSYM_OK;
    if (set.rec && set.rec_bytes != bytes) {
        dev_free(ctx, set.rec);
        set.rec = nullptr;
    }
    if (!set.rec) {
        int32_t rca = dev_alloc(ctx, &set.rec, bytes);
        if (rca != SSYM_OK)
            return rca;
    }
    set.rec_bytes = bytes;
    dim3 grid((slots + 63) / 64, set.n_pad);
    const int dimUse = filter_dim_used((int)set.dim);
    unsigned *resid = (unsigned *)(set.max_sqnorm + 2 * (size_t)set.n_pad);      // (non-negative floats: integer maximum)
    SSYM_HIP_CHECK(ctx, hipMemsetAsync(resid, 0, sizeof(unsigned) * set.n_pad, ctx->stream));
    build_filter_records_kernel<<<grid, 64, 0, ctx->stream>>>(set.raw, set.off, set.perm, set.n, set.dim,
                                                              (uint32_t)dimUse, slots, set.is_source ? 1 : 0, lead,
                                                              filter_pieces(dimUse), scale,
                                                              (_Float16 *)set.rec, resid);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    set.rec_scale = scale;
    set.rec_slots = slots;
    set.rec_lead = lead;
    return SSYM_OK;
}

// The unbanded launcher's knobs (FilterKnobs, dtw_filter_plan.hpp), read once per filter call -- the only place that names
// them.  Without the test hooks (one lookup) the product's defaults.
static FilterKnobs read_filter_knobs()
{
    FilterKnobs k;
    g_filter_wg2.store(true, std::memory_order_relaxed);
    g_filter_wg2u.store(true, std::memory_order_relaxed);
    if (!ssym_knob("SSYM_TEST_HOOKS"))
        return k;
    auto num = [](const char *name, int unset) {
        const char *v = ssym_knob(name);
        return v ? atoi(v) : unset;
    };
    k.pk = num("SSYM_FILTER_PK", 0) != 0;
    k.sp = num("SSYM_FILTER_SP", 1) != 0;
    const int mp = num("SSYM_SP_MULTIPAIR", 1);
    k.spMultipair = mp == 0 || mp == 2 ? mp : 1;
    k.spPairBlock = ssym_knob("SSYM_SP_PAIRBLOCK") ? std::max(num("SSYM_SP_PAIRBLOCK", 0), 0) : -1;
    k.wg = num("SSYM_FILTER_WG", k.wg) != 0;
    g_filter_wg2.store(num("SSYM_FILTER_WG2", 1) != 0, std::memory_order_relaxed);
    g_filter_wg2u.store(num("SSYM_FILTER_WG2U", 1) != 0, std::memory_order_relaxed);
    k.skip0 = num("SSYM_FILTER_SKIP0", 1) != 0;
    k.nt8 = ssym_knob("SSYM_FILTER_NT8") != nullptr;
    k.oneLaunch = ssym_knob("SSYM_FILTER_ONE_LAUNCH") != nullptr;
    k.longClasses = num("SSYM_FILTER_LONG_CLASSES", 1) != 0;
    k.pruneNt = num("SSYM_PRUNE_NT", 0);
    return k;
}

// The plan's view of a set: the frames of the longest member of every `group` consecutive record slots -- source pairs (2),
// target groups (32); slots [0, n) are real, ascending by length, the rest padding.  Built on a set's first filter call
// (pack drops it): a search of 4096 x 4096 short segments is 1.6 ms, walking both sets' offsets 10 us of host time in
// front of its first launch.
static const std::vector<uint32_t> &plan_lens(const SegmentSet &set, uint32_t group)
{
    if (set.plan_lens.size() != set.n_pad / group) {       // (not built yet, or built for the set in the other role)
        set.plan_lens.assign(set.n_pad / group, 0u);
        set.plan_min_lens.assign(set.n_pad / group, 0xffffffffu);
        for (uint32_t slot = 0; slot < set.n; ++slot) {
            const uint32_t s = set.h_perm[slot];
            const uint32_t f = (uint32_t)(set.h_off[s + 1] - set.h_off[s]);
            uint32_t &m = set.plan_lens[slot / group], &lo = set.plan_min_lens[slot / group];
            m = std::max(m, f);
            lo = std::min(lo, f);
        }
    }
    return set.plan_lens;
}

// The uniform gate's facts, kept with the set beside plan_lens (built with them): the one frame count of the real members
// of the groups [lo, hi), 0 when they differ or when one of the groups' slots is padding.  (Slots ascend by length: the
// range's shortest member is in its first group, its longest in its last.)
static uint32_t uniform_len(const SegmentSet &set, uint32_t group, uint32_t lo, uint32_t hi)
{
    const std::vector<uint32_t> &longest = plan_lens(set, group);
    if (lo >= hi || hi > longest.size() || (uint64_t)hi * group > set.n)
        return 0;
    return set.plan_min_lens[lo] == longest[hi - 1] ? longest[hi - 1] : 0;
}

// what every launch of one filter call shares
struct FilterCall {
    hipStream_t st;
    const SegmentSet &src, &tgt;
    bool sq;                        // squared local costs
    int ku;                         // operand planes
    float outScale;
    float *handoff;
    unsigned *taskCtr;              // kMaxClasses sets of 8 counters
    float *cmat;
    const float *abandon;
    unsigned long long *colCtr;
    const uint32_t *candSlot;
    bool wg2;                       // two-pass Wg launches on dtw_filter_wg2_kernel (SSYM_FILTER_WG2)
    uint32_t uniF;                  // the targets' one frame count when wg2's uniform instantiation may serve them, else 0
};

// One entry of the plan as the kernel launch it names: the instantiations of (tiles per pass, cost, operand planes).
// false: the plan names a kernel these parameters have none of.
template <int NT, bool SQ, int KU>
static bool run_kernel(const FilterCall &c, const FilterLaunch &l)
{
    constexpr int OCC = NT == 1 ? 3 : NT == 8 ? 1 : 2;
    const dim3 grid(l.grid), block(64 * kFilterWavesPerBlock);
    const _Float16 *srec = (const _Float16 *)c.src.rec, *trec = (const _Float16 *)c.tgt.rec;
    const int rowsPad = (int)c.src.frames_pad, colsPad = (int)c.tgt.frames_pad, tgtPad = (int)c.tgt.n_pad;
    const int nSrcPairs = l.hi - l.lo, nTasks = nSrcPairs * (tgtPad / 32);
    unsigned *ctr = c.taskCtr + l.ctrSet * 8 * kTaskCtrStride;
    switch (l.kind) {
    case FilterKernel::Mp:
        if constexpr (NT == 1) {
            dtw_filter_sp_kernel<KU == 2 ? 3 : 2, SQ, 2, KU, kSpRowBlock, true><<<grid, block, 0, c.st>>>(
                srec, trec, c.src.len, c.tgt.len, rowsPad, colsPad, tgtPad, l.taskPairs, nSrcPairs, l.taskChunk, c.outScale,
                ctr, c.cmat, l.origin, l.lo, l.pairBlock);
            return true;
        }
        return false;
    case FilterKernel::Sp:
        if constexpr (NT <= 3 && (KU == 2 || NT <= 2)) {
            constexpr int OCCSP = (NT == 1 && KU == 2) ? 3 : (NT == 2 && KU == 2) ? SSYM_SP_OCC_NT2 : 2;
            dtw_filter_sp_kernel<NT, SQ, OCCSP, KU, kSpRowBlock><<<grid, block, 0, c.st>>>(
                srec, trec, c.src.len, c.tgt.len, rowsPad, colsPad, tgtPad, nSrcPairs, nTasks, l.taskChunk, c.outScale, ctr,
                c.cmat, l.origin, l.lo, l.pairBlock);
            return true;
        }
        return false;
    case FilterKernel::GenericSkip0:
        if constexpr (NT == 3 || NT == 4) {
            dtw_filter_kernel<NT, SQ, OCC, false, KU, true><<<grid, block, 0, c.st>>>(
                srec, trec, c.src.len, c.tgt.len, rowsPad, l.passes, colsPad, tgtPad, nSrcPairs, nTasks, l.taskChunk,
                c.outScale, c.handoff, ctr, c.cmat, nullptr, nullptr, nullptr, l.origin, l.lo);
            return true;
        }
        return false;
    case FilterKernel::Wg:
        if constexpr (NT == 4) {
            // exactly two passes: both at once on two waves per pair, the hand-off in LDS (dtw_filter_wg2_kernel.hpp)
            if (l.passes == 2 && c.wg2) {
                // lengths that do not differ -- every target real and of c.uniF frames, every source of the launch's pairs
                // of uniFa, the launch's rows the slots' last 128: the instantiation without the lengths' bookkeeping
                const uint32_t uniFa = c.uniF && rowsPad - l.origin == 128 ? uniform_len(c.src, 2, l.lo, l.hi) : 0;
                if (uniFa > 64 && uniFa <= 128) {
                    dtw_filter_wg2_kernel<SQ, KU, true><<<grid, block, 0, c.st>>>(
                        srec, trec, c.src.len, c.tgt.len, rowsPad, colsPad, tgtPad, nSrcPairs / 4, l.taskChunk, c.outScale, ctr,
                        c.cmat, l.origin, l.lo, (int)c.uniF, (int)uniFa);
                    g_filter_wg_launches.fetch_add(1, std::memory_order_relaxed);
                    g_filter_wg2_launches.fetch_add(1, std::memory_order_relaxed);
                    g_filter_wg2u_launches.fetch_add(1, std::memory_order_relaxed);
                    return true;
                }
                dtw_filter_wg2_kernel<SQ, KU><<<grid, block, 0, c.st>>>(
                    srec, trec, c.src.len, c.tgt.len, rowsPad, colsPad, tgtPad, nSrcPairs / 4, l.taskChunk, c.outScale, ctr,
                    c.cmat, l.origin, l.lo);
                g_filter_wg_launches.fetch_add(1, std::memory_order_relaxed);
                g_filter_wg2_launches.fetch_add(1, std::memory_order_relaxed);
                return true;
            }
            dtw_filter_wg_kernel<SQ, KU><<<grid, block, 0, c.st>>>(
                srec, trec, c.src.len, c.tgt.len, rowsPad, l.passes, colsPad, tgtPad, nSrcPairs / 4, l.taskChunk, c.outScale,
                c.handoff, ctr, c.cmat, l.origin, l.lo);
            g_filter_wg_launches.fetch_add(1, std::memory_order_relaxed);
            return true;
        }
        return false;
    case FilterKernel::Pk:
        if constexpr (NT == 4) {
            dtw_filter_pk_kernel<SQ, KU><<<grid, block, 0, c.st>>>(
                srec, trec, c.src.len, c.tgt.len, rowsPad, l.passes, colsPad, tgtPad, nSrcPairs, nTasks, l.taskChunk,
                c.outScale, c.handoff, ctr, c.cmat, l.origin, l.lo);
            return true;
        }
        return false;
    case FilterKernel::GenericPrune:
        dtw_filter_kernel<NT, SQ, OCC, true, KU><<<grid, block, 0, c.st>>>(
            srec, trec, c.src.len, c.tgt.len, rowsPad, l.passes, colsPad, tgtPad, nSrcPairs, nTasks, l.taskChunk, c.outScale,
            c.handoff, ctr, c.cmat, c.abandon, c.colCtr, c.candSlot, l.origin, l.lo);
        return true;
    case FilterKernel::Generic:
        dtw_filter_kernel<NT, SQ, OCC, false, KU><<<grid, block, 0, c.st>>>(
            srec, trec, c.src.len, c.tgt.len, rowsPad, l.passes, colsPad, tgtPad, nSrcPairs, nTasks, l.taskChunk, c.outScale,
            c.handoff, ctr, c.cmat, nullptr, nullptr, nullptr, l.origin, l.lo);
        return true;
    }
    return false;
}

template <int NT>
static bool run_tiles(const FilterCall &c, const FilterLaunch &l)
{
    if (c.sq)
        return c.ku == 2 ? run_kernel<NT, true, 2>(c, l) : run_kernel<NT, true, 3>(c, l);
    return c.ku == 2 ? run_kernel<NT, false, 2>(c, l) : run_kernel<NT, false, 3>(c, l);
}

static bool run_launch(const FilterCall &c, const FilterLaunch &l)
{
    switch (l.nt) {
    case 1: return run_tiles<1>(c, l);
    case 2: return run_tiles<2>(c, l);
    case 3: return run_tiles<3>(c, l);
    case 4: return run_tiles<4>(c, l);
    case 8: return run_tiles<8>(c, l);      // SSYM_FILTER_NT8
    }
    return false;
}

template <int NTB, int WB, int OCC, bool SQ, int LASTN, bool PRUNE>
static int32_t launch_band_cfg2(ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, uint32_t slots,
                                size_t lds, float outScale, float *cmat, const float *abandon,
                                unsigned long long *colCtr, const uint32_t *candSlot)
{
    const int nTgtBlocks = (int)tgt.n_pad / (32 * WB);
    const int nTasks = ((int)src.n_pad / 2) * nTgtBlocks;
    const int grid = std::max(1, std::min(ctx->num_cus, nTasks));
    int32_t rc = ensure(ctx, ctx->handoff, 8 * sizeof(unsigned));      // the banded kernel's task counter
    if (rc != SSYM_OK)
        return rc;
    unsigned *taskCtr = (unsigned *)ctx->handoff.ptr;
    rc = zero_words(ctx, taskCtr, sizeof(unsigned));
    if (rc != SSYM_OK)
        return rc;
    // operand planes the kernel multiplies: record layout 3 leaves the third one zero
    const bool two = filter_mfmas(filter_pieces(filter_dim_used((int)src.dim)), filter_dim_used((int)src.dim)) == 2;
    auto kern = two ? dtw_band_kernel<NTB, WB, OCC, SQ, LASTN, PRUNE, 2> : dtw_band_kernel<NTB, WB, OCC, SQ, LASTN, PRUNE, 3>;
    // two columns per source read (dtw_band_kernel.hpp, PC): an experiment that measured nothing (LAB.md R4.3), kept out of
    // the product library -- tools/band_paircols_ab.py builds its own with EXTRA=-DSSYM_BAND_PAIRCOLS_BUILD
#ifdef SSYM_BAND_PAIRCOLS_BUILD
    if constexpr (!PRUNE && LASTN == 1 && NTB >= 4 && OCC == 2) {
        const char *pc = ssym_knob("SSYM_BAND_PAIRCOLS");
        if (pc && atoi(pc) != 0)
            kern = two ? dtw_band_kernel<NTB, WB, OCC, SQ, LASTN, PRUNE, 2, true> : dtw_band_kernel<NTB, WB, OCC, SQ, LASTN, PRUNE, 3, true>;
    }
#endif
    if (lds > 64 * 1024)
        SSYM_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<dim3(grid), 64 * WB, lds, ctx->stream>>>(
        (const _Float16 *)src.rec, (const _Float16 *)tgt.rec, src.len, tgt.len, (int)slots, ctx->band,
        (int)tgt.frames_pad, (int)tgt.n_pad, nTgtBlocks, nTasks, taskCtr, outScale, cmat, abandon, colCtr, candSlot);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

template <int NTB, int WB, int OCC, bool SQ, int LASTN>
static int32_t launch_band_cfg(ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, uint32_t slots,
                               size_t lds, float outScale, float *cmat, const float *abandon,
                               unsigned long long *colCtr, const uint32_t *candSlot)
{
    return abandon ? launch_band_cfg2<NTB, WB, OCC, SQ, LASTN, true>(ctx, src, tgt, slots, lds, outScale, cmat, abandon, colCtr, candSlot)
                   : launch_band_cfg2<NTB, WB, OCC, SQ, LASTN, false>(ctx, src, tgt, slots, lds, outScale, cmat, nullptr, nullptr, nullptr);
}

// Up to 5 tiles of diagonals (r <= 39) run two waves per SIMD (8-wave workgroups); at 4 and 5 tiles
// that costs a few register spills but measured 10 % faster than one wave per SIMD at r = 32.
// 6 tiles run one wave per SIMD (4-wave workgroups) with the whole register file.  (Only the variant a tile count
// uses is instantiated: the other half of the kernels doubled the compile time for a tuning knob.)
template <int NTB, bool SQ>
static int32_t launch_band(ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, uint32_t slots,
                           size_t lds, float outScale, float *cmat, const float *abandon, unsigned long long *colCtr, const uint32_t *candSlot)
{
    // radii that are multiples of 8 end exactly one diagonal into their last tile
    const bool last1 = 2 * ctx->band + 1 == 16 * (NTB - 1) + 1;
    if constexpr (NTB <= 5)
        return last1 ? launch_band_cfg<NTB, 8, 2, SQ, 1>(ctx, src, tgt, slots, lds, outScale, cmat, abandon, colCtr, candSlot)
                     : launch_band_cfg<NTB, 8, 2, SQ, 16>(ctx, src, tgt, slots, lds, outScale, cmat, abandon, colCtr, candSlot);
    else
        return last1 ? launch_band_cfg<NTB, 4, 1, SQ, 1>(ctx, src, tgt, slots, lds, outScale, cmat, abandon, colCtr, candSlot)
                     : launch_band_cfg<NTB, 4, 1, SQ, 16>(ctx, src, tgt, slots, lds, outScale, cmat, abandon, colCtr, candSlot);
}

static int32_t launch_dtw_filter_banded(ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, float *cmat,
                                        const float *abandon, unsigned long long *colCtr, const uint32_t *candSlot)
{
    if (tgt.n_pad % kBandTgtQuantum != 0 || src.n_pad % 2 != 0) {
        ctx->err = "dtw band filter: segment set not padded for the banded kernel";
        return SSYM_E_UNSUPPORTED;
    }
    const uint32_t slots = band_slots(ctx->band, src, tgt);
    const size_t lds = band_lds_bytes(ctx->band, src, tgt);
    const double scale = common_scale(src, tgt);
    int32_t rc = ensure_records(ctx, src, scale, slots, ctx->band);
    if (rc != SSYM_OK)
        return rc;
    rc = ensure_records(ctx, tgt, scale, tgt.frames_pad, 0);
    if (rc != SSYM_OK)
        return rc;
    const bool sq = ctx->squared != 0;
    const float outScale = (float)(sq ? 1.0 / (scale * scale) : 1.0 / scale);
    const int ntb = (2 * ctx->band + 1 + 15) / 16;
#define SSYM_BCASE(N_)                                                                                  \
    case N_:                                                                                            \
        return sq ? launch_band<N_, true>(ctx, src, tgt, slots, lds, outScale, cmat, abandon, colCtr, candSlot)   \
                  : launch_band<N_, false>(ctx, src, tgt, slots, lds, outScale, cmat, abandon, colCtr, candSlot);
    switch (ntb) {
        SSYM_BCASE(1) SSYM_BCASE(2) SSYM_BCASE(3) SSYM_BCASE(4) SSYM_BCASE(5) SSYM_BCASE(6)
    default:
        ctx->err = "dtw band filter: band radius too large";
        return SSYM_E_UNSUPPORTED;
    }
#undef SSYM_BCASE
}

int32_t ensure_filter_records(ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, double *scale_out)
{
    const double scale = common_scale(src, tgt);
    int32_t rc = ctx->band >= 0 && !filter_band_as_bound(ctx, src, tgt)
                     ? ensure_records(ctx, src, scale, band_slots(ctx->band, src, tgt), ctx->band)
                     : ensure_records(ctx, src, scale, src.frames_pad, -1);
    if (rc == SSYM_OK)
        rc = ensure_records(ctx, tgt, scale, tgt.frames_pad, 0);
    if (scale_out)
        *scale_out = scale;
    return rc;
}

int32_t launch_dtw_filter(ssym_ctx *ctx, const SegmentSet &src, const SegmentSet &tgt, float *cmat,
                          const float *abandon, unsigned long long *colCtr, const uint32_t *candSlot)
{
    ctx->filter_launches = 1;
    if (ctx->band >= 0 && !filter_band_as_bound(ctx, src, tgt))
        return launch_dtw_filter_banded(ctx, src, tgt, cmat, abandon, colCtr, candSlot);
    const FilterShape shape = filter_shape((int)src.max_frames);
    if (shape.nt == 0 || (int)src.frames_pad != shape.rows() || src.n_pad % 8 != 0 || tgt.n_pad % 32 != 0) {
        ctx->err = "dtw filter: segment set not padded for the filter kernel";
        return SSYM_E_UNSUPPORTED;
    }
    // the kernel addresses a wave's hand-off row as a buffer: 32-bit byte offsets, a signed extent in the descriptor
    if (((size_t)tgt.frames_pad + 3) / 4 * 1024 >= ((size_t)1 << 31)) {
        ctx->err = "dtw filter: targets too long for the hand-off rows";
        return SSYM_E_UNSUPPORTED;
    }
    const double scale = common_scale(src, tgt);
    int32_t rc = ensure_records(ctx, src, scale, src.frames_pad, -1);
    if (rc != SSYM_OK)
        return rc;
    rc = ensure_records(ctx, tgt, scale, tgt.frames_pad, 0);
    if (rc != SSYM_OK)
        return rc;
    // persistent grid: 2 workgroups of 4 waves per CU (2 waves per SIMD), a multiple of 8 so that
    // task & 7 is the XCD group; one hand-off row of [target frames][64] floats per wave
    const int gridBlocks = std::max(8, ctx->num_cus * 2 / 8 * 8);
    // + kMaxClasses x 8 task counters behind the hand-off rows (one set per launch of the plan)
    // (sized for the three-workgroups-per-CU launch of the one-tile kernel too)
    const size_t handBytes = (size_t)(gridBlocks / 2 * 3) * kFilterWavesPerBlock * ((tgt.frames_pad + 3) / 4) * 256 * sizeof(float);
    const size_t ctrBytes = 8 * kTaskCtrStride * sizeof(unsigned);
    rc = ensure(ctx, ctx->handoff, handBytes + kMaxClasses * ctrBytes);
    if (rc != SSYM_OK)
        return rc;
    unsigned *taskCtr = (unsigned *)((char *)ctx->handoff.ptr + handBytes);
    rc = zero_words(ctx, taskCtr, kMaxClasses * ctrBytes);
    if (rc != SSYM_OK)
        return rc;
    const bool sq = ctx->squared != 0;
    const int dimUse = filter_dim_used((int)src.dim);

    FilterPlanInput in;
    in.pairLen = plan_lens(src, 2).data(), in.groupCols = plan_lens(tgt, 32).data();
    in.srcN = src.n, in.srcNPad = src.n_pad, in.framesPad = src.frames_pad;
    in.tgtN = tgt.n, in.tgtGroups = tgt.n_pad / 32, in.tgtTotalFrames = tgt.total_frames;
    in.numCus = ctx->num_cus;
    // operand planes the kernels multiply: record layout 3 leaves the third one zero
    in.ku = filter_mfmas(filter_pieces(dimUse), dimUse);
    in.abandon = abandon != nullptr;
    in.pruneSwept = ctx->prune_swept;
    in.knobs = read_filter_knobs();
    const std::vector<FilterLaunch> plan = plan_filter(in);

    ctx->filter_launches = (int)plan.size();
    ctx->launched_cells = 0;
    for (const FilterLaunch &l : plan)
        ctx->launched_cells += l.cells;
    // wg2's uniform instantiation: every target real and of one frame count, at least four and a multiple of four
    uint32_t uniF = g_filter_wg2u.load(std::memory_order_relaxed) && !abandon && tgt.n == tgt.n_pad
                        ? uniform_len(tgt, 32, 0, tgt.n_pad / 32) : 0;
    if (uniF < 4 || uniF % 4 != 0 || uniF > tgt.frames_pad)
        uniF = 0;
    const FilterCall call{ctx->stream, src, tgt, sq, in.ku, (float)(sq ? 1.0 / (scale * scale) : 1.0 / scale),
                          (float *)ctx->handoff.ptr, taskCtr, cmat, abandon, colCtr, candSlot,
                          g_filter_wg2.load(std::memory_order_relaxed), uniF};
    for (const FilterLaunch &l : plan)
        if (!run_launch(call, l)) {
            ctx->err = "dtw filter: the plan names a kernel that is not built";
            return SSYM_E_UNSUPPORTED;
        }
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

}  // namespace ssym

// tests and tools: launches of dtw_filter_wg_kernel in this process so far
extern "C" __attribute__((visibility("default"))) unsigned long long ssym_debug_filter_wg_launches(void)
{
    return ssym::g_filter_wg_launches.load(std::memory_order_relaxed);
}

// ... and those of them that were launches of dtw_filter_wg2_kernel
extern "C" __attribute__((visibility("default"))) unsigned long long ssym_debug_filter_wg2_launches(void)
{
    return ssym::g_filter_wg2_launches.load(std::memory_order_relaxed);
}

// ... and those of them that took its uniform-length instantiation
extern "C" __attribute__((visibility("default"))) unsigned long long ssym_debug_filter_wg2u_launches(void)
{
    return ssym::g_filter_wg2u_launches.load(std::memory_order_relaxed);
}

#ifdef SSYM_SP_PROF
// tools only: read and clear the single-pass kernel's tick sums (dtw_filter_sp_kernel.hpp)
extern "C" __attribute__((visibility("default"))) int ssym_debug_sp_prof(unsigned long long *out)
{
    unsigned long long zero[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ssym::ssym_sp_prof), sizeof(zero)) != hipSuccess)
        return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(ssym::ssym_sp_prof), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif
