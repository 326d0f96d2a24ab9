// dtw_align.hip -- DTW alignment: the optimal warping path of a list of (source, target) pairs, its cost and the
// per-target-frame map onto source frames (DESIGN.md 2 "Alignment", 5.12).
//
// Role on the path: ssym_match_* answer "how far apart"; this answers "which frame goes with which" for the pairs a
// match has chosen (thousands after one ssym_match_queries), in one launch and one synchronisation.
//
// Arithmetic: dtw_wave.hpp's, so D(Fa-1, Fb-1) has the bits ssym_pair_matrix(exact = 1) returns; the backward rule is
// its predecessor rule on those exact values.
//
// Mapping: one wave per pair, grid-stride over the list.
//   forward   dtw_wave.hpp's wavefront, inside the band if there is one, from a virtual D(-1,-1) = 0.  Each lane has
//             dg, up, lf in registers when it forms min3; the 2-bit step code goes into a dword of 16 codes per row,
//             stored when full.  The direction matrix (Fa x ceil(Fb / 16) dwords) lives in LDS when it fits
//             kAlignDirLdsBytes, else in this workgroup's slab of global scratch.
//   backward  lane 0 walks the codes from (Fa-1, Fb-1) to (0, 0): one dependent read per step, one code byte into
//             LDS per step.  Other waves of the CU hide it (a pair of 128 x 128 frames takes about 20 KB of LDS).
//   output    the wave turns the reversed code string into cells with two ballots per 64 steps (i and j of path
//             position f are the numbers of row / column steps before f) and writes the path in forward order and
//             the map (the first cell of every column) with coalesced vector stores.
#include "dtw_wave.hpp"

#include <algorithm>

namespace ssym {

// Limits of ssym_dtw_align (soundsym_amd.h): frames per segment of a listed pair, values per frame
constexpr int kAlignMaxFrames = 4096;
constexpr int kAlignMaxDim = 64;
// Limit of ssym_dtw_align_step with SSYM_STEP_PACED: frames of a listed target (two f64 hand-off rows, 16 bytes per target
// frame; the paced spot kernels' limit, so that every span they report can be aligned); a source keeps kAlignMaxFrames
constexpr int kAlignPacedMaxTargetFrames = 2048;
// a pair whose direction matrix (Fa * ceil(Fb / 16) * 4 bytes) is at most this keeps it in LDS, a larger one uses global scratch
constexpr int kAlignDirLdsBytes = 16384;
// global scratch of one call: at most this many bytes of direction slabs (one per workgroup)
constexpr size_t kAlignScratchBytes = (size_t)512 << 20;

namespace {

struct AlignArgs {
    const double *srcRaw;
    const uint64_t *srcOff;
    const double *tgtRaw;
    const uint64_t *tgtOff;
    uint32_t dim;
    int band, squared;
    const uint2 *pairs;          // (source, target); source 0xffffffff = no match
    uint32_t nPairs;
    const uint64_t *pathOff;     // [nPairs + 1] in steps
    const uint64_t *mapOff;      // [nPairs + 1] in frames (NULL with map == NULL)
    double *cost;                // [nPairs]
    uint32_t *len;               // [nPairs]
    uint2 *path;
    uint32_t *map;               // nullable
    uint32_t fbCap;              // even, >= the longest listed target
    uint32_t ringRows;           // 64 or 128
    uint32_t codeCap;            // bytes of the code string (>= longest Fa + Fb - 1, a multiple of 16); paced: of the row of i_j (4 fbCap)
    uint32_t dirLdsBytes;        // LDS room of the direction matrix
    uint32_t *slabs;             // global direction slabs, slabWords each (NULL: every listed pair fits LDS)
    uint64_t slabWords;
};

template <int DIMR>
__global__ __launch_bounds__(64) void dtw_align_kernel(const AlignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int LD = wave_ld(DIMR);
    double *bound = smem;                                           // [fbCap]   bottom row of the chunk above
    double *ring = smem + a.fbCap;                                  // [ringRows][LD]
    unsigned char *codes = reinterpret_cast<unsigned char *>(ring + (size_t)a.ringRows * LD);     // [codeCap]
    uint32_t *dirLds = reinterpret_cast<uint32_t *>(codes + a.codeCap);                         // [dirLdsBytes / 4]
    const double INF = __builtin_inf();
    const int lane = threadIdx.x;
    const int dim = (int)a.dim, band = a.band;
    const uint32_t ringMask = a.ringRows - 1;

    for (uint32_t k = blockIdx.x; k < a.nPairs; k += gridDim.x) {
        const uint2 p = a.pairs[k];
        int Fa = 0, Fb = 0;
        if (p.x != 0xffffffffu) {
            Fa = (int)(a.srcOff[p.x + 1] - a.srcOff[p.x]);
            Fb = (int)(a.tgtOff[p.y + 1] - a.tgtOff[p.y]);
        }
        if (Fa == 0 || Fb == 0) {
            if (lane == 0) {
                a.cost[k] = INF;
                a.len[k] = 0;
            }
            continue;
        }
        const double *a0 = a.srcRaw + a.srcOff[p.x] * dim;
        const double *b0 = a.tgtRaw + a.tgtOff[p.y] * dim;
        const uint32_t rowWords = ((uint32_t)Fb + 15) >> 4;
        const bool dirInLds = (uint64_t)Fa * rowWords * 4 <= a.dirLdsBytes;
        uint32_t *dirG = a.slabs + (size_t)blockIdx.x * a.slabWords;     // only touched when !dirInLds (then slabs != NULL)

        __syncthreads();   // the previous pair's LDS reads are done
        for (int j = lane; j < Fb; j += 64)
            bound[j] = INF;
        double result = INF;
        for (int c0 = 0; c0 < Fa; c0 += 64) {
            const int r = c0 + lane;
            const bool rowValid = r < Fa;
            const int rowsHere = min(64, Fa - c0);
            double ar[DIMR];
            {   // wave_load_frame's text: see the note at the ring refill below
                const double *arow = a0 + (size_t)(rowValid ? r : c0) * dim;
#pragma unroll
                for (int e = 0; e < DIMR; ++e)
                    ar[e] = e < dim ? arow[e] : 0.0;
            }
            int jlo = 0, jhi = Fb - 1;
            if (band >= 0) {
                jlo = max(0, c0 - band);
                jhi = min(Fb - 1, c0 + rowsHere - 1 + band);
            }
            double mine = INF;      // D(r, j-1)
            double diagReg = INF;   // D(r-1, j-1)
            uint32_t pack = 0;      // step codes of this row's current group of 16 columns
            const int tauEnd = jhi + rowsHere;     // exclusive: lane l works on column tau - l
            for (int tau = jlo; tau < tauEnd; ++tau) {
                if (tau == jlo || (tau & 63) == 0) {
                    // wave_refill(..., tau & ~63), written out: called as functions, this and the frame load above
                    // change the register allocation of this kernel (not of dtw_spot_kernel) and <40> runs 1 - 3 % slower
                    const int f0 = tau & ~63;
                    const int cnt = min(64, Fb - f0);
                    __syncthreads();
                    for (int i = lane; i < cnt * DIMR; i += 64) {
                        const int fr = i / DIMR, e = i % DIMR;
                        ring[(size_t)((uint32_t)(f0 + fr) & ringMask) * LD + e] = e < dim ? b0[(size_t)(f0 + fr) * dim + e] : 0.0;
                    }
                    __syncthreads();
                }
                const int j = tau - lane;
                const double c = wave_cell_cost(ar, ring, ringMask, min(max(j, 0), Fb - 1), a.squared);
                double up = shfl_up1(mine);               // D(r-1, j) for lanes >= 1
                double dg = diagReg;
                if (lane == 0) {
                    if (c0 == 0) {
                        up = INF;
                        dg = (j == 0) ? 0.0 : INF;        // virtual D(-1,-1) = 0
                    } else {
                        up = (j >= 0 && j < Fb) ? bound[j] : INF;
                        dg = (j >= 1 && j <= Fb) ? bound[j - 1] : INF;
                    }
                }
                const bool active = rowValid && j >= 0 && j < Fb;
                if (active) {
                    double cur = INF;
                    const int dij = r - j;
                    if (band < 0 || (dij <= band && -dij <= band)) {
                        cur = __dadd_rn(c, wave_min3(up, mine, dg));
                        pack |= wave_pred(up, mine, dg) << (2 * (j & 15));
                    }
                    if (j <= jhi && ((j & 15) == 15 || j == jhi)) {     // (columns beyond jhi are outside every row's band)
                        const size_t w = (size_t)r * rowWords + ((uint32_t)j >> 4);
                        if (dirInLds)
                            dirLds[w] = pack;
                        else
                            dirG[w] = pack;
                        pack = 0;
                    }
                    if (lane == 63)
                        bound[j] = cur;
                    if (r == Fa - 1 && j == Fb - 1)
                        result = cur;
                    mine = cur;
                }
                diagReg = up;
            }
        }
        const double total = __shfl(result, (Fa - 1) & 63);
        if (lane == 0)
            a.cost[k] = total;
        if (!(total < INF)) {      // +inf or NaN: no path (dtw_exact.hip never forms -inf: every term is >= 0)
            if (lane == 0)
                a.len[k] = 0;
            continue;
        }
        // the codes this wave stored are read back by its lane 0: LDS after a barrier; the slab after the stores have
        // left the wave (release) and by loads that bypass this CU's L1, which may hold lines of the previous pair
        if (!dirInLds)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        int steps = 0;
        if (lane == 0) {
            int i = Fa - 1, j = Fb - 1;
            while (i > 0 || j > 0) {
                const size_t w = (size_t)i * rowWords + ((uint32_t)j >> 4);
                const uint32_t word = dirInLds ? dirLds[w] : __hip_atomic_load(dirG + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                uint32_t code = (word >> (2 * (j & 15))) & 3u;
                // (row 0 can only go left and column 0 only up: the rule says so too, the walk never leaves the matrix)
                code = i == 0 ? 2u : j == 0 ? 1u : code;
                codes[steps++] = (unsigned char)code;
                i -= code != 2u;
                j -= code != 1u;
            }
        }
        __syncthreads();
        const int L = __builtin_amdgcn_readfirstlane(steps) + 1;
        if (lane == 0)
            a.len[k] = (uint32_t)L;
        uint2 *path = a.path + a.pathOff[k];
        uint32_t *map = a.map ? a.map + a.mapOff[k] : nullptr;
        // path position f is entered by walk step L - 1 - f; its cell = (row steps, column steps) up to and including it
        int ci = 0, cj = 0;
        for (int base = 0; base < L; base += 64) {
            const int f = base + lane;
            uint32_t code = 3u;      // position 0 and positions beyond the path: no step
            if (f >= 1 && f < L)
                code = codes[L - 1 - f];
            const bool di = code == 0u || code == 1u, dj = code == 0u || code == 2u;
            const unsigned long long mi = __ballot(di), mj = __ballot(dj);
            const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1);
            const int i = ci + __popcll(mi & le), j = cj + __popcll(mj & le);
            if (f < L) {
                path[f] = make_uint2((uint32_t)i, (uint32_t)j);
                if (map && (f == 0 || dj))
                    map[j] = (uint32_t)i;        // the first cell of column j on the path holds its smallest i
            }
            ci += __popcll(mi);
            cj += __popcll(mj);
        }
    }
}

// Paced alignment (ssym_dtw_align_step with SSYM_STEP_PACED; DESIGN.md 2 "Paced alignment", 5.19): the path of the paced
// step pattern between pinned ends.  N, H, E and the arithmetic are the paced cell's (dtw_wave.hpp: SSYM_PACED_PRED,
// SSYM_PACED_STATES -- the text dtw_paced_kernel runs, so a cost here has a paced spot's bits); what differs is
// column 0 (N(0,0) = c(0,0), every other row +inf: the path starts at source frame 0) and what a cell leaves behind: no
// start word, but one bit per comparison of the cell -- skip (P came from row i - 2) and rep (H < N) -- packed 16 per
// dword like dtw_align_kernel's codes, in LDS up to dirLdsBytes and in the workgroup's global slab beyond.
//   forward   dtw_paced_kernel's wavefront: N and E of the previous column per lane, d1 = E(r-1, j-1) and d2 = E(r-2, j-1)
//             by DPP, two f64 hand-off rows written in place by lanes 63 and 62 (the order argument is the one given there)
//   backward  lane 0 walks Fb - 1 steps from (Fa-1, Fb-1) with the wanted state in a register: E (the cell's better state:
//             H if rep, else N) or N (the cell was left by a repeat, which may only follow a source step).  State H: the cell
//             before is (i, j-1), wanted in state N.  State N: the cell before is (i-2, j-1) if skip, else (i-1, j-1),
//             wanted in state E.  One dependent read and one LDS word (the row of column j) per step; the row is clamped at 0.
//   output    every admissible path has one cell per target frame: path[j] = (i_j, j), map[j] = i_j, len = Fb, stored
//             coalesced from the LDS row.  A pair whose shape admits no path (Fa outside floor((Fb-1)/2)+1 ... 2 Fb - 1) is
//             decided before the recurrence; a cost that is not finite writes cost and len = 0 alone.
template <int DIMR>
__global__ __launch_bounds__(64) void dtw_align_paced_kernel(const AlignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int LD = wave_ld(DIMR);
    double *bound1 = smem;                                          // [fbCap]   E of row c0 - 1
    double *bound2 = smem + a.fbCap;                                // [fbCap]   E of row c0 - 2
    double *ring = smem + 2 * (size_t)a.fbCap;                      // [ringRows][LD]
    uint32_t *rows = reinterpret_cast<uint32_t *>(ring + (size_t)a.ringRows * LD);                // [codeCap / 4]  i_j
    uint32_t *dirLds = rows + a.codeCap / 4;                                                    // [dirLdsBytes / 4]
    const double INF = __builtin_inf();
    const int lane = threadIdx.x;
    const int dim = (int)a.dim;
    const uint32_t ringMask = a.ringRows - 1;

    for (uint32_t k = blockIdx.x; k < a.nPairs; k += gridDim.x) {
        const uint2 p = a.pairs[k];
        int Fa = 0, Fb = 0;
        if (p.x != 0xffffffffu) {
            Fa = (int)(a.srcOff[p.x + 1] - a.srcOff[p.x]);
            Fb = (int)(a.tgtOff[p.y + 1] - a.tgtOff[p.y]);
        }
        // nothing to align, or a shape no admissible path fits: one source frame per target frame, steps of 0, 1 or 2
        if (Fa == 0 || Fb == 0 || Fa < (Fb - 1) / 2 + 1 || Fa > 2 * Fb - 1) {
            if (lane == 0) {
                a.cost[k] = INF;
                a.len[k] = 0;
            }
            continue;
        }
        const double *a0 = a.srcRaw + a.srcOff[p.x] * dim;
        const double *b0 = a.tgtRaw + a.tgtOff[p.y] * dim;
        const uint32_t rowWords = ((uint32_t)Fb + 15) >> 4;
        const bool dirInLds = (uint64_t)Fa * rowWords * 4 <= a.dirLdsBytes;
        uint32_t *dirG = a.slabs + (size_t)blockIdx.x * a.slabWords;     // only touched when !dirInLds (then slabs != NULL)

        double result = INF;
        for (int c0 = 0; c0 < Fa; c0 += 64) {
            const int r = c0 + lane;
            const bool rowValid = r < Fa;
            const int rowsHere = min(64, Fa - c0);
            double ar[DIMR];
            wave_load_frame(ar, a0 + (size_t)(rowValid ? r : c0) * dim, dim);
            double mineN = INF, mineE = INF;                        // N(r, j-1), E(r, j-1)
            double d1 = INF, d2 = INF;                              // E(r-1, j-1), E(r-2, j-1)
            uint32_t pack = 0;                                      // codes of this row's current group of 16 columns
            const int tauEnd = Fb - 1 + rowsHere;     // exclusive: lane l works on column tau - l
            for (int tau = 0; tau < tauEnd; ++tau) {
                // (the refill's barrier also orders the hand-off rows, the row of i_j and the codes in LDS: the previous
                // chunk's writes, and the previous pair's reads, are done before tau = 0 goes on)
                if ((tau & 63) == 0)
                    wave_refill<DIMR>(ring, ringMask, b0, dim, Fb, tau);
                const int j = tau - lane;
                const double c = wave_cell_cost(ar, ring, ringMask, min(max(j, 0), Fb - 1), a.squared);
                const double up = shfl_up1(mineE);        // E(r-1, j) for lanes >= 1: the next step's d1
                if (lane == 0) {
                    d1 = d2 = INF;                        // above row 0 there is nothing
                    if (c0 != 0 && j >= 1 && j < Fb) {
                        d1 = bound1[j - 1];
                        d2 = bound2[j - 1];
                    }
                }
                // E(r-2, j) for the next step: the d1 of lane l - 1, lane 0's being what it read from the hand-off row
                const double nx = shfl_up1(d1);
                const bool active = rowValid && j >= 0 && j < Fb;
                if (active) {
                    double nD = r == 0 ? c : INF;         // column 0: the path starts at source frame 0, in state N
                    double eD = nD;
                    if (j > 0) {
                        double pD;
                        uint32_t code = 0;                // the two code bits ride on the cell's two comparisons
                        SSYM_PACED_PRED(pD, d1, d2, code = 1u)                         // skip
                        SSYM_PACED_STATES(nD, eD, c, pD, mineN, code |= 2u)           // rep
                        pack |= code << (2 * (j & 15));
                    }
                    if ((j & 15) == 15 || j == Fb - 1) {
                        const size_t w = (size_t)r * rowWords + ((uint32_t)j >> 4);
                        if (dirInLds)
                            dirLds[w] = pack;
                        else
                            dirG[w] = pack;
                        pack = 0;
                    }
                    if (lane == 63)
                        bound1[j] = eD;
                    if (lane == 62)
                        bound2[j] = eD;
                    if (r == Fa - 1 && j == Fb - 1)
                        result = eD;
                    mineN = nD;
                    mineE = eD;
                }
                d1 = up;
                d2 = nx;
            }
        }
        const double total = __shfl(result, (Fa - 1) & 63);
        if (lane == 0)
            a.cost[k] = total;
        if (!(total < INF)) {      // +inf or NaN: no path
            if (lane == 0)
                a.len[k] = 0;
            continue;
        }
        // the codes are read back by lane 0 as dtw_align_kernel reads its own: LDS after a barrier, the slab after a release
        // and by loads that bypass this CU's L1
        if (!dirInLds)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if (lane == 0) {
            int i = Fa - 1;
            bool wantE = true;
            for (int j = Fb - 1; j >= 1; --j) {
                rows[j] = (uint32_t)i;
                const size_t w = (size_t)i * rowWords + ((uint32_t)j >> 4);
                const uint32_t word = dirInLds ? dirLds[w] : __hip_atomic_load(dirG + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t code = (word >> (2 * (j & 15))) & 3u;
                if (wantE && (code & 2u)) {
                    wantE = false;                        // state H: (i, j-1), in state N
                } else {
                    i = max(i - ((code & 1u) ? 2 : 1), 0);      // (a finite cost's codes never lead above row 0)
                    wantE = true;
                }
            }
            rows[0] = (uint32_t)i;
        }
        __syncthreads();
        if (lane == 0)
            a.len[k] = (uint32_t)Fb;
        uint2 *path = a.path + a.pathOff[k];
        uint32_t *map = a.map ? a.map + a.mapOff[k] : nullptr;
        for (int j = lane; j < Fb; j += 64) {
            const uint32_t i = rows[j];
            path[j] = make_uint2(i, (uint32_t)j);
            if (map)
                map[j] = i;
        }
    }
}

// Spans (ssym_dtw_align_spans; DESIGN.md 2 "Spans", 5.22): a listed source is frames first[p] ... last[p] of its segment.
// The kernels are untouched: they find a source through srcOff[s] and srcOff[s + 1], so a spans call hands them a per-call
// offset table with two entries per pair -- the span's first frame and the frame after its last, both counted from the
// dictionary's first frame -- and lists pair p with source 2 p.
struct AlignSpans {
    const uint32_t *first = nullptr, *last = nullptr;     // HOST, n_pairs each; both NULL: whole segments
    explicit operator bool() const { return first != nullptr; }
};

// the span of listed pair p against its segment (s: the set's own index, SSYM_NO_MATCH stays): *none = a spot without a span
inline int32_t check_span(std::string &err, const std::string &name, const SegmentSet &src, uint32_t s, const AlignSpans &sp,
                          uint32_t p, bool *none)
{
    const uint32_t f = sp.first[p], l = sp.last[p];
    *none = f == SSYM_NO_MATCH && l == SSYM_NO_MATCH;
    if (*none || s == SSYM_NO_MATCH)
        return SSYM_OK;
    if (f == SSYM_NO_MATCH || l == SSYM_NO_MATCH || f > l || (uint64_t)l >= src.h_off[s + 1] - src.h_off[s]) {
        err = name + ": span " + std::to_string(p) + " is not first <= last < the segment's frames (or only one end is SSYM_NO_MATCH)";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

// the frames of a listed pair, (0, 0) for a pair without a source or with an empty segment; with spans (checked) the
// source's frames are the span's, and a spot without a span is a pair without a source
inline void align_shape(const SegmentSet &src, const SegmentSet &tgt, uint32_t s, uint32_t t, uint64_t *fa, uint64_t *fb,
                        const AlignSpans &sp = AlignSpans(), uint32_t p = 0)
{
    *fa = *fb = 0;
    if (s == SSYM_NO_MATCH || (sp && sp.first[p] == SSYM_NO_MATCH))
        return;
    const uint64_t a = sp ? (uint64_t)sp.last[p] - sp.first[p] + 1 : src.h_off[s + 1] - src.h_off[s];
    const uint64_t b = tgt.h_off[t + 1] - tgt.h_off[t];
    if (a == 0 || b == 0)
        return;
    *fa = a;
    *fb = b;
}

// Fa + Fb - 1 steps and Fb map entries per pair, 0 for a pair without a source or with an empty segment
inline void align_capacity(const SegmentSet &src, const SegmentSet &tgt, uint32_t s, uint32_t t, uint64_t *steps,
                           uint64_t *frames, const AlignSpans &sp = AlignSpans(), uint32_t p = 0)
{
    uint64_t fa, fb;
    align_shape(src, tgt, s, t, &fa, &fb, sp, p);
    *steps = fb ? fa + fb - 1 : 0;
    *frames = fb;
}

int32_t dtw_align(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                  const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, double *out_cost, uint32_t *out_len,
                  const uint64_t *path_offsets, uint32_t *out_path, const uint64_t *map_offsets, uint32_t *out_map,
                  uint32_t flags, uint32_t step = SSYM_STEP_SYMMETRIC, const char *fn = "ssym_dtw_align",
                  const AlignSpans &sp = AlignSpans())
{
    if (!ctx)
        return SSYM_E_INVALID;
    const std::string name(fn);
    const bool paced = step == SSYM_STEP_PACED;
    if (step != SSYM_STEP_SYMMETRIC && !paced) {
        ctx->err = name + ": step must be SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED";
        return SSYM_E_INVALID;
    }
    if (ctx->metric != SSYM_METRIC_DTW) {
        ctx->err = name + ": the context's metric is refcos, which has no alignment";
        return SSYM_E_UNSUPPORTED;
    }
    if (paced && ctx->band >= 0) {
        ctx->err = name + ": the paced step pattern bounds the slope itself and takes no Sakoe-Chiba band; use a context without one";
        return SSYM_E_UNSUPPORTED;
    }
    int32_t rc = check_pair_list(ctx->err, fn, dict, q, src_idx, tgt_idx, n_pairs, index_base);
    if (rc != SSYM_OK)
        return rc;
    if (n_pairs == 0)
        return SSYM_OK;
    if (!out_cost || !out_len || !path_offsets || !out_path || (out_map && !map_offsets)) {
        ctx->err = name + ": out_cost, out_len, path_offsets, out_path (and map_offsets with out_map) must not be NULL";
        return SSYM_E_INVALID;
    }
    if (sp && n_pairs > 0x7fffffffu) {
        ctx->err = name + ": more than 2^31 - 1 spans in one call";
        return SSYM_E_UNSUPPORTED;
    }
    const SegmentSet &src = dict->set, &tgt = q->set;
    // the pair list, the offsets against the capacities, the shape limits: all on the host, before any device work
    PairList pairs(src_idx, tgt_idx, index_base, n_pairs);
    uint64_t listedFa = 0, listedFb = 0;               // what the limits hold: every listed pair with frames
    uint64_t maxFa = 0, maxFb = 0, maxSlab = 0;        // what sizes LDS and the slabs: the pairs the kernel runs
    std::vector<uint64_t> hSpan(sp ? 2 * (size_t)n_pairs : 0);     // the kernels' source offsets of a spans call
    for (uint32_t p = 0; p < n_pairs; ++p) {
        uint64_t fa, fb;
        if (sp) {
            bool none;
            rc = check_span(ctx->err, name, src, pairs.host[p].x, sp, p, &none);
            if (rc != SSYM_OK)
                return rc;
        }
        align_shape(src, tgt, pairs.host[p].x, pairs.host[p].y, &fa, &fb, sp, p);
        if (sp) {
            // the source the kernel sees: entries 2 p and 2 p + 1 of the span table, or none
            const uint32_t s = pairs.host[p].x;
            const bool has = s != SSYM_NO_MATCH && sp.first[p] != SSYM_NO_MATCH;
            if (has) {
                hSpan[2 * (size_t)p] = src.h_off[s] + sp.first[p];
                hSpan[2 * (size_t)p + 1] = src.h_off[s] + sp.last[p] + 1;
            }
            pairs.host[p].x = has ? 2 * p : SSYM_NO_MATCH;
        }
        // a paced path has one cell per target frame
        const uint64_t steps = fb == 0 ? 0 : paced ? fb : fa + fb - 1;
        if (path_offsets[p + 1] < path_offsets[p] || path_offsets[p + 1] - path_offsets[p] < steps ||
            (out_map && (map_offsets[p + 1] < map_offsets[p] || map_offsets[p + 1] - map_offsets[p] < fb))) {
            ctx->err = name + ": offsets of pair " + std::to_string(p) + " decrease or leave less room than " +
                       (paced ? "the target's frames" : "ssym_dtw_align_sizes asks for");
            return SSYM_E_INVALID;
        }
        if (steps == 0)
            continue;
        listedFa = std::max(listedFa, fa);
        listedFb = std::max(listedFb, fb);
        // a shape without a paced path is decided before the recurrence: it takes no LDS and no slab, so it sizes none
        if (paced && (fa < (fb - 1) / 2 + 1 || fa > 2 * fb - 1))
            continue;
        maxFa = std::max(maxFa, fa);
        maxFb = std::max(maxFb, fb);
        const uint64_t dirBytes = fa * ((fb + 15) / 16) * 4;
        if (dirBytes > (uint64_t)kAlignDirLdsBytes)
            maxSlab = std::max(maxSlab, dirBytes);
    }
    if (listedFa > (uint64_t)kAlignMaxFrames || listedFb > (uint64_t)kAlignMaxFrames || src.dim > (uint32_t)kAlignMaxDim) {
        ctx->err = name + ": a listed " + (sp ? "span or target" : "segment") + " has more than " + std::to_string(kAlignMaxFrames) +
                   " frames, or frames have more than " + std::to_string(kAlignMaxDim) + " values";
        return SSYM_E_UNSUPPORTED;
    }
    if (paced && listedFb > (uint64_t)kAlignPacedMaxTargetFrames) {
        ctx->err = name + ": a listed target has more than " + std::to_string(kAlignPacedMaxTargetFrames) +
                   " frames, the limit of SSYM_STEP_PACED";
        return SSYM_E_UNSUPPORTED;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;
    const uint64_t pathTotal = path_offsets[n_pairs] - path_offsets[0];
    const uint64_t mapTotal = out_map ? map_offsets[n_pairs] - map_offsets[0] : 0;

    Blocks bl(ctx);
    AlignArgs a{};
    uint64_t *dOff = nullptr;        // path offsets, then map offsets, both rebased to the first pair's; then the span table
    rc = bl.get(&dOff, 2 * ((size_t)n_pairs + 1) + hSpan.size());
    std::vector<uint64_t> hOff(2 * ((size_t)n_pairs + 1) + hSpan.size());
    for (uint32_t p = 0; p <= n_pairs; ++p) {
        hOff[p] = path_offsets[p] - path_offsets[0];
        hOff[(size_t)n_pairs + 1 + p] = out_map ? map_offsets[p] - map_offsets[0] : 0;
    }
    std::copy(hSpan.begin(), hSpan.end(), hOff.begin() + 2 * ((size_t)n_pairs + 1));
    double *dCost = out_cost;
    uint32_t *dLen = out_len, *dPath = out_path + 2 * path_offsets[0], *dMap = out_map ? out_map + map_offsets[0] : nullptr;
    if (!outDev) {
        if (rc == SSYM_OK)
            rc = bl.get(&dCost, n_pairs);
        if (rc == SSYM_OK)
            rc = bl.get(&dLen, n_pairs);
        if (rc == SSYM_OK)
            rc = bl.get(&dPath, 2 * (size_t)pathTotal);
        if (rc == SSYM_OK && out_map)
            rc = bl.get(&dMap, (size_t)mapTotal);
    }
    const WaveGeom g = wave_geom(ctx, maxFb, src.dim, n_pairs);
    a.fbCap = g.fbCap;
    a.ringRows = g.ringRows;
    // symmetric: the code string, one byte per step; paced: the source frame of every target frame, one word each
    a.codeCap = paced ? 4 * g.fbCap : ((uint32_t)(maxFa + maxFb) + 15) & ~15u;
    a.dirLdsBytes = (uint32_t)std::min<uint64_t>((uint64_t)kAlignDirLdsBytes, (maxFa * ((maxFb + 15) / 16) * 4 + 15) & ~15ull);
    const size_t lds = (paced ? 2 : 1) * (size_t)a.fbCap * sizeof(double) + g.ringBytes + a.codeCap + a.dirLdsBytes;
    unsigned grid = g.grid;
    if (maxSlab) {
        // one slab per workgroup, as many workgroups as kAlignScratchBytes holds (128 for a 4096 x 4096 pair)
        a.slabWords = (maxSlab + 3) / 4;
        grid = (unsigned)std::min<uint64_t>(grid, std::max<uint64_t>(1, kAlignScratchBytes / (a.slabWords * 4)));
        if (rc == SSYM_OK)
            rc = bl.get(&a.slabs, (size_t)grid * a.slabWords);
    }
    if (rc == SSYM_OK)
        rc = pairs.upload(ctx, bl);
    if (rc != SSYM_OK)
        return rc;
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dOff, hOff.data(), sizeof(uint64_t) * hOff.size(), hipMemcpyHostToDevice, st));
    a.srcRaw = src.raw;
    a.srcOff = sp ? dOff + 2 * ((size_t)n_pairs + 1) : src.off;
    a.tgtRaw = tgt.raw;
    a.tgtOff = tgt.off;
    a.dim = src.dim;
    a.band = ctx->band;
    a.squared = ctx->squared;
    a.pairs = pairs.dev;
    a.nPairs = n_pairs;
    a.pathOff = dOff;
    a.mapOff = dOff + n_pairs + 1;
    a.cost = dCost;
    a.len = dLen;
    a.path = reinterpret_cast<uint2 *>(dPath);
    a.map = dMap;
    rc = paced ? wave_launch(ctx, SSYM_WAVE_KERNEL(dtw_align_paced_kernel, g.dimr), grid, lds, a)
               : wave_launch(ctx, SSYM_WAVE_KERNEL(dtw_align_kernel, g.dimr), grid, lds, a);
    if (rc != SSYM_OK)
        return rc;
    if (outDev) {
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        return SSYM_OK;
    }
    // host outputs: only what the kernel wrote reaches the caller's buffers (a pair without a path leaves its slots alone)
    std::vector<double> hCost(n_pairs);
    std::vector<uint32_t> hLen(n_pairs), hPath(2 * (size_t)pathTotal), hMap((size_t)mapTotal);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(hCost.data(), dCost, sizeof(double) * n_pairs, hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(hLen.data(), dLen, sizeof(uint32_t) * n_pairs, hipMemcpyDeviceToHost, st));
    if (pathTotal)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(hPath.data(), dPath, sizeof(uint32_t) * 2 * pathTotal, hipMemcpyDeviceToHost, st));
    if (mapTotal)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(hMap.data(), dMap, sizeof(uint32_t) * mapTotal, hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    std::copy(hCost.begin(), hCost.end(), out_cost);
    std::copy(hLen.begin(), hLen.end(), out_len);
    for (uint32_t p = 0; p < n_pairs; ++p) {
        if (hLen[p] == 0)
            continue;
        std::copy(hPath.begin() + 2 * hOff[p], hPath.begin() + 2 * (hOff[p] + hLen[p]), out_path + 2 * path_offsets[p]);
        if (out_map) {
            const uint64_t m0 = hOff[(size_t)n_pairs + 1 + p], fb = tgt.h_off[pairs.host[p].y + 1] - tgt.h_off[pairs.host[p].y];
            std::copy(hMap.begin() + m0, hMap.begin() + m0 + fb, out_map + map_offsets[p]);
        }
    }
    return SSYM_OK;
}

// ssym_dtw_align_sizes, and with spans ssym_dtw_align_spans_sizes: nothing is written before every pair is checked
int32_t dtw_align_sizes(const char *fn, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                        const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint64_t *path_offsets,
                        uint64_t *map_offsets, const AlignSpans &sp = AlignSpans())
{
    std::string err;
    int32_t rc = check_pair_list(err, fn, dict, q, src_idx, tgt_idx, n_pairs, index_base);
    if (rc != SSYM_OK)
        return rc;
    if (!path_offsets || !map_offsets)
        return SSYM_E_INVALID;
    for (uint32_t p = 0; sp && p < n_pairs; ++p) {
        bool none;
        rc = check_span(err, fn, dict->set, pair_at(src_idx, tgt_idx, index_base, p).x, sp, p, &none);
        if (rc != SSYM_OK)
            return rc;
    }
    path_offsets[0] = map_offsets[0] = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        const uint2 pr = pair_at(src_idx, tgt_idx, index_base, p);
        uint64_t steps, frames;
        align_capacity(dict->set, q->set, pr.x, pr.y, &steps, &frames, sp, p);
        path_offsets[p + 1] = path_offsets[p] + steps;
        map_offsets[p + 1] = map_offsets[p] + frames;
    }
    return SSYM_OK;
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_dtw_align_sizes(const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                             const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint64_t *path_offsets,
                             uint64_t *map_offsets)
{
    return guarded(nullptr, [&]() -> int32_t {
        return dtw_align_sizes("ssym_dtw_align", dict, q, src_idx, tgt_idx, n_pairs, index_base, path_offsets, map_offsets);
    });
}

// the two calls above with a span of source frames per pair: the same drivers, the kernels untouched (AlignSpans)
int32_t ssym_dtw_align_spans_sizes(const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                                   const uint32_t *tgt_idx, const uint32_t *span_first, const uint32_t *span_last,
                                   uint32_t n_pairs, uint32_t index_base, uint64_t *path_offsets, uint64_t *map_offsets)
{
    return guarded(nullptr, [&]() -> int32_t {
        if (n_pairs && (!span_first || !span_last))
            return SSYM_E_INVALID;
        AlignSpans sp;
        sp.first = span_first;
        sp.last = span_last;
        return dtw_align_sizes("ssym_dtw_align_spans", dict, q, src_idx, tgt_idx, n_pairs, index_base, path_offsets,
                               map_offsets, sp);
    });
}

int32_t ssym_dtw_align_spans(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                             const uint32_t *tgt_idx, const uint32_t *span_first, const uint32_t *span_last,
                             uint32_t n_pairs, uint32_t index_base, uint32_t step, double *out_cost, uint32_t *out_len,
                             const uint64_t *path_offsets, uint32_t *out_path, const uint64_t *map_offsets,
                             uint32_t *out_map, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        if (ctx && n_pairs && (!span_first || !span_last)) {
            ctx->err = "ssym_dtw_align_spans: span_first and span_last must not be NULL";
            return SSYM_E_INVALID;
        }
        AlignSpans sp;
        sp.first = span_first;
        sp.last = span_last;
        return dtw_align(ctx, dict, q, src_idx, tgt_idx, n_pairs, index_base, out_cost, out_len, path_offsets, out_path,
                         map_offsets, out_map, flags, step, "ssym_dtw_align_spans", sp);
    });
}

int32_t ssym_dtw_align(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                       const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, double *out_cost,
                       uint32_t *out_len, const uint64_t *path_offsets, uint32_t *out_path, const uint64_t *map_offsets,
                       uint32_t *out_map, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_align(ctx, dict, q, src_idx, tgt_idx, n_pairs, index_base, out_cost, out_len, path_offsets, out_path,
                         map_offsets, out_map, flags);
    });
}

// the call above with the step pattern as an argument: SSYM_STEP_SYMMETRIC is the call above itself
int32_t ssym_dtw_align_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                            const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint32_t step, double *out_cost,
                            uint32_t *out_len, const uint64_t *path_offsets, uint32_t *out_path,
                            const uint64_t *map_offsets, uint32_t *out_map, uint32_t flags)
{
    return guarded(ctx, [&]() -> int32_t {
        return dtw_align(ctx, dict, q, src_idx, tgt_idx, n_pairs, index_base, out_cost, out_len, path_offsets, out_path,
                         map_offsets, out_map, flags, step, "ssym_dtw_align_step");
    });
}

}  // extern "C"
