// dtw_wave.hpp -- the anti-diagonal wavefront forward pass dtw_align.hip and dtw_spot.hip share (and the lane - 1 move
// and ring stride dtw_exact.hip shares with them), each piece written once, plus the host side their drivers and
// dtw_spotter.hip's share: launch geometry, the pair-list checks and upload, and the spot family's refusals, LDS size and
// output rule.  What is here is what must not differ between the kernels, the paced pattern's cell included
// (SSYM_PACED_PRED, SSYM_PACED_STATES: one text for the six kernels that run it).
// Each kernel keeps its own step loop: the symmetric spot cell and its loop stand twice, in dtw_spot_kernel and
// dtw_watch_kernel, because one shared loop was measured slower than either kernel's own on some shape.
// (dtw_align_kernel still carries the text of wave_load_frame and wave_refill in its body, for the reason given there:
// change them together.)
//
// The pass: one wave per pair, grid-stride over the list.  Lane l owns source row c0 + l of a 64-row chunk and works on
// target column j = tau - l at step tau.  D(i-1, j) comes from lane l - 1 by a DPP move, D(i-1, j-1) is what came one step
// earlier, D(i, j-1) is the lane's own previous value.  The lane's source frame sits in registers (wave_load_frame);
// target frames pass through an LDS ring of 128 frames refilled 64 at a time (wave_refill: at step tau the lanes read
// columns tau - 63 ... tau), so the LDS a pair needs does not grow with the target.  A chunk's bottom row is handed to
// the next chunk through ONE LDS row overwritten in place: lane 63 writes column tau - 63 while lane 0 reads columns tau
// and tau - 1 (the kernels' own code: what the row carries differs).  Frames are zero-padded to DIMR = 14 / 16 / 40 / 64.
//
// Arithmetic: D is formed exactly as dtw_exact.hip forms it (f64, k ascending, sub / mul / add rounded separately, the
// square root rounded separately, c + min3 with min3's comparisons in the same order), so a cost has the bits
// ssym_pair_matrix(exact = 1) returns.  The predecessor rule compares those exact values:
//   dg = D(i-1,j-1), up = D(i-1,j), lf = D(i,j-1):  diagonal if dg <= up && dg <= lf, else up if up <= lf, else left.
#pragma once
#include "ssym_internal.hpp"

#include <algorithm>
#include <initializer_list>
#include <utility>

namespace ssym {

constexpr int kWaveRing = 128;              // target frames resident in LDS (two blocks of 64)

// ---- device -------------------------------------------------------------------------------------------------------------

// value of lane - 1 (lane 0 keeps its own): one DPP move per half (wave_shr:1, gfx9 encoding 0x138)
// instead of a ds_bpermute round trip through the LDS crossbar -- the shuffle sits on the critical
// path of every anti-diagonal step
__device__ __forceinline__ int shfl_up1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ double shfl_up1(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// LDS row stride of f64 frames padded to dimr values: 2 (mod 4) doubles, so rows are 16-byte aligned and 128-bit reads
// by consecutive lanes tile the banks
constexpr int wave_ld(int dimr) { return dimr % 4 == 2 ? dimr : dimr + 2; }

// the lane's source frame into registers, zero-padded
template <int DIMR>
__device__ __forceinline__ void wave_load_frame(double (&ar)[DIMR], const double *arow, int dim)
{
#pragma unroll
    for (int e = 0; e < DIMR; ++e)
        ar[e] = e < dim ? arow[e] : 0.0;
}

// the 64 target frames from column f0 on enter the ring, zero-padded; the block they replace ended at column f0 - 65,
// and the lanes still read from column f0 - 63 on.  Every lane of the wave calls it.
template <int DIMR>
__device__ __forceinline__ void wave_refill(double *ring, uint32_t ringMask, const double *b0, int dim, int Fb, int f0)
{
    const int cnt = min(64, Fb - f0);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * DIMR; i += 64) {
        const int fr = i / DIMR, e = i % DIMR;
        ring[(size_t)((uint32_t)(f0 + fr) & ringMask) * wave_ld(DIMR) + e] = e < dim ? b0[(size_t)(f0 + fr) * dim + e] : 0.0;
    }
    __syncthreads();
}

// c(i, jc): sum_k (a_k - b_k)^2, k ascending, sub / mul / add rounded separately (the oracle's order), then the square
// root unless squared; the zero padding adds +0.0 to a non-negative sum and leaves its bits alone
template <int DIMR>
__device__ __forceinline__ double wave_cell_cost(const double (&ar)[DIMR], const double *ring, uint32_t ringMask, int jc,
                                                 int squared)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2 *bp = reinterpret_cast<const d2 *>(ring + (size_t)((uint32_t)jc & ringMask) * wave_ld(DIMR));
    double acc = 0.0;
#pragma unroll
    for (int e0 = 0; e0 < DIMR; e0 += 8) {
        d2 bv[4];
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (e0 + 2 * v < DIMR)
                bv[v] = bp[e0 / 2 + v];
#pragma unroll
        for (int v = 0; v < 8; ++v)
            if (e0 + v < DIMR) {
                const double df = __dsub_rn(ar[e0 + v], bv[v / 2][v % 2]);
                acc = __dadd_rn(acc, __dmul_rn(df, df));
            }
    }
    return squared ? acc : sqrt(acc);
}

// min3 in dtw_exact.hip's comparison order
__device__ __forceinline__ double wave_min3(double up, double lf, double dg)
{
    double best = up;                 // D(i-1, j)
    if (lf < best) best = lf;         // D(i,   j-1)
    if (dg < best) best = dg;         // D(i-1, j-1)
    return best;
}

// the predecessor rule: ties prefer the diagonal, then the source step.  0 = diagonal, 1 = up, 2 = left
__device__ __forceinline__ uint32_t wave_pred(double up, double lf, double dg)
{
    return (dg <= up && dg <= lf) ? 0u : (up <= lf ? 1u : 2u);
}

// The paced step pattern's cell, once, for the six kernels that run it: dtw_paced_kernel,
// dtw_watch_paced_kernel, dtw_align_paced_kernel, dtw_match_paced_kernel, cover_forward_kernel and mosaic_column.  Two
// pieces, because the mosaic puts a third candidate (a new piece) between them.  What rides on a comparison (a start
// word, a code bit, a flag) is a statement the caller hands in, run where the comparison holds; (void)0 where nothing does.
// Macros, because as functions that hand the comparisons back as flags the cell changes what the kernels compile to:
// dtw_paced_kernel keeps its instruction count and registers, holds the second comparison in another SGPR pair and runs
// 1 % slower on two of three workloads.  In this shape all six compile to the instructions they had with
// their own copies.
// The predecessor: P = d1 = E(i-1, j-1), replaced by d2 = E(i-2, j-1) if that is < d1 (strict: a tie keeps row i - 1, and so
// does a NaN on either side); ON_SKIP runs where P came from row i - 2
#define SSYM_PACED_PRED(P, d1, d2, ON_SKIP)                                                                               \
    P = (d1);                                                                                                             \
    if ((d2) < P) {                                                                                                       \
        P = (d2);                                                                                                         \
        ON_SKIP;                                                                                                          \
    }
// The states: N = c + P, H = c + nPrev (nPrev = N(i, j-1)), each sum rounded once; E = N, replaced by H if that is < N
// (strict: a tie keeps N); ON_REP runs where E is H, the source frame repeated
#define SSYM_PACED_STATES(N, E, c, P, nPrev, ON_REP)                                                                      \
    N = __dadd_rn(c, P);                                                                                                  \
    {                                                                                                                     \
        const double h_ = __dadd_rn(c, nPrev);                                                                            \
        E = N;                                                                                                            \
        if (h_ < N) {                                                                                                     \
            E = h_;                                                                                                       \
            ON_REP;                                                                                                       \
        }                                                                                                                 \
    }

// the first minimum among the 64 lanes' candidates (bestD f64, bestEnd u32, bestSt u32), ordered by (D, row), in every
// lane; a lane without a candidate holds (+inf, 0xffffffff), which loses against every candidate and ties with its like.
// One text for the spot kernels' end reduction, the selection passes and the spotter, as a macro: the same lines as a function cost
// dtw_spot_kernel<64> 18 spilled VGPRs and dtw_spot_kernel<14> one more register
#define SSYM_SPOT_FIRST_MIN(bestD, bestEnd, bestSt)                                                                       \
    _Pragma("unroll") for (int m_ = 32; m_ >= 1; m_ >>= 1)                                                                \
    {                                                                                                                     \
        const double oD_ = __shfl_xor(bestD, m_);                                                                         \
        const uint32_t oE_ = (uint32_t)__shfl_xor((int)bestEnd, m_), oS_ = (uint32_t)__shfl_xor((int)bestSt, m_);         \
        if (oD_ < bestD || (oD_ == bestD && oE_ < bestEnd)) {                                                             \
            bestD = oD_;                                                                                                  \
            bestEnd = oE_;                                                                                                \
            bestSt = oS_;                                                                                                 \
        }                                                                                                                 \
    }

// ---- host: launch geometry ----------------------------------------------------------------------------------------------

inline int wave_dimr(uint32_t dim) { return dim <= 14 ? 14 : dim <= 16 ? 16 : dim <= 40 ? 40 : 64; }
// entries of the hand-off row: even (what follows it in LDS stays 16-byte aligned), >= the longest listed target
inline uint32_t wave_fb_cap(uint64_t maxFb) { return ((uint32_t)std::max<uint64_t>(maxFb, 1) + 1) & ~1u; }
inline uint32_t wave_ring_rows(uint64_t maxFb) { return maxFb <= 64 ? 64 : kWaveRing; }
inline size_t wave_ring_bytes(uint32_t ringRows, int dimr) { return (size_t)ringRows * wave_ld(dimr) * sizeof(double); }

// what every launch of the wavefront derives from (context, longest listed target, dim, pairs).  The caller adds its own
// LDS terms to ringBytes: dtw_align the code row and the direction matrix, the spot family spot_lds_bytes' hand-off rows
struct WaveGeom {
    uint32_t fbCap, ringRows;
    int dimr;
    size_t ringBytes;
    unsigned grid;               // one wave per pair, 8 x CUs at most
};
inline WaveGeom wave_geom(const ssym_ctx *ctx, uint64_t maxFb, uint32_t dim, uint64_t n_pairs)
{
    WaveGeom g;
    g.fbCap = wave_fb_cap(maxFb);
    g.ringRows = wave_ring_rows(maxFb);
    g.dimr = wave_dimr(dim);
    g.ringBytes = wave_ring_bytes(g.ringRows, g.dimr);
    g.grid = (unsigned)std::min<uint64_t>(n_pairs, (uint64_t)ctx->num_cus * 8);
    return g;
}

// the instantiation of kernel template K_ (one wave per workgroup, one argument struct) for wave_dimr's value; what
// follows dimr_ goes behind DIMR in the template's argument list (", ##__VA_ARGS__" is the GNU extension that drops the
// comma when nothing follows; hipcc is clang and takes it, C++17 has no __VA_OPT__)
#define SSYM_WAVE_KERNEL(K_, dimr_, ...)                                                                                  \
    ((dimr_) == 14   ? K_<14, ##__VA_ARGS__>                                                                              \
     : (dimr_) == 16 ? K_<16, ##__VA_ARGS__>                                                                              \
     : (dimr_) == 40 ? K_<40, ##__VA_ARGS__>                                                                              \
                     : K_<64, ##__VA_ARGS__>)

template <class Args>
inline int32_t wave_launch(ssym_ctx *ctx, void (*kern)(Args), unsigned grid, size_t lds, const Args &a)
{
    if (lds > 64 * 1024)
        SSYM_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<grid, 64, lds, ctx->stream>>>(a);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

// ---- host: argument checks (fn: the entry point's name, err: where the message goes) -----------------------------------

inline int32_t check_handles(std::string &err, const char *fn, const ssym_dict *dict, const ssym_queries *q)
{
    if (!dict || !q) {
        err = std::string(fn) + ": dictionary or queries handle is NULL";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

// what a call with something to do needs of its two sets
inline int32_t check_sets(std::string &err, const SegmentSet &src, const SegmentSet &tgt)
{
    if (src.n == 0) {
        err = "empty dictionary";
        return SSYM_E_EMPTY_DICT;
    }
    if (src.dim != tgt.dim) {
        err = "dim mismatch between dictionary and targets";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

// a (src_idx, tgt_idx, n_pairs, index_base) list against a dictionary and a query set.  An empty list is fine whatever
// else holds: the caller returns after it.
inline int32_t check_pair_list(std::string &err, const char *fn, const ssym_dict *dict, const ssym_queries *q,
                               const uint32_t *src_idx, const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base)
{
    int32_t rc = check_handles(err, fn, dict, q);
    if (rc != SSYM_OK || n_pairs == 0)
        return rc;
    const std::string name(fn);
    if (!src_idx) {
        err = name + ": src_idx is NULL";
        return SSYM_E_INVALID;
    }
    rc = check_sets(err, dict->set, q->set);
    if (rc != SSYM_OK)
        return rc;
    if (!tgt_idx && n_pairs > q->set.n) {
        err = name + ": tgt_idx is NULL and n_pairs exceeds the number of targets";
        return SSYM_E_INVALID;
    }
    for (uint32_t p = 0; p < n_pairs; ++p) {
        if (src_idx[p] != SSYM_NO_MATCH && (src_idx[p] < index_base || src_idx[p] - index_base >= dict->set.n)) {
            err = name + ": src_idx[" + std::to_string(p) + "] is outside the dictionary";
            return SSYM_E_INVALID;
        }
        if (tgt_idx && tgt_idx[p] >= q->set.n) {
            err = name + ": tgt_idx[" + std::to_string(p) + "] is outside the targets";
            return SSYM_E_INVALID;
        }
    }
    return SSYM_OK;
}

// entry p of a checked list as (source, target) in the sets' own indices; SSYM_NO_MATCH stays
inline uint2 pair_at(const uint32_t *src_idx, const uint32_t *tgt_idx, uint32_t index_base, uint32_t p)
{
    return make_uint2(src_idx[p] == SSYM_NO_MATCH ? SSYM_NO_MATCH : src_idx[p] - index_base, tgt_idx ? tgt_idx[p] : p);
}

// a checked list as the kernels read it: on the host from the start, in a block of bl once upload has enqueued the copy
// on ctx's stream (the list outlives the call's synchronisation)
struct PairList {
    std::vector<uint2> host;
    uint2 *dev = nullptr;
    PairList(const uint32_t *src_idx, const uint32_t *tgt_idx, uint32_t index_base, uint32_t n_pairs) : host(n_pairs)
    {
        for (uint32_t p = 0; p < n_pairs; ++p)
            host[p] = pair_at(src_idx, tgt_idx, index_base, p);
    }
    int32_t upload(ssym_ctx *ctx, Blocks &bl)
    {
        const int32_t rc = bl.get(&dev, host.size());
        if (rc != SSYM_OK)
            return rc;
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dev, host.data(), sizeof(uint2) * host.size(), hipMemcpyHostToDevice, ctx->stream));
        return SSYM_OK;
    }
};

// ---- host: the spot family (dtw_spot.hip, dtw_spotter.hip) --------------------------------------------------------------

// what spotting refuses of a context
inline int32_t check_spot_ctx(ssym_ctx *ctx, const char *fn)
{
    if (ctx->metric != SSYM_METRIC_DTW) {
        ctx->err = std::string(fn) + ": the context's metric is refcos, which has no alignment to spot";
        return SSYM_E_UNSUPPORTED;
    }
    if (ctx->band >= 0) {
        ctx->err = std::string(fn) + ": a Sakoe-Chiba band has no meaning with a free start; use a context without one";
        return SSYM_E_UNSUPPORTED;
    }
    return SSYM_OK;
}

// ... and of the shapes: the longest target that will run against the caller's limit for its step pattern, values per frame
inline int32_t check_spot_limits(ssym_ctx *ctx, const char *fn, uint64_t maxFb, uint32_t dim, uint64_t maxFrames,
                                 uint32_t maxDim)
{
    if (maxFb > maxFrames || dim > maxDim) {
        ctx->err = std::string(fn) + ": a target has more than " + std::to_string(maxFrames) +
                   " frames, or frames have more than " + std::to_string(maxDim) + " values";
        return SSYM_E_UNSUPPORTED;
    }
    return SSYM_OK;
}

// dynamic LDS of a launch: the hand-off rows (12 bytes per target frame each: one row, at most 48 KiB, or the paced
// pattern's two, at most 48 KiB as well) + the ring (at most 66 KiB)
inline size_t spot_lds_bytes(const WaveGeom &g, uint32_t step)
{
    const size_t rows = step == SSYM_STEP_PACED ? 2 : 1;
    return rows * g.fbCap * (sizeof(double) + sizeof(uint32_t)) + g.ringBytes;
}

// The output rule of the calls that give several arrays of f64 and of u32 (the spot drivers, dtw_cover.hip, dtw_mosaic.hip).
// Host outputs: the kernel writes device scratch (alloc) -- the f64 arrays packed into ONE block in the order given, the u32
// arrays into another; an output that is NULL has scratch like any other -- and finish enqueues one copy back of each block,
// synchronises and hands the values to the caller's arrays that are not NULL.  SSYM_OUT_DEVICE: the kernel writes the
// caller's arrays in place (a NULL is handed through as it is) and finish only synchronises.  Either way: the call's one
// synchronisation.
template <class T>
struct OutBlock {
    struct Part {
        T *out;                  // the caller's array
        size_t n;
        T *dev;                  // where the kernel writes
    };
    std::vector<Part> parts;
    size_t total = 0;

    OutBlock(std::initializer_list<std::pair<T *, size_t>> list)
    {
        for (const auto &a : list) {
            parts.push_back(Part{a.first, a.second, a.first});
            total += a.second;
        }
    }
    T *operator[](size_t i) const { return parts[i].dev; }
    int32_t alloc(Blocks &bl)
    {
        T *block = nullptr;
        const int32_t rc = bl.get(&block, total);
        for (Part &p : parts) {
            p.dev = block;
            block += p.n;
        }
        return rc;
    }
    void hand_over(const T *from) const
    {
        for (const Part &p : parts) {
            if (p.out)
                std::copy(from, from + p.n, p.out);
            from += p.n;
        }
    }
};

struct StagedOut {
    bool inPlace;
    OutBlock<double> f64;
    OutBlock<uint32_t> u32;

    StagedOut(uint32_t flags, std::initializer_list<std::pair<double *, size_t>> f, std::initializer_list<std::pair<uint32_t *, size_t>> u)
        : inPlace((flags & SSYM_OUT_DEVICE) != 0), f64(f), u32(u)
    {
    }
    int32_t alloc(Blocks &bl)
    {
        if (inPlace)
            return SSYM_OK;
        const int32_t rc = f64.alloc(bl);
        return rc == SSYM_OK ? u32.alloc(bl) : rc;
    }
    int32_t finish(ssym_ctx *ctx)
    {
        if (inPlace) {
            SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            return SSYM_OK;
        }
        std::vector<double> hF64(f64.total);
        std::vector<uint32_t> hU32(u32.total);
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(hF64.data(), f64[0], sizeof(double) * f64.total, hipMemcpyDeviceToHost, ctx->stream));
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(hU32.data(), u32[0], sizeof(uint32_t) * u32.total, hipMemcpyDeviceToHost, ctx->stream));
        SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        f64.hand_over(hF64.data());
        u32.hand_over(hU32.data());
        return SSYM_OK;
    }
};

}  // namespace ssym
