// dtw_mosaic_common.hpp -- what the mosaic (dtw_mosaic.hip) and the live mosaic (dtw_mosaicker.hip) share on the device: the
// limits, pos(g) and the transposed source frames (mosaic_prep_kernel), the segment of a global source frame, the local
// cost in the oracle's order, and one body each for both callers of
//   the column      mosaic_column: one column of "Mosaic" (dtw_mosaic.hip) from S to best(j) and arg(j), with the column's one
//                   barrier.  The forward kernels keep what differs: column -1, the first frame, the record of the lane.
//   the backward    MosaicColumns and mosaic_enter / mosaic_back / mosaic_word / mosaic_walk: the "backward" rule over keys
//                   (g << 1 | H, or GAP), on the offline tables (mask all ones) or the live ring (mask cap - 1).
//   the frame       mosaic_frame: (src, frame, cost) of a walked arg word.
// Every file that includes it gets its own copies (anonymous namespace).
#pragma once

#include "dtw_wave.hpp"
#include "dtw_cover_chain.hpp"

namespace ssym {

// Limits of the mosaic (soundsym_amd.h)
constexpr uint32_t kMosaicMaxDim = 64;
constexpr uint64_t kMosaicScratchBytes = 512ull << 20;
constexpr uint32_t kMosaicThreads = 1024;
constexpr uint32_t kMosaicMaxWaves = kMosaicThreads / 64;
constexpr uint32_t kMosaicStart = 0x80000000u;            // arg row, after the walk: a piece starts at this column

namespace {

// the segment of global source frame g: the last s with off[s] <= g (empty segments are passed over)
__device__ __forceinline__ uint32_t mosaic_segment(const uint64_t *off, uint32_t n, uint64_t g)
{
    uint32_t lo = 0, hi = n;     // off[lo] <= g < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void mosaic_prep_kernel(const uint64_t *__restrict__ off, uint32_t n, uint32_t G,
                                                          const double *__restrict__ raw, uint32_t dim,
                                                          uint8_t *__restrict__ posc, double *__restrict__ srcT)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G)
        return;
    const uint64_t pos = g - off[mosaic_segment(off, n, g)];
    posc[g] = (uint8_t)(pos < 2 ? pos : 2);
    for (uint32_t k = 0; k < dim; ++k)
        srcT[(size_t)k * G + g] = raw[g * dim + k];
}

// c: sum_k (a_k - b_k)^2, k ascending, sub / mul / add rounded separately (the oracle's order, wave_cell_cost's bits), then
// the square root unless squared
__device__ __forceinline__ double mosaic_cost(const double *ar, size_t stride, const double *br, uint32_t dim, int squared)
{
    double acc = 0.0;
#pragma unroll 4
    for (uint32_t k = 0; k < dim; ++k) {
        const double df = __dsub_rn(ar[k * stride], br[k]);
        acc = __dadd_rn(acc, __dmul_rn(df, df));
    }
    return squared ? acc : sqrt(acc);
}

// what a column needs beside the column itself; the same for every column of a launch but for the slab
struct MosaicCore {
    uint32_t G, dim;             // source frames of the whole dictionary, values per frame
    int squared;
    double penalty, gapCost;
    const uint8_t *posc;         // [G] min(pos(g), 2)
    const double *srcT;          // [dim][G] the source frames, transposed
    double *slab;                // E / N of the two column parities, 4 G doubles per workgroup
};

// The columns of a walk: the direction bytes and arg(j) of the offline tables (mask all ones) or of the live ring (mask
// cap - 1), column j at j & mask.  The forward pass writes them, the backward rule reads them.
struct MosaicColumns {
    uint8_t *dir;                // [columns][G] direction bytes: bit 0 H < N; bits 1-2: 0 diagonal, 1 skip, 2 open
    uint32_t *arg;               // [columns] arg(j); after the walk g | kMosaicStart, or GAP
    uint32_t G;
    uint64_t mask;

    __device__ __forceinline__ uint8_t *column(long long j) const { return dir + ((uint64_t)j & mask) * G; }
    __device__ __forceinline__ uint32_t byte(long long j, uint32_t g) const { return column(j)[g]; }
    __device__ __forceinline__ uint32_t &word(long long j) const { return arg[(uint64_t)j & mask]; }
};

// Column j of the workgroup whose slab k.slab is: E / N of column j - 1 at parity (j - 1) & 1 and target frame j in
// ring[j & 1] -> E / N of column j, the direction bytes and arg(j) (thread 0 stores it) in cols, and best(j), returned in
// every thread.  best: best(j - 1).  stageNext(ring row) stages target frame j + 1; the column's ONE barrier orders it with the
// slab and the waves' pairs (all double-buffered by the column's parity).
template <class Stage>
__device__ __forceinline__ double mosaic_column(const MosaicCore &k, const MosaicColumns &cols, uint64_t j, double best,
                                                double (*ring)[kMosaicMaxDim], double (*partV)[kMosaicMaxWaves],
                                                uint32_t (*partG)[kMosaicMaxWaves], Stage stageNext)
{
    const double INF = __builtin_inf();
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, nWaves = nthr >> 6, G = k.G;
    const uint32_t par = (uint32_t)j & 1;
    const double S = __dadd_rn(k.penalty, best);
    const double *Eo = k.slab + (size_t)(par ^ 1) * 2 * G, *No = Eo + G;
    double *En = k.slab + (size_t)par * 2 * G, *Nn = En + G;
    uint8_t *dcol = cols.column((long long)j);
    double bv = INF;
    uint32_t bg = kCoverNone;
    for (uint32_t g = tid; g < G; g += nthr) {
        const uint32_t pc = k.posc[g];
        const double nOld = No[g];
        // dtw_wave.hpp's paced cell, with the new piece (S) between its two halves; a segment's first frames have no rows above
        double P = INF, nD, eD;
        uint32_t code = 0;
        bool rep = false;
        if (pc >= 1)
            P = Eo[g - 1];
        if (pc >= 2) {
            const double e1 = P, e2 = Eo[g - 2];
            SSYM_PACED_PRED(P, e1, e2, code = 1)
        }
        if (!(P <= S)) {
            P = S;
            code = 2;
        }
        const double c = mosaic_cost(k.srcT + g, G, ring[par], k.dim, k.squared);
        SSYM_PACED_STATES(nD, eD, c, P, nOld, rep = true)
        En[g] = eD;
        Nn[g] = nD;
        dcol[g] = (uint8_t)(code << 1 | (rep ? 1u : 0u));
        if (eD < bv) {                                       // g ascends within a thread: the first minimum stays
            bv = eD;
            bg = g;
        }
    }
    stageNext(ring[par ^ 1]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oV = __shfl_xor(bv, m);
        const uint32_t oG = (uint32_t)__shfl_xor((int)bg, m);
        if (oV < bv || (oV == bv && oG < bg)) {
            bv = oV;
            bg = oG;
        }
    }
    if ((tid & 63) == 0) {
        partV[par][wave] = bv;
        partG[par][wave] = bg;
    }
    __syncthreads();
    double v = INF;
    uint32_t arg = kCoverNone;
    for (uint32_t w = 0; w < nWaves; ++w) {
        const double oV = partV[par][w];
        const uint32_t oG = partG[par][w];
        if (oV < v || (oV == v && oG < arg)) {
            v = oV;
            arg = oG;
        }
    }
    const double vg = __dadd_rn(k.gapCost, best);
    if (vg < v) {
        v = vg;
        arg = kCoverGap;
    }
    if (tid == 0)
        cols.word((long long)j) = arg;
    return v;
}

// "Mosaic: backward", once.  A position of the walk at column j is a key: g << 1 | (1: state H), or GAP.  Whatever the bytes
// hold, a key's g stays below G: a g at or past G reads as GAP.  A walk carries the direction byte of its cell beside the key
// (MosaicPos), so that a step back costs it one load, the byte of the cell it enters.
struct MosaicPos {
    uint32_t key;
    uint32_t d;                  // the direction byte of (g, j); 0 for GAP
};

// the position of `key` at column j
__device__ __forceinline__ MosaicPos mosaic_pos(const MosaicColumns &v, uint32_t key, long long j)
{
    return MosaicPos{key, key == kCoverGap ? 0u : v.byte(j, key >> 1)};
}

// the position of a walk that enters column j at g, in g's E state
__device__ __forceinline__ MosaicPos mosaic_enter(const MosaicColumns &v, uint32_t g, long long j)
{
    if (g >= v.G)
        return MosaicPos{kCoverGap, 0u};
    const uint32_t d = v.byte(j, g);
    return MosaicPos{g << 1 | (d & 1u), d};
}

// the position at column j - 1 of the walk that is at p in column j; arg(j - 1) must still be the forward pass's.  (One
// load site and few branches: a walk is one thread's chain of dependent steps, and every instruction of a step shows.)
__device__ __forceinline__ MosaicPos mosaic_back(const MosaicColumns &v, MosaicPos p, long long j)
{
    const uint32_t g = p.key >> 1, code = p.d >> 1;
    const bool gap = p.key == kCoverGap, repeat = !gap && (p.key & 1);   // state H: the cell before is (g, j-1) in state N
    uint32_t to = repeat ? g : g > code ? g - 1 - code : 0;
    if (gap || (!repeat && code >= 2))                       // a gap frame, or a piece starts here: on from arg(j - 1)
        to = v.word(j - 1);
    if (to >= v.G)
        return MosaicPos{kCoverGap, 0u};
    const uint32_t d = v.byte(j - 1, to);
    return MosaicPos{to << 1 | (repeat ? 0u : d & 1u), d};
}

// what the walk leaves in the arg row for p at column j: g, with the start bit where a piece starts, or GAP
__device__ __forceinline__ uint32_t mosaic_word(MosaicPos p, long long j)
{
    if (p.key == kCoverGap)
        return kCoverGap;
    const bool start = !(p.key & 1) && ((p.d >> 1) >= 2 || j == 0);
    return (p.key >> 1) | (start ? kMosaicStart : 0u);
}

// one thread walks from p at column top down to column floor + 1 and leaves the words in the arg row
__device__ __forceinline__ void mosaic_walk(const MosaicColumns &v, MosaicPos p, long long top, long long floor)
{
    for (long long col = top; col > floor; --col) {
        const uint32_t word = mosaic_word(p, col);
        if (col - 1 > floor)
            p = mosaic_back(v, p, col);                      // reads arg(col - 1) before it is walked
        v.word(col) = word;
    }
}

// (src, frame, cost) of target frame x [dim] from its walked arg word: dtw_mosaic's per-frame outputs
struct MosaicFrame {
    uint32_t src, frame;
    double cost;
};

__device__ __forceinline__ MosaicFrame mosaic_frame(uint32_t word, const double *srcRaw, const uint64_t *srcOff, uint32_t nSrc,
                                                    const MosaicCore &k, const double *x)
{
    if (word == kCoverGap)
        return MosaicFrame{kCoverGap, kCoverNone, k.gapCost};
    const uint32_t g = min(word & ~kMosaicStart, k.G - 1);
    const uint32_t src = mosaic_segment(srcOff, nSrc, g);
    return MosaicFrame{src, (uint32_t)(g - srcOff[src]), mosaic_cost(srcRaw + (size_t)g * k.dim, 1, x, k.dim, k.squared)};
}

}  // namespace
}  // namespace ssym
