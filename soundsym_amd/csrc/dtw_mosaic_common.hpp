// dtw_mosaic_common.hpp -- what the mosaic (dtw_mosaic.hip) and the live mosaic (dtw_mosaicker.hip) share on the device: the
// limits, pos(g) and the transposed source frames (mosaic_prep_kernel), the segment of a global source frame and the local
// cost in the oracle's order.  Every file that includes it gets its own copies (anonymous namespace).
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

}  // namespace
}  // namespace ssym
