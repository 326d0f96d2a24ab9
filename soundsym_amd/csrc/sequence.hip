// sequence.hip -- SoundSequence::new's distances (src/sound.rs:392-398) on the device: the mean MFCC of every sound
// (analyze_mean_mfccs, :271-286) and cosine_sim_angular (:59-69) between each pair of neighbours.
//
// Definitions (every product and sum rounded separately: __dmul_rn / __dadd_rn, and the library builds with
// -ffp-contract=off):
//   mean     per coefficient j: acc = +0.0; for t in the sound's frames, ascending: acc = acc + f[t][j]; then acc / T.
//            T = 0 gives 0 / 0 = NaN.  The same fold as api.Sound.mean_mfccs() and ssym_mfcc's host out_mean.
//   norm     sum of x*x as the sequential fold `item * item + memo` from 0 (src/sound.rs:35-38): NO sqrt
//   dot      rulinalg 0.4.2's eight-way dot: p_i = p_i + x[8b+i] y[8b+i] over whole blocks of eight, the eight
//            partials combined by SSYM_RULINALG_STEP (include/ssym_rulinalg.h, the one place the association lives),
//            then the dim % 8 tail one product at a time
//   sim      dot / (norm(me) * norm(you))                                          (cosine_sim, src/sound.rs:22-33)
//   clamp    sim > 1 -> 1, sim < -1 -> 1 (not -1: the reference's own bug, :63-67), else sim; NaN passes through
//   distance acos(clamped) * FRAC_1_PI, a multiplication by 0.3183098861837907 (not a division by pi)
//
// Mapping: the means are one thread per (sound, coefficient), each a sequential fold over the sound's frames -- that
// is what makes them bit-exact, and it makes one very long sound a serial chain of adds (fine at the reference's
// sizes).  The distances are one thread per neighbour pair.  No atomics.
#include "ssym_internal.hpp"
#include "ssym_rulinalg.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace ssym {
namespace {

constexpr int kThreads = 256;
constexpr double kFrac1Pi = 0.3183098861837907;    // f64::consts::FRAC_1_PI

__global__ __launch_bounds__(kThreads) void frame_means_kernel(const double *__restrict__ feats,
                                                               const uint64_t *__restrict__ off, uint32_t n,
                                                               uint32_t dim, double *__restrict__ mean)
{
    const uint64_t total = (uint64_t)n * dim;
    const uint64_t f0 = off[0];
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t s = i / dim, j = i % dim;
        const uint64_t a = off[s] - f0, b = off[s + 1] - f0;
        double acc = 0.0;
        for (uint64_t t = a; t < b; ++t)
            acc = __dadd_rn(acc, feats[t * dim + j]);
        mean[i] = __ddiv_rn(acc, (double)(b - a));
    }
}

__global__ __launch_bounds__(kThreads) void neighbour_distances_kernel(const double *__restrict__ mean, uint32_t nPairs,
                                                                       uint32_t dim, double *__restrict__ sim,
                                                                       double *__restrict__ dist)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nPairs)
        return;
    const double *me = mean + (size_t)i * dim, *you = me + dim;
    double nm = 0.0, ny = 0.0;
    for (uint32_t k = 0; k < dim; ++k) {
        nm = __dadd_rn(__dmul_rn(me[k], me[k]), nm);
        ny = __dadd_rn(__dmul_rn(you[k], you[k]), ny);
    }
    double p[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t k = 0;
    for (; k + 8 <= dim; k += 8)
#pragma unroll
        for (int q = 0; q < 8; ++q)
            p[q] = __dadd_rn(p[q], __dmul_rn(me[k + q], you[k + q]));
    double dot = 0.0;
    dot = SSYM_RULINALG_STEP(__dadd_rn, dot, p[0], p[4]);
    dot = SSYM_RULINALG_STEP(__dadd_rn, dot, p[1], p[5]);
    dot = SSYM_RULINALG_STEP(__dadd_rn, dot, p[2], p[6]);
    dot = SSYM_RULINALG_STEP(__dadd_rn, dot, p[3], p[7]);
    for (; k < dim; ++k)
        dot = __dadd_rn(dot, __dmul_rn(me[k], you[k]));
    const double s = __ddiv_rn(dot, __dmul_rn(nm, ny));
    const double c = s > 1.0 ? 1.0 : (s < -1.0 ? 1.0 : s);
    sim[i] = c;
    dist[i] = __dmul_rn(acos(c), kFrac1Pi);
}

#define SSYM_SEQ_TRY(expr)                     \
    do {                                       \
        const int32_t rc__ = (expr);           \
        if (rc__ != SSYM_OK)                   \
            return rc__;                       \
    } while (0)

int32_t sequence_distances(ssym_ctx *ctx, const double *feats, const uint64_t *off, uint32_t n, uint32_t dim,
                           uint32_t flags, double *outMean, double *outSim, double *outDist)
{
    const char *fn = "ssym_sequence_distances";
    if (!ctx)
        return SSYM_E_INVALID;
    if (dim == 0 || dim > 64) {
        ctx->err = std::string(fn) + ": need 1 <= dim <= 64";
        return SSYM_E_INVALID;
    }
    if (n == 0)
        return SSYM_OK;
    if (!off) {
        ctx->err = std::string(fn) + ": NULL frame_offsets";
        return SSYM_E_INVALID;
    }
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) {
            ctx->err = std::string(fn) + ": frame_offsets must not decrease";
            return SSYM_E_INVALID;
        }
    const uint64_t F = off[n] - off[0];
    if (F && !feats) {
        ctx->err = std::string(fn) + ": NULL feats";
        return SSYM_E_INVALID;
    }
    const uint32_t nPairs = n - 1;
    if (!outMean && !(nPairs && (outSim || outDist)))
        return SSYM_OK;
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool inDev = (flags & SSYM_OUT_DEVICE) != 0;

    Blocks bl(ctx);
    const double *dF = nullptr;
    double *dMean = nullptr, *dRes = nullptr;
    uint64_t *dOff = nullptr;
    SSYM_SEQ_TRY(bl.get(&dOff, (size_t)n + 1));
    SSYM_SEQ_TRY(bl.get(&dMean, (size_t)n * dim));
    SSYM_SEQ_TRY(bl.get(&dRes, 2 * (size_t)nPairs));       // sim, then distance
    if (inDev) {
        dF = feats + off[0] * dim;
    } else {
        double *d = nullptr;
        SSYM_SEQ_TRY(bl.get(&d, F * dim));
        if (F)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(d, feats + off[0] * dim, F * dim * sizeof(double),
                                               hipMemcpyHostToDevice, st));
        dF = d;
    }
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dOff, off, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SSYM_SEQ_TRY(launch_frame_means(ctx, dF, dOff, n, dim, dMean));
    if (nPairs) {
        neighbour_distances_kernel<<<(nPairs + kThreads - 1) / kThreads, kThreads, 0, st>>>(dMean, nPairs, dim, dRes,
                                                                                           dRes + nPairs);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    std::vector<double> host((size_t)n * dim + 2 * (size_t)nPairs);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(host.data(), dMean, (size_t)n * dim * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nPairs)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(host.data() + (size_t)n * dim, dRes, 2 * (size_t)nPairs * sizeof(double),
                                           hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    const double *hMean = host.data(), *hSim = hMean + (size_t)n * dim, *hDist = hSim + nPairs;
    if (outMean)
        std::copy(hMean, hMean + (size_t)n * dim, outMean);
    if (outSim)
        std::copy(hSim, hSim + nPairs, outSim);
    if (outDist)
        std::copy(hDist, hDist + nPairs, outDist);
    return SSYM_OK;
}

}  // namespace

int32_t launch_frame_means(ssym_ctx *ctx, const double *feats, const uint64_t *off, uint32_t n, uint32_t dim,
                           double *mean)
{
    const uint64_t total = (uint64_t)n * dim;
    if (total == 0)
        return SSYM_OK;
    const unsigned grid = (unsigned)std::min<uint64_t>((total + kThreads - 1) / kThreads, (uint64_t)ctx->num_cus * 8);
    frame_means_kernel<<<grid, kThreads, 0, ctx->stream>>>(feats, off, n, dim, mean);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_sequence_distances(ssym_ctx *ctx, const double *feats, const uint64_t *frame_offsets, uint32_t n_sounds,
                                uint32_t dim, uint32_t flags, double *out_mean, double *out_sim, double *out_dist)
{
    return guarded(ctx, [&]() -> int32_t {
        return sequence_distances(ctx, feats, frame_offsets, n_sounds, dim, flags, out_mean, out_sim, out_dist);
    });
}

}  // extern "C"
