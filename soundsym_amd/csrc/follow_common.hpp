// follow_common.hpp -- what envelope following (follow.hip: ssym_follow_envelope, whole targets) and the live follower
// (follower.hip: ssym_follower_*, growing lanes) share on the device: the geometry of a block of boundaries in LDS, the
// 1024-step energy chain, the gain's division, square root and selects, and the arithmetic of one output sample.  One text
// for both, as wsola_step is for wsola.hip and resynth.hip: the live follower is held to the offline call bit for bit, and
// it gets there by running the same instructions on the same staged values.
//
// Layout (follow.hip describes why): a block of up to 32 consecutive boundaries, its windows spanning up to 35 hops; the
// span of y and of x staged hop by hop with a pitch of 257 doubles, +0.0 wherever the definition leaves a term out; the
// window table beside them.  Wave 0 runs the chains: lanes 0 ... 31 the block's boundaries on y, lanes 32 ... 63 on x.
#pragma once
#include "warp_common.hpp"

namespace ssym {

constexpr int kFollowBlock = 32;                           // boundaries per workgroup of a gain kernel
constexpr int kFollowHops = kFollowBlock + kWarpTaps - 1;  // 35 hops under a full block's windows
constexpr int kFollowPitch = kWarpHop + 1;                 // doubles from one staged hop to the next
constexpr uint64_t kFollowMaxLen = 1ull << 40;             // samples per target or lane: boundaries then fit 32 bits with room
static_assert(kFollowBlock == 32 && kWarpHop == 256 && kWarpBin == 1024, "gain kernels: one wave of chains, 256 stagers");

// doubles of dynamic LDS of a gain kernel whose largest block has nb boundaries: [1024] the window, then [2][nb + 3][257]
inline size_t follow_lds_doubles(uint64_t nb)
{
    return kWarpBin + 2 * (size_t)(std::min<uint64_t>(nb, kFollowBlock) + kWarpTaps - 1) * kFollowPitch;
}
static_assert((kWarpBin + 2 * kFollowHops * kFollowPitch) * sizeof(double) <= 160 * 1024, "gain kernels: a CU's LDS");

// E_s(b) of one lane: s the staged hop the boundary's window starts at, sw the window.  Sixteen steps at a time, the next
// sixteen's reads issued before the sum goes through these (one wave: nothing else hides an LDS read); a group of 16 never
// straddles a hop, so its slots are consecutive.
__device__ __forceinline__ double follow_chain(const double *s, const double *sw)
{
    constexpr int U = 16;
    double acc = 0.0, v[U], w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        v[u] = s[u];
        w[u] = sw[u];
    }
    for (int m = 0; m < kWarpBin; m += U) {
        double nv[U], nw[U];
        const int mn = m + U < kWarpBin ? m + U : m;            // the last group reads itself again: in range, unused
        const double *sn = s + mn + (mn >> 8);                  // hop mn / 256 of the window, pitch 257
#pragma unroll
        for (int u = 0; u < U; ++u) {
            nv[u] = sn[u];
            nw[u] = sw[mn + u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double p = __dmul_rn(v[u], v[u]);
            p = __dmul_rn(w[u], p);
            acc = __dadd_rn(acc, p);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = nv[u];
            w[u] = nw[u];
        }
    }
    return acc;
}

// g(b) from the two energies
__device__ __forceinline__ double follow_gain(double ex, double ey, double maxGain)
{
    double g = __dsqrt_rn(__ddiv_rn(ex, ey));
    if (g != g)
        g = 1.0;
    else if (g > maxGain)
        g = maxGain;
    return g;
}

// out[k] of the sample v in hop j: g0 = g(j), g1 = g(j + 1), f = (k - j * HOP) / 256.0, fm = 1.0 - f (both exact)
__device__ __forceinline__ double follow_sample(double v, double g0, double g1, double f, double fm)
{
    const double ga = __dmul_rn(g0, fm), gc = __dmul_rn(g1, f);
    return __dmul_rn(v, __dadd_rn(ga, gc));
}

}  // namespace ssym
