// warp_common.hpp -- what the two resynthesis kernels share (warp.hip: plain overlap-add along the frame map; wsola.hip:
// the same overlap-add from searched frame positions): the frame geometry, the window's bits and the 32-bit conversion.
#pragma once
#include "ssym_internal.hpp"

#include <cmath>
#include <vector>

namespace ssym {

constexpr int kWarpHop = SSYM_MFCC_HOP, kWarpBin = SSYM_MFCC_BIN;
constexpr int kWarpTaps = kWarpBin / kWarpHop;                    // 4 windows cover a sample
constexpr int kWarpChunk = 4096;                                  // samples per workgroup
constexpr int kWarpFrames = kWarpChunk / kWarpHop + kWarpTaps - 1;    // 19 target frames reach into a chunk
static_assert(kWarpHop == 256 && kWarpTaps == 4 && kWarpFrames == 19, "warp kernels: 256 threads, one hop each");

// (i32::max_value() as f64 * sample) as i32, as reconstruct_kernel: truncate toward zero, saturate, NaN -> 0
__device__ __forceinline__ int32_t warp_pcm32(double v)
{
    const double x = __dmul_rn(2147483647.0, v);
    if (x != x) return 0;
    if (x >= 2147483647.0) return 2147483647;
    if (x <= -2147483648.0) return (int32_t)0x80000000;
    return (int32_t)x;
}

// w[m] = 0.5 - 0.5 cos(2 pi m / 1024): the text of build_tables (mfcc_frame.hpp), so the bits of the MFCC window
inline const std::vector<double> &warp_window()
{
    static const std::vector<double> win = [] {
        const double PI = 3.14159265358979323846;
        std::vector<double> w(kWarpBin);
        for (int i = 0; i < kWarpBin; ++i)
            w[i] = 0.5 - 0.5 * std::cos(2.0 * PI * (double)i / (double)kWarpBin);
        return w;
    }();
    return win;
}

}  // namespace ssym
