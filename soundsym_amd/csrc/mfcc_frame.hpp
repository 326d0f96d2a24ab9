// mfcc_frame.hpp -- the per-frame body of the MFCC front-end and its host tables, shared by mfcc.hip (whole sounds,
// batches) and stream.hip (the new frames of a growing sound).  One text, one arithmetic: a frame is the same bits
// whichever kernel computes it.  The definition is written down at the top of mfcc.hip.
//
// The including unit states the geometry it launches with -- kBin, kHop, kSpec, kMaxFilters in namespace ssym -- before
// this header; the assertion below keeps every unit on the public constants.
#pragma once

#include "ssym_internal.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace ssym {

static_assert(kBin == SSYM_MFCC_BIN && kHop == SSYM_MFCC_HOP && kSpec == kBin / 2 + 1 && kMaxFilters == 130,
              "mfcc_frame: 1024-sample windows hopped by 256, up to 2 * 64 + 2 filters");

struct MfccTables {
    const double *win;      // [1024]
    const double *twRe;     // [512]  cos(-2 pi k / 1024)
    const double *twIm;     // [512]  sin(-2 pi k / 1024)
    const double *weights;  // [nf][513]
    const int *lo, *hi;     // [nf] first / one-past-last bin with a non-zero weight
    const double *dct;      // [n_coeffs][nf]
};

__device__ __forceinline__ uint32_t bitrev10(uint32_t i) { return __brev(i) >> 22; }

// one frame: samples x[base .. base + 1024) of a sound of n samples (zeros past n) -> out[0 .. nCoeffs).  Called
// by every thread of a 256-thread workgroup; re / im / logE are the workgroup's LDS, free on entry and on return.
__device__ __forceinline__ void mfcc_frame(const double *__restrict__ x, uint64_t n, uint64_t base,
                                           const MfccTables &tb, int nf, int nCoeffs, double *__restrict__ out,
                                           double *re, double *im, double *logE)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < kBin / 256; ++q) {
        const int i = tid + 256 * q;
        const uint64_t g = base + i;
        const double v = g < n ? x[g] : 0.0;
        const uint32_t r = bitrev10((uint32_t)i);
        re[r] = __dmul_rn(v, tb.win[i]);
        im[r] = 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s <= 10; ++s) {
        const int half = 1 << (s - 1);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int b = tid + 256 * q;
            const int j = b & (half - 1);
            const int i0 = ((b >> (s - 1)) << s) + j, i1 = i0 + half;
            const int k = j << (10 - s);
            const double wr = tb.twRe[k], wi = tb.twIm[k];
            const double xr = re[i1], xi = im[i1];
            const double tr = __dsub_rn(__dmul_rn(wr, xr), __dmul_rn(wi, xi));
            const double ti = __dadd_rn(__dmul_rn(wr, xi), __dmul_rn(wi, xr));
            const double ar = re[i0], ai = im[i0];
            re[i1] = __dsub_rn(ar, tr);
            im[i1] = __dsub_rn(ai, ti);
            re[i0] = __dadd_rn(ar, tr);
            im[i0] = __dadd_rn(ai, ti);
        }
        __syncthreads();
    }
    // power spectrum into re[0..512] (each thread reads and writes its own bins only)
    for (int k = tid; k < kSpec; k += 256) {
        const double a = re[k], b = im[k];
        re[k] = __dadd_rn(__dmul_rn(a, a), __dmul_rn(b, b));
    }
    __syncthreads();
    if (tid < nf) {
        const double *w = tb.weights + (size_t)tid * kSpec;
        double e = 0.0;
        for (int k = tb.lo[tid]; k < tb.hi[tid]; ++k)
            e = __dadd_rn(e, __dmul_rn(w[k], re[k]));
        logE[tid] = log(fmax(e, 1e-30));
    }
    __syncthreads();
    if (tid < nCoeffs) {
        const double *d = tb.dct + (size_t)tid * nf;
        double c = 0.0;
        for (int m = 0; m < nf; ++m)
            c = __dadd_rn(c, __dmul_rn(logE[m], d[m]));
        out[tid] = c;
    }
    __syncthreads();   // re / im / logE are reused by the next frame
}

static inline double mel_of(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }
static inline double hz_of(double m) { return 700.0 * (std::exp(m / 1127.0) - 1.0); }

// the host tables of one (rate, n_coeffs, f_lo, f_hi) in f64 (the oracle tabulates the same expressions), and where
// each lies in `tab` / `range` (nf lower, then nf upper bin bounds)
struct HostTables {
    int nf = 0;
    size_t oWin = 0, oTwRe = 0, oTwIm = 0, oW = 0, oDct = 0;
    std::vector<double> tab;
    std::vector<int> range;
    MfccTables on(const double *dTab, const int *dRange) const
    {
        return MfccTables{dTab + oWin, dTab + oTwRe, dTab + oTwIm, dTab + oW, dRange, dRange + nf, dTab + oDct};
    }
};

static inline void build_tables(HostTables &h, double sample_rate, uint32_t n_coeffs, double f_lo, double f_hi)
{
    const int nf = 2 * (int)n_coeffs + 2;
    const double PI = 3.14159265358979323846;
    h.nf = nf;
    h.oWin = 0;
    h.oTwRe = h.oWin + kBin;
    h.oTwIm = h.oTwRe + kBin / 2;
    h.oW = h.oTwIm + kBin / 2;
    h.oDct = h.oW + (size_t)nf * kSpec;
    std::vector<double> &tab = h.tab;
    tab.assign(h.oDct + (size_t)n_coeffs * nf, 0.0);
    for (int i = 0; i < kBin; ++i)
        tab[h.oWin + i] = 0.5 - 0.5 * std::cos(2.0 * PI * (double)i / (double)kBin);
    for (int k = 0; k < kBin / 2; ++k) {
        tab[h.oTwRe + k] = std::cos(-2.0 * PI * (double)k / (double)kBin);
        tab[h.oTwIm + k] = std::sin(-2.0 * PI * (double)k / (double)kBin);
    }
    std::vector<int> &range = h.range;
    range.assign(2 * (size_t)nf, 0);
    {
        const double top = std::min(f_hi, 0.5 * sample_rate);
        const double m0 = mel_of(f_lo), m1 = mel_of(top);
        for (int m = 0; m < nf; ++m) {
            const double h0 = hz_of(m0 + (m1 - m0) * (double)m / (double)(nf + 1));
            const double h1 = hz_of(m0 + (m1 - m0) * (double)(m + 1) / (double)(nf + 1));
            const double h2 = hz_of(m0 + (m1 - m0) * (double)(m + 2) / (double)(nf + 1));
            int lo = kSpec, hi = 0;
            for (int k = 0; k < kSpec; ++k) {
                const double f = (double)k * sample_rate / (double)kBin;
                double w = 0.0;
                if (f > h0 && f <= h1)
                    w = (f - h0) / (h1 - h0);
                else if (f > h1 && f < h2)
                    w = (h2 - f) / (h2 - h1);
                tab[h.oW + (size_t)m * kSpec + k] = w;
                if (w != 0.0) {
                    lo = std::min(lo, k);
                    hi = std::max(hi, k + 1);
                }
            }
            range[m] = lo < hi ? lo : 0;
            range[nf + m] = lo < hi ? hi : 0;
        }
    }
    for (uint32_t j = 0; j < n_coeffs; ++j)
        for (int m = 0; m < nf; ++m)
            tab[h.oDct + (size_t)j * nf + m] = std::cos(PI * (double)(j + 1) * ((double)m + 0.5) / (double)nf);
}

// the band must be non-empty below Nyquist: with f_lo >= min(f_hi, rate / 2) the mel grid runs from f_lo DOWN to
// rate / 2, every filter weight is 0 and the coefficients would be the DCT of the constant 1e-30 floor
static inline bool mfcc_args_ok(double sample_rate, uint32_t n_coeffs, double f_lo, double f_hi)
{
    return !(n_coeffs == 0 || n_coeffs > 64 || !(sample_rate > 0.0) || !(f_lo >= 0.0) || !(f_hi > f_lo) ||
             !(f_lo < 0.5 * sample_rate));
}

}  // namespace ssym
