// mfcc.hip -- feature front-end: the step right before the hot path.
//
// Replaces analyze_mfccs (src/sound.rs:215-242): 1024-sample Hanning windows hopped by 256
// (src/lib.rs:24-25, src/sound.rs:228-229), per window a 12-coefficient MFCC between 100 Hz and
// 8 kHz (src/sound.rs:218), all frames of a sound back to back (frame-major, the layout
// Sound::mfccs() hands to the matcher, src/sound.rs:189-193).
//
// PARITY UNPINNED: the reference's arithmetic lives in two un-vendored crates (`vox_box` at git
// HEAD for the MFCC, `sample` 0.9.1 for the Windower) and no reference test holds a number for it.
// This is therefore a self-consistent extractor with its definition written down here (and
// restated on the CPU by the test oracle, which the parity tests compare against):
//   frames   T = (n - 1024) / 256 + 1 full windows (0 when n < 1024); with SSYM_MFCC_PAD_TAIL
//            T = n / 256 windows, samples past the end read as 0
//   window   w[i] = 0.5 - 0.5 cos(2 pi i / 1024)
//   spectrum X = FFT_1024(w x) (radix-2 decimation in time, f64), P[k] = re^2 + im^2, k = 0..512
//   mel      NF = 2 n_coeffs + 2 triangular filters, equally spaced on mel(f) = 1127 ln(1 + f/700)
//            between f_lo and min(f_hi, rate/2), evaluated at the bin centres k rate / 1024
//   E[m]     = sum_k W[m][k] P[k] (k ascending);  L[m] = ln(max(E[m], 1e-30))
//   c[j]     = sum_m L[m] cos(pi j (m + 1/2) / NF), j = 1..n_coeffs (m ascending; c0 is not kept)
// Window, twiddles, filter weights and the DCT matrix are tabulated on the host in f64 and uploaded,
// so device and oracle share every constant; FFT, spectrum and filter sums use the same operation
// order on both sides (bit-identical), the natural log is each side's libm.
//
// Mapping: one frame per 256-thread workgroup, the 1024-point FFT in LDS (16 KB), two butterflies
// per thread per stage; filter m and coefficient j are each one thread's sequential sum.
//
// Batch (ssym_mfcc_batch): a ragged batch of sounds, sound i = samples[off[i], off[i+1]).  Its frames
// are numbered across the batch (the prefix sums of ssym_mfcc_num_frames per sound); a grid-stride loop takes one
// frame per workgroup, which finds its sound by a wave-uniform binary search over the n + 1 frame offsets and runs
// the same per-frame body (mfcc_frame) as the single-sound kernel on that sound's samples alone: a window reads
// zeros past ITS sound's end (SSYM_MFCC_PAD_TAIL), never the next sound.  So every sound's frames are bit for bit
// those of ssym_mfcc.  One upload of all samples, one launch (plus the means kernel of sequence.hip when out_mean
// is asked), one copy back, one synchronisation per call.
#include "ssym_internal.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace ssym {

constexpr int kBin = SSYM_MFCC_BIN, kHop = SSYM_MFCC_HOP, kSpec = kBin / 2 + 1;
constexpr int kMaxFilters = 130;      // n_coeffs <= 64

}  // namespace ssym

#include "mfcc_frame.hpp"      // MfccTables, mfcc_frame, HostTables / build_tables, mfcc_args_ok

namespace ssym {

__global__ __launch_bounds__(256) void mfcc_kernel(const double *__restrict__ samples, uint64_t nSamples,
                                                   uint64_t nFrames, MfccTables tb, int nf, int nCoeffs,
                                                   double *__restrict__ out)
{
    __shared__ double re[kBin], im[kBin];
    __shared__ double logE[kMaxFilters];
    for (uint64_t t = blockIdx.x; t < nFrames; t += gridDim.x)
        mfcc_frame(samples, nSamples, t * kHop, tb, nf, nCoeffs, out + t * nCoeffs, re, im, logE);
}

// frameOff / smpOff: n + 1 offsets each (frames across the batch, samples from the batch's first sample)
__global__ __launch_bounds__(256) void mfcc_batch_kernel(const double *__restrict__ samples,
                                                         const uint64_t *__restrict__ frameOff,
                                                         const uint64_t *__restrict__ smpOff, uint32_t nSounds,
                                                         MfccTables tb, int nf, int nCoeffs, double *__restrict__ out)
{
    __shared__ double re[kBin], im[kBin];
    __shared__ double logE[kMaxFilters];
    const uint64_t nFrames = frameOff[nSounds];
    for (uint64_t t = blockIdx.x; t < nFrames; t += gridDim.x) {
        // the sound s with frameOff[s] <= t < frameOff[s + 1] (the last such s: empty sounds hold no frame)
        uint32_t lo = 0, hi = nSounds;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (frameOff[mid] <= t)
                lo = mid;
            else
                hi = mid;
        }
        const uint64_t s0 = smpOff[lo], len = smpOff[lo + 1] - s0;
        mfcc_frame(samples + s0, len, (t - frameOff[lo]) * kHop, tb, nf, nCoeffs, out + t * nCoeffs, re, im, logE);
    }
}

#define SSYM_MFCC_TRY(expr)                    \
    do {                                       \
        const int32_t rc__ = (expr);           \
        if (rc__ != SSYM_OK)                   \
            return rc__;                       \
    } while (0)

static int32_t mfcc_batch(ssym_ctx *ctx, const double *samples, const uint64_t *off, uint32_t n, double rate,
                          uint32_t nc, double f_lo, double f_hi, uint32_t flags, uint64_t *outFrameOff,
                          double *outMfccs, double *outMean)
{
    const char *fn = "ssym_mfcc_batch";
    if (!ctx)
        return SSYM_E_INVALID;
    if (!mfcc_args_ok(rate, nc, f_lo, f_hi)) {
        ctx->err = std::string(fn) + ": need 1 <= n_coeffs <= 64, sample_rate > 0, 0 <= f_lo < min(f_hi, sample_rate / 2)";
        return SSYM_E_INVALID;
    }
    if (n == 0)
        return SSYM_OK;
    if (!off) {
        ctx->err = std::string(fn) + ": NULL sample_offsets";
        return SSYM_E_INVALID;
    }
    // every check before any output or device memory is touched
    std::vector<uint64_t> offs(2 * ((size_t)n + 1));      // frame offsets [n + 1], then rebased sample offsets [n + 1]
    uint64_t *fo = offs.data(), *so = offs.data() + n + 1;
    const uint64_t base = off[0];
    for (uint32_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) {
            ctx->err = std::string(fn) + ": sample_offsets must not decrease";
            return SSYM_E_INVALID;
        }
        uint64_t T = 0;
        ssym_mfcc_num_frames(off[i + 1] - off[i], flags, &T);
        fo[i + 1] = fo[i] + T;
        so[i + 1] = off[i + 1] - base;
    }
    const uint64_t F = fo[n], total = so[n];
    if (total && !samples) {
        ctx->err = std::string(fn) + ": NULL samples";
        return SSYM_E_INVALID;
    }
    if (F && !outMfccs) {
        ctx->err = std::string(fn) + ": NULL out_mfccs";
        return SSYM_E_INVALID;
    }
    if (F == 0) {                            // no frame anywhere: nothing runs on the device
        if (outFrameOff)
            std::copy(fo, fo + n + 1, outFrameOff);
        if (outMean)
            for (size_t i = 0; i < (size_t)n * nc; ++i)
                outMean[i] = std::nan("");
        return SSYM_OK;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;
    HostTables ht;
    build_tables(ht, rate, nc, f_lo, f_hi);

    Blocks bl(ctx);
    double *dTab = nullptr, *dX = nullptr, *dOut = nullptr, *dMean = nullptr;
    int *dRange = nullptr;
    uint64_t *dOff = nullptr;
    SSYM_MFCC_TRY(bl.get(&dTab, ht.tab.size()));
    SSYM_MFCC_TRY(bl.get(&dRange, ht.range.size()));
    SSYM_MFCC_TRY(bl.get(&dOff, offs.size()));
    SSYM_MFCC_TRY(bl.get(&dX, total));
    if (outDev)
        dOut = outMfccs;
    else
        SSYM_MFCC_TRY(bl.get(&dOut, F * nc));
    if (outMean)
        SSYM_MFCC_TRY(bl.get(&dMean, (size_t)n * nc));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dTab, ht.tab.data(), ht.tab.size() * sizeof(double), hipMemcpyHostToDevice, st));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dRange, ht.range.data(), ht.range.size() * sizeof(int), hipMemcpyHostToDevice,
                                       st));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dOff, offs.data(), offs.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dX, samples + base, total * sizeof(double), hipMemcpyHostToDevice, st));
    const unsigned grid = (unsigned)std::min<uint64_t>(F, (uint64_t)ctx->num_cus * 16);
    mfcc_batch_kernel<<<grid, 256, 0, st>>>(dX, dOff, dOff + n + 1, n, ht.on(dTab, dRange), ht.nf, (int)nc, dOut);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    if (outMean)
        SSYM_MFCC_TRY(launch_frame_means(ctx, dOut, dOff, n, nc, dMean));
    if (!outDev)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(outMfccs, dOut, F * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    std::vector<double> mean;
    if (outMean) {
        mean.resize((size_t)n * nc);
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(mean.data(), dMean, mean.size() * sizeof(double), hipMemcpyDeviceToHost,
                                           st));
    }
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (outFrameOff)
        std::copy(fo, fo + n + 1, outFrameOff);
    if (outMean)
        std::copy(mean.begin(), mean.end(), outMean);
    return SSYM_OK;
}

}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_mfcc_num_frames(uint64_t n_samples, uint32_t flags, uint64_t *out_frames)
{
    if (!out_frames)
        return SSYM_E_INVALID;
    if (flags & SSYM_MFCC_PAD_TAIL)
        *out_frames = n_samples / kHop;
    else
        *out_frames = n_samples >= (uint64_t)kBin ? (n_samples - kBin) / kHop + 1 : 0;
    return SSYM_OK;
}

int32_t ssym_mfcc(ssym_ctx *ctx, const double *samples, uint64_t n_samples, double sample_rate,
                  uint32_t n_coeffs, double f_lo, double f_hi, uint32_t flags, double *out_mfccs,
                  double *out_mean)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (!mfcc_args_ok(sample_rate, n_coeffs, f_lo, f_hi)) {
        ctx->err = "ssym_mfcc: need 1 <= n_coeffs <= 64, sample_rate > 0, 0 <= f_lo < min(f_hi, sample_rate / 2)";
        return SSYM_E_INVALID;
    }
    uint64_t T = 0;
    ssym_mfcc_num_frames(n_samples, flags, &T);
    if (out_mean)
        for (uint32_t j = 0; j < n_coeffs; ++j)
            out_mean[j] = 0.0;
    if (T == 0)
        return SSYM_OK;
    if (!samples || !out_mfccs) {
        ctx->err = "ssym_mfcc: NULL buffer";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool outDev = (flags & SSYM_OUT_DEVICE) != 0;

    HostTables ht;
    build_tables(ht, sample_rate, n_coeffs, f_lo, f_hi);
    const std::vector<double> &tab = ht.tab;
    const std::vector<int> &range = ht.range;
    const size_t nTab = tab.size();
    const int nf = ht.nf;

    double *dTab = nullptr, *dSmp = nullptr, *dOut = nullptr;
    int *dRange = nullptr;
    int32_t rc = dev_alloc(ctx, (void **)&dTab, nTab * sizeof(double));
    if (rc == SSYM_OK)
        rc = dev_alloc(ctx, (void **)&dRange, range.size() * sizeof(int));
    if (rc == SSYM_OK)
        rc = dev_alloc(ctx, (void **)&dSmp, n_samples * sizeof(double));
    if (rc == SSYM_OK && !outDev)
        rc = dev_alloc(ctx, (void **)&dOut, T * n_coeffs * sizeof(double));
    hipError_t e = hipSuccess;
    if (rc == SSYM_OK) {
        if (outDev)
            dOut = out_mfccs;
        e = hipMemcpyAsync(dTab, tab.data(), nTab * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dRange, range.data(), range.size() * sizeof(int), hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dSmp, samples, n_samples * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            const MfccTables tb = ht.on(dTab, dRange);
            const unsigned grid = (unsigned)std::min<uint64_t>(T, (uint64_t)ctx->num_cus * 16);
            mfcc_kernel<<<grid, 256, 0, st>>>(dSmp, n_samples, T, tb, nf, (int)n_coeffs, dOut);
            e = hipGetLastError();
        }
        std::vector<double> hostOut;
        double *res = out_mfccs;
        if (e == hipSuccess && outDev && out_mean) {
            hostOut.resize(T * n_coeffs);
            res = hostOut.data();
        }
        if (e == hipSuccess && (!outDev || out_mean))
            e = hipMemcpyAsync(res, dOut, T * n_coeffs * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e == hipSuccess && out_mean) {
            // analyze_mean_mfccs (src/sound.rs:271-286): per-coefficient sum over frames, then / T
            for (uint64_t t = 0; t < T; ++t)
                for (uint32_t j = 0; j < n_coeffs; ++j)
                    out_mean[j] += res[t * n_coeffs + j];
            for (uint32_t j = 0; j < n_coeffs; ++j)
                out_mean[j] = out_mean[j] / (double)T;
        }
    }
    dev_free(ctx, dTab);
    dev_free(ctx, dRange);
    dev_free(ctx, dSmp);
    if (!outDev)
        dev_free(ctx, dOut);
    if (rc != SSYM_OK)
        return rc;
    if (e != hipSuccess) {
        ctx->err = std::string("ssym_mfcc: ") + hipGetErrorString(e);
        return SSYM_E_HIP;
    }
    return SSYM_OK;
    });
}

int32_t ssym_mfcc_batch(ssym_ctx *ctx, const double *samples, const uint64_t *sample_offsets, uint32_t n_sounds,
                        double sample_rate, uint32_t n_coeffs, double f_lo, double f_hi, uint32_t flags,
                        uint64_t *out_frame_offsets, double *out_mfccs, double *out_mean)
{
    return guarded(ctx, [&]() -> int32_t {
        return mfcc_batch(ctx, samples, sample_offsets, n_sounds, sample_rate, n_coeffs, f_lo, f_hi, flags,
                          out_frame_offsets, out_mfccs, out_mean);
    });
}

}  // extern "C"
