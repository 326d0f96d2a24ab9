// pitch.hip -- per-sound descriptors of a ragged batch of sounds: max_power and pitch_confidence
// (Sound::max_power / pitch_confidence, src/sound.rs:166-179, analyze_max_power / analyze_pitch_confidence :244-269).
//
// PARITY UNPINNED: analyze_pitch_confidence calls vox_box's `pitch::<Hanning>` (an un-vendored crate at an unpinned git
// HEAD), so the definition is this library's own, after Boersma (1993), written down in DESIGN.md section 5.9 and
// restated in numpy by tests/pitch_ref.py.  Per sound, with W = 2048, H = 1024, h[n] = 0.5 - 0.5 cos(2 pi n / W):
//   G        max |x| over the sound (NaN skipped)
//   window   c = x[s..s+W) h, y = c h (the second Hanning of pitch::<Hanning>), L = max |c|
//   a(tau)   sum_{n < W - tau} y[n] y[n + tau], n ASCENDING, one sequential f64 fold per lag (two lags per thread)
//   r(tau)   (a(tau) / a(0)) / bnorm(tau), bnorm = b(tau) / b(0) the same sums of h^2 (host table)
//   voiced   local maxima of r in [tau_lo, tau_hi], parabolic refinement, strength R - kappa log2(f_min (tau+d) / rate)
//   unvoiced u = v + max(0, 2 - (L / G) / (sigma / (1 + v)))
//   score    max(u, best voiced) (voiced wins ties; SSYM_PITCH_VOICED: best voiced or 0); NaN for a window holding a
//            non-finite sample; the sound's confidence is the max over its windows from 0, NaN skipped
// max_power: the largest sqrt((sum of squares, sequential) / 128) over full 128-sample windows hopped by 64, from 0.
// The maxima are order-independent, so both folds are integer atomicMax on the bits of non-negative doubles: every
// value is bit-identical to a sequential host fold and a second call gives the same bits.  No floating-point atomics.
//
// Mapping: one 256-thread workgroup per 8192-sample chunk for the peaks and power windows, one per pitch window for the
// autocorrelation (y staged in LDS, 16 KB).  Every read lies inside its sound: nothing past sample_offsets[n_sounds].
#include "ssym_internal.hpp"

#include <climits>
#include <cmath>
#include <vector>

namespace ssym {
namespace {

constexpr int kW = SSYM_PITCH_WINDOW, kH = SSYM_PITCH_HOP, kPW = SSYM_POWER_WINDOW, kPH = SSYM_POWER_HOP;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kChunk = 8192;                 // samples per workgroup of the peak / power pass (a multiple of kPH)
constexpr int kMaxTau = kW / 3;              // tau_hi <= 682: three periods per window
constexpr int kMaxLags = kMaxTau + 2;        // r(tau) for tau in [tau_lo - 1, tau_hi + 1], tau_lo >= 2
static_assert(kChunk % kPH == 0, "chunks start on power windows");

struct Chunk {
    uint64_t start, end, soundEnd;           // samples [start, end) of a sound ending at soundEnd
    uint32_t sound, pad;
};
struct Win {
    uint64_t start;
    uint32_t sound, pad;
};
struct PitchArgs {
    double rate, fMin, voicing;
    int lo, hi;                              // tau_lo, tau_hi
    uint32_t flags;
};

// max of a non-negative, non-NaN value over the workgroup (every thread gets it)
__device__ double block_max(double v, double *red)
{
    for (int o = 32; o > 0; o >>= 1)
        v = fmax(v, __shfl_down(v, o));
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int i = 1; i < kWaves; ++i)
        r = fmax(r, red[i]);
    __syncthreads();
    return r;
}

// fold a value > 0 into a max that starts at +0.0: the bits of non-negative doubles order like the doubles
__device__ void atomic_max_pos(double *p, double v)
{
    if (v > 0.0)
        atomicMax((unsigned long long *)p, (unsigned long long)__double_as_longlong(v));
}

__global__ __launch_bounds__(kThreads) void peaks_kernel(const double *__restrict__ x, const Chunk *__restrict__ chunks,
                                                         uint32_t nChunks, double *__restrict__ peak,
                                                         double *__restrict__ power)
{
    __shared__ double red[kWaves];
    for (uint32_t c = blockIdx.x; c < nChunks; c += gridDim.x) {
        const Chunk ch = chunks[c];
        double g = 0.0, p = 0.0;
        for (uint64_t i = ch.start + threadIdx.x; i < ch.end; i += kThreads) {
            const double a = fabs(x[i]);
            if (a > g)          // a NaN never compares greater: skipped, as by f64::max
                g = a;
        }
        // the power windows that start in this chunk (sound-relative multiples of kPH) and end inside the sound
        for (uint64_t w = ch.start + (uint64_t)threadIdx.x * kPH; w < ch.end && w + kPW <= ch.soundEnd;
             w += (uint64_t)kThreads * kPH) {
            double acc = 0.0;
            for (int i = 0; i < kPW; ++i)
                acc = __dadd_rn(acc, __dmul_rn(x[w + i], x[w + i]));
            const double rms = sqrt(acc / (double)kPW);
            if (rms > p)
                p = rms;
        }
        g = block_max(g, red);
        p = block_max(p, red);
        if (threadIdx.x == 0) {
            atomic_max_pos(peak + ch.sound, g);
            atomic_max_pos(power + ch.sound, p);
        }
    }
}

__global__ __launch_bounds__(kThreads) void pitch_kernel(const double *__restrict__ x, const Win *__restrict__ wins,
                                                         uint32_t nWins, const double *__restrict__ hann,
                                                         const double *__restrict__ bnorm, PitchArgs pa,
                                                         const double *__restrict__ peak, double *__restrict__ conf,
                                                         double *__restrict__ outFreq, double *__restrict__ outStr,
                                                         double *__restrict__ outU)
{
    __shared__ double y[kW];
    __shared__ double a[kMaxLags + 1];       // a(0), then a(tau) for tau = lo - 1 .. hi + 1
    __shared__ double r[kMaxLags];           // r(tau) for tau = lo - 1 .. hi + 1
    __shared__ double red[kWaves], redS[kWaves], redD[kWaves];
    __shared__ int redT[kWaves];
    const int tid = threadIdx.x;
    const int nR = pa.hi - pa.lo + 3;        // lags of r
    for (uint32_t t = blockIdx.x; t < nWins; t += gridDim.x) {
        const Win wn = wins[t];
        const double *xs = x + wn.start;     // wn.start + kW <= the sound's end (host table)
        double l = 0.0;
        int bad = 0;
        for (int n = tid; n < kW; n += kThreads) {
            const double v = xs[n];
            bad |= !isfinite(v);
            const double c = __dmul_rn(v, hann[n]);
            y[n] = __dmul_rn(c, hann[n]);
            const double ac = fabs(c);
            if (ac > l)
                l = ac;
        }
        bad = __syncthreads_or(bad);
        if (bad) {
            if (tid == 0) {
                const double nan = __longlong_as_double(0x7ff8000000000000ll);
                if (outFreq)
                    outFreq[t] = nan;
                if (outStr)
                    outStr[t] = nan;
                if (outU)
                    outU[t] = nan;
            }
            continue;                        // uniform: nobody reads y in this window, the next one may overwrite it
        }
        const double L = block_max(l, red);
        // thread 0: a(0); thread q >= 1: the two lags a[2q - 1], a[2q] (tau, tau + 1), which share their loads --
        // y[n + tau] of step n + 1 is y[n + tau + 1] of step n.  Each lag stays one fold in ascending n.  An odd
        // count computes one lag past hi + 1 (tau <= 684 < kW, a[] has room) that nobody reads.
        for (int q = tid; q <= (nR + 1) / 2; q += kThreads) {
            if (q == 0) {
                double acc = 0.0;
                for (int n = 0; n < kW; ++n)
                    acc = __dadd_rn(acc, __dmul_rn(y[n], y[n]));
                a[0] = acc;
                continue;
            }
            const int tau = pa.lo - 3 + 2 * q;
            double acc0 = 0.0, acc1 = 0.0, cur = y[tau];
            for (int n = 0; n < kW - tau - 1; ++n) {
                const double yn = y[n], next = y[n + tau + 1];
                acc0 = __dadd_rn(acc0, __dmul_rn(yn, cur));
                acc1 = __dadd_rn(acc1, __dmul_rn(yn, next));
                cur = next;
            }
            acc0 = __dadd_rn(acc0, __dmul_rn(y[kW - tau - 1], cur));       // cur = y[kW - 1]
            a[2 * q - 1] = acc0;
            a[2 * q] = acc1;
        }
        __syncthreads();
        const double a0 = a[0];
        for (int j = tid; j < nR; j += kThreads)
            r[j] = (a[j + 1] / a0) / bnorm[j];
        __syncthreads();
        // best voiced candidate of this thread: lags ascending, so the first maximum (the smaller tau) is kept
        double bestS = -INFINITY, bestD = 0.0;
        int bestT = INT_MAX;
        if (a0 != 0.0) {
            for (int k = tid; k <= pa.hi - pa.lo; k += kThreads) {
                const double rm = r[k], r0 = r[k + 1], rp = r[k + 2];
                if (!(r0 > rm && r0 >= rp))
                    continue;
                const double d = __dadd_rn(__dsub_rn(rm, __dmul_rn(2.0, r0)), rp);
                const double diff = __dsub_rn(rm, rp);
                const double delta = d < 0.0 ? diff / __dmul_rn(2.0, d) : 0.0;
                const double R = __dsub_rn(r0, __dmul_rn(diff, delta) / 4.0);
                const double tq = __dadd_rn((double)(pa.lo + k), delta);
                const double S = __dsub_rn(R, __dmul_rn(SSYM_PITCH_OCTAVE_COST, log2(__dmul_rn(pa.fMin, tq) / pa.rate)));
                if (S > bestS) {
                    bestS = S;
                    bestT = pa.lo + k;
                    bestD = delta;
                }
            }
        }
        // workgroup arg-max: the larger strength, then the smaller tau (independent of the reduction order)
        for (int o = 32; o > 0; o >>= 1) {
            const double s2 = __shfl_down(bestS, o), d2 = __shfl_down(bestD, o);
            const int t2 = __shfl_down(bestT, o);
            if (s2 > bestS || (s2 == bestS && t2 < bestT)) {
                bestS = s2;
                bestT = t2;
                bestD = d2;
            }
        }
        if ((tid & 63) == 0) {
            redS[tid >> 6] = bestS;
            redT[tid >> 6] = bestT;
            redD[tid >> 6] = bestD;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 1; i < kWaves; ++i)
                if (redS[i] > bestS || (redS[i] == bestS && redT[i] < bestT)) {
                    bestS = redS[i];
                    bestT = redT[i];
                    bestD = redD[i];
                }
            const bool has = bestT != INT_MAX;
            const double freq = has ? pa.rate / __dadd_rn((double)bestT, bestD) : 0.0;
            const double str = has ? bestS : 0.0;
            const double v = pa.voicing;
            const double q = (L / peak[wn.sound]) / (SSYM_PITCH_SILENCE / __dadd_rn(1.0, v));
            const double u = __dadd_rn(v, fmax(0.0, __dsub_rn(2.0, q)));     // fmax: a NaN (G = 0) gives v
            double score = has && str >= u ? str : u;
            if (pa.flags & SSYM_PITCH_VOICED)
                score = str;
            atomic_max_pos(conf + wn.sound, score);
            if (outFreq)
                outFreq[t] = freq;
            if (outStr)
                outStr[t] = str;
            if (outU)
                outU[t] = u;
        }
        __syncthreads();                     // y, a, r and the reduction slots are reused by the next window
    }
}

#define SSYM_PITCH_TRY(expr)                   \
    do {                                       \
        const int32_t rc__ = (expr);           \
        if (rc__ != SSYM_OK)                   \
            return rc__;                       \
    } while (0)

uint64_t num_windows(uint64_t n) { return n >= (uint64_t)kW ? (n - kW) / kH + 1 : 0; }

// every limit of DESIGN.md 5.9, checked before anything touches the device
int32_t check_args(ssym_ctx *ctx, const char *fn, const double *samples, const uint64_t *off, uint32_t n, double rate,
                   double fMin, double fMax, double voicing, int *lo, int *hi)
{
    if (!(std::isfinite(rate) && rate > 0.0 && std::isfinite(fMin) && std::isfinite(fMax) && fMin > 0.0 &&
          fMin < fMax && std::isfinite(voicing))) {
        ctx->err = std::string(fn) + ": need a finite rate > 0, 0 < f_min < f_max and a finite voicing threshold";
        return SSYM_E_INVALID;
    }
    const double tl = std::ceil(rate / fMax), th = std::floor(rate / fMin);
    if (!(tl >= 2.0 && th <= (double)kMaxTau && tl <= th)) {
        ctx->err = std::string(fn) + ": need 2 <= ceil(rate / f_max) <= floor(rate / f_min) <= 682 (three periods per "
                                     "2048-sample window)";
        return SSYM_E_INVALID;
    }
    *lo = (int)tl;
    *hi = (int)th;
    if (n == 0)
        return SSYM_OK;
    if (!off) {
        ctx->err = std::string(fn) + ": NULL sample_offsets";
        return SSYM_E_INVALID;
    }
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) {
            ctx->err = std::string(fn) + ": sample_offsets must not decrease";
            return SSYM_E_INVALID;
        }
    if (off[n] > off[0] && !samples) {
        ctx->err = std::string(fn) + ": NULL samples";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

int32_t run(ssym_ctx *ctx, const char *fn, const double *samples, const uint64_t *off, uint32_t n, double rate,
            double fMin, double fMax, double voicing, uint32_t flags, double *outPower, double *outConf,
            double *outFreq, double *outStr, double *outU)
{
    if (!ctx)
        return SSYM_E_INVALID;
    int lo = 0, hi = 0;
    SSYM_PITCH_TRY(check_args(ctx, fn, samples, off, n, rate, fMin, fMax, voicing, &lo, &hi));
    if (n == 0)
        return SSYM_OK;
    const uint64_t base = off[0], total = off[n] - base;
    std::vector<Win> wins;
    std::vector<Chunk> chunks;
    for (uint32_t s = 0; s < n; ++s) {
        const uint64_t a = off[s] - base, len = off[s + 1] - off[s];
        const uint64_t nw = num_windows(len);
        for (uint64_t k = 0; k < nw; ++k)
            wins.push_back(Win{a + k * kH, s, 0});
        for (uint64_t c = 0; c < len; c += kChunk)
            chunks.push_back(Chunk{a + c, a + std::min<uint64_t>(c + kChunk, len), a + len, s, 0});
    }
    if (wins.size() >= (1ull << 31) || chunks.size() >= (1ull << 31)) {
        ctx->err = std::string(fn) + ": more than 2^31 windows in one call";
        return SSYM_E_INVALID;
    }
    if (total == 0) {                        // only empty sounds: every descriptor is 0
        for (uint32_t s = 0; s < n; ++s) {
            if (outPower)
                outPower[s] = 0.0;
            if (outConf)
                outConf[s] = 0.0;
        }
        return SSYM_OK;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // tables: h [kW], then bnorm [nR] = b(tau) / b(0) for tau = lo - 1 .. hi + 1, b the sequential sums of h^2
    const int nR = hi - lo + 3;
    const double PI = 3.14159265358979323846;
    std::vector<double> tab(kW + nR), hh(kW);
    for (int i = 0; i < kW; ++i) {
        tab[i] = 0.5 - 0.5 * std::cos(2.0 * PI * (double)i / (double)kW);
        hh[i] = tab[i] * tab[i];
    }
    auto bsum = [&](int tau) {
        double acc = 0.0;
        for (int i = 0; i < kW - tau; ++i)
            acc = acc + hh[i] * hh[i + tau];
        return acc;
    };
    const double b0 = bsum(0);
    for (int j = 0; j < nR; ++j)
        tab[kW + j] = bsum(lo - 1 + j) / b0;

    const uint64_t nW = wins.size();
    const bool track = nW && (outFreq || outStr || outU);
    Blocks bl(ctx);
    double *dX = nullptr, *dTab = nullptr, *dRes = nullptr, *dTrack = nullptr;
    Win *dWins = nullptr;
    Chunk *dChunks = nullptr;
    SSYM_PITCH_TRY(bl.get(&dX, total));
    SSYM_PITCH_TRY(bl.get(&dTab, tab.size()));
    SSYM_PITCH_TRY(bl.get(&dRes, 3 * (size_t)n));            // peak, power, confidence
    SSYM_PITCH_TRY(bl.get(&dChunks, chunks.size()));
    if (nW)
        SSYM_PITCH_TRY(bl.get(&dWins, nW));
    if (track)
        SSYM_PITCH_TRY(bl.get(&dTrack, 3 * nW));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dX, samples + base, total * sizeof(double), hipMemcpyHostToDevice, st));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dTab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dChunks, chunks.data(), chunks.size() * sizeof(Chunk), hipMemcpyHostToDevice, st));
    if (nW)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(dWins, wins.data(), nW * sizeof(Win), hipMemcpyHostToDevice, st));
    SSYM_HIP_CHECK(ctx, hipMemsetAsync(dRes, 0, 3 * (size_t)n * sizeof(double), st));
    double *dPeak = dRes, *dPower = dRes + n, *dConf = dRes + 2 * (size_t)n;

    const uint64_t cap = (uint64_t)ctx->num_cus * 8;
    peaks_kernel<<<(unsigned)std::min<uint64_t>(chunks.size(), cap), kThreads, 0, st>>>(
        dX, dChunks, (uint32_t)chunks.size(), dPeak, dPower);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    if (nW) {
        const PitchArgs pa{rate, fMin, voicing, lo, hi, flags};
        pitch_kernel<<<(unsigned)std::min<uint64_t>(nW, cap), kThreads, 0, st>>>(
            dX, dWins, (uint32_t)nW, dTab, dTab + kW, pa, dPeak, dConf, track && outFreq ? dTrack : nullptr,
            track && outStr ? dTrack + nW : nullptr, track && outU ? dTrack + 2 * nW : nullptr);
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    if (outPower)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(outPower, dPower, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (outConf)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(outConf, dConf, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (track && outFreq)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(outFreq, dTrack, nW * sizeof(double), hipMemcpyDeviceToHost, st));
    if (track && outStr)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(outStr, dTrack + nW, nW * sizeof(double), hipMemcpyDeviceToHost, st));
    if (track && outU)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(outU, dTrack + 2 * nW, nW * sizeof(double), hipMemcpyDeviceToHost, st));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return SSYM_OK;
}

}  // namespace
}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_pitch_num_windows(uint64_t n_samples, uint64_t *out_windows)
{
    if (!out_windows)
        return SSYM_E_INVALID;
    *out_windows = num_windows(n_samples);
    return SSYM_OK;
}

int32_t ssym_sound_descriptors(ssym_ctx *ctx, const double *samples, const uint64_t *sample_offsets, uint32_t n_sounds,
                               double rate, double f_min, double f_max, double voicing, uint32_t flags,
                               double *out_max_power, double *out_pitch_conf)
{
    return guarded(ctx, [&]() -> int32_t {
        return run(ctx, "ssym_sound_descriptors", samples, sample_offsets, n_sounds, rate, f_min, f_max, voicing,
                   flags, out_max_power, out_pitch_conf, nullptr, nullptr, nullptr);
    });
}

int32_t ssym_pitch_track(ssym_ctx *ctx, const double *samples, const uint64_t *sample_offsets, uint32_t n_sounds,
                         double rate, double f_min, double f_max, double voicing, uint32_t flags, double *out_freq,
                         double *out_strength, double *out_unvoiced)
{
    return guarded(ctx, [&]() -> int32_t {
        return run(ctx, "ssym_pitch_track", samples, sample_offsets, n_sounds, rate, f_min, f_max, voicing, flags,
                   nullptr, nullptr, out_freq, out_strength, out_unvoiced);
    });
}

}  // extern "C"
