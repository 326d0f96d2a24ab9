// partition.hip -- the partitioner: standardiser, Gaussian mixture (EM), letters, voting experts.
//
// Replaces Partitioner / train_model / discretize / discretize_with_model (src/lib.rs:32-151).  PARITY UNPINNED: the
// reference's arithmetic lives in un-vendored crates (rusty_machine's Standardizer and GaussianMixtureModel, the
// voting_experts crate's cast_votes / split_string), so this file implements the definitions written down in DESIGN.md
// section 5.8, restated independently in numpy by tests/partition_ref.py:
//
//   standardiser  z = (x - mean) / s per column, s the sample standard deviation (n - 1); fitted on the data it
//                 transforms; a column with s == 0 (or n < 2) maps to 0
//   GMM           means = rows init_rows[0..K), every covariance = cov(data) (n - 1) + eps I, weights 1 / K; then up to
//                 max_iters times: E-step (log domain, max subtracted; the constant (2 pi)^(d/2) is DROPPED from every
//                 density, as the crate drops it, so log_lik = sum_i log sum_k pi_k |S_k|^-1/2 exp(-maha / 2)); stop when
//                 |log_lik - previous| < 1e-15 (previous starts at 0); M-step N_k = sum r, pi = N_k / n,
//                 mu = sum r x / N_k, S = sum r (x - mu)(x - mu)^T / N_k + eps I, formed from moments about the
//                 data's column means c (mu = c + delta, S = sum r (x - c)(x - c)^T / N_k - delta delta^T + eps I;
//                 moments about 0 would cancel for large offsets).  A component with N_k == 0 keeps mu and
//                 S and gets weight 0 (the crate would produce NaN).  f64 throughout, Cholesky factors,
//                 log det = 2 sum log L_jj
//   letters       max_index of each posterior row (src/sound.rs:486-495): first strict maximum starting from (0, 0.0)
//   votes         n-grams n = 1..d counted exactly; z-scores per length over the distinct n-grams (population std, 0
//                 when the std is 0); frequency mean / variance from the exact integer sums S1, S2 as
//                 mean = S1 / D, var = S2 / D - mean * mean; boundary entropy H(g) = -sum_c p_c ln p_c over the
//                 successors (p first, then the sum in ascending symbol order); per window s[w..w+d) and split
//                 i = 1..d-1 the frequency expert scores zf(s[w..w+i)) + zf(s[w+i..w+d)), the entropy expert zH(s[w..w+i));
//                 each votes for w + its best i (first maximum); p in 1..N-1 is a boundary when votes[p] >= t,
//                 votes[p] > votes[p-1] and votes[p] >= votes[p+1] (votes[N] = 0)
//
// Mapping.  Column statistics: per-block partial sums over fixed frame chunks, summed over the blocks in block order by
// one finishing kernel (no floating-point atomics anywhere in this file: a second run gives the same bits).  E-step: a
// block walks its chunk in tiles of 32 frames; the means, inverse Cholesky factors and log coefficients of all K
// components sit in LDS when they fit (d = 12, K = 26: 19 KB), else they are read through the same flat pointers from
// global memory; 8 groups of 32 lanes take the components of the tile's frames, one lane per (frame, component)
// Mahalanobis term; then every lane owns a few of the K (d+1)(d+2)/2 moments about the column means c (1, y_i,
// y_i y_j with y = x - c, a second copy of the tile) and adds the tile's
// r-weighted values into the block's private partial slab.  Update: one block per component sums the slabs in block
// order, forms pi, mu, S and re-factors.  Every EM iteration is enqueued up front; a device word makes the iterations
// after convergence return at once, and the host synchronises once per call.  Voting: n-gram codes in base A (first
// symbol most significant) sorted with hipCUB's radix sort, run-length ranks, successor runs by binary search, one
// thread per window with integer atomics for the votes, a scan for the boundaries.
#include "ssym_internal.hpp"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <vector>

struct ssym_gmm {
    uint32_t K = 0, d = 0;
    double eps = 0.0;
    double log_lik = 0.0;
    uint32_t iters = 0;
    double *dev = nullptr;              // [K] weights, [K d] means, [K d d] covariances, [K d(d+1)/2] inverse factors, [K] log coefficients
    std::vector<double> host;           // the same, weights .. covariances (ssym_gmm_get)
};

namespace ssym {

constexpr int kTile = 32;               // frames per E-step tile
constexpr int kGroups = 256 / kTile;    // component groups per tile
constexpr int kMaxDim = 64, kMaxK = 64;
constexpr int kMaxMoments = (kMaxDim + 1) * (kMaxDim + 2) / 2;
constexpr size_t kModelLdsBytes = 24 * 1024;
constexpr size_t kPartialBudget = size_t(64) << 20;

struct GmmLayout {
    int K, d;
    size_t w, mu, cov, linv, logc, total;
    __host__ __device__ explicit GmmLayout(int K_, int d_) : K(K_), d(d_)
    {
        w = 0;
        mu = w + K;
        cov = mu + (size_t)K * d;
        linv = cov + (size_t)K * d * d;
        logc = linv + (size_t)K * d * (d + 1) / 2;
        total = logc + K;
    }
};

// moment table: entry m = (i | j << 8), i <= j <= d, column d of a frame is the constant 1; ordered j-major so that the
// d(d+1)/2 cross products come first, then x_0 .. x_{d-1}, then the constant (N_k)
static std::vector<uint16_t> moment_table(int d)
{
    std::vector<uint16_t> t;
    for (int j = 0; j <= d; ++j)
        for (int i = 0; i <= j; ++i)
            t.push_back((uint16_t)(i | (j << 8)));
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------
// column statistics
// mode 0: sum x_e (e < d); mode 1: sum (x_e - m_e)^2 (e < d); mode 2: sum (x_i - m_i)(x_j - m_j) over the first
// d(d+1)/2 moment-table entries
__global__ __launch_bounds__(256) void colstats_kernel(const double *__restrict__ x, uint64_t n, int d, int mode,
                                                       int E, const double *__restrict__ mean,
                                                       const uint16_t *__restrict__ tab, uint64_t chunk,
                                                       double *__restrict__ part)
{
    __shared__ double red[256];
    const uint64_t f0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t f1 = f0 + chunk < n ? f0 + chunk : n;
    // S lanes per entry take every S-th frame of the chunk; their sums are added in lane order
    const int S = E <= 128 ? 256 / E : 1;
    for (int e0 = 0; e0 < E; e0 += 256 / S) {
        const int e = e0 + threadIdx.x % (256 / S), s = threadIdx.x / (256 / S);
        double acc = 0.0;
        if (e < E && s < S) {
            int i = e, j = e;
            if (mode == 2) {
                i = tab[e] & 0xff;
                j = tab[e] >> 8;
            }
            const double mi = mode ? mean[i] : 0.0, mj = mode ? mean[j] : 0.0;
#pragma unroll 4
            for (uint64_t f = f0 + s; f < f1; f += S) {
                const double a = x[f * d + i];
                acc = __dadd_rn(acc, mode ? __dmul_rn(__dsub_rn(a, mi), __dsub_rn(x[f * d + j], mj)) : a);
            }
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        const int per = 256 / S;
        if ((int)threadIdx.x < per && e0 + (int)threadIdx.x < E) {
            double t = 0.0;
            for (int q = 0; q < S; ++q)
                t = __dadd_rn(t, red[q * per + threadIdx.x]);
            part[(size_t)blockIdx.x * E + e0 + threadIdx.x] = t;
        }
        __syncthreads();
    }
}

// one block: sum the G partials of every entry in block order.  mode 0 -> mean; mode 1 -> standard deviation (n - 1);
// mode 2 -> covariance (n - 1) + eps I written into every one of K covariance slots (the GMM's start)
__global__ __launch_bounds__(256) void colstats_finish_kernel(const double *__restrict__ part, int G, int E, int d,
                                                              int mode, uint64_t n, const uint16_t *__restrict__ tab,
                                                              double eps, int K, double *__restrict__ out)
{
    for (int e = threadIdx.x; e < E; e += blockDim.x) {
        double s = 0.0;
        for (int g = 0; g < G; ++g)
            s = __dadd_rn(s, part[(size_t)g * E + e]);
        if (mode == 0) {
            out[e] = __ddiv_rn(s, (double)n);
        } else if (mode == 1) {
            out[e] = n >= 2 ? sqrt(__ddiv_rn(s, (double)(n - 1))) : 0.0;
        } else {
            const int i = tab[e] & 0xff, j = tab[e] >> 8;
            double c = n >= 2 ? __ddiv_rn(s, (double)(n - 1)) : 0.0;
            if (i == j)
                c = __dadd_rn(c, eps);
            for (int k = 0; k < K; ++k) {
                out[(size_t)k * d * d + (size_t)i * d + j] = c;
                out[(size_t)k * d * d + (size_t)j * d + i] = c;
            }
        }
    }
}

__global__ void standardize_kernel(const double *__restrict__ x, uint64_t n, int d, const double *__restrict__ mean,
                                   const double *__restrict__ sd, double *__restrict__ z)
{
    const uint64_t total = n * (uint64_t)d;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (uint64_t)gridDim.x * blockDim.x) {
        const int j = (int)(q % (uint64_t)d);
        const double s = sd[j];
        z[q] = s > 0.0 ? __ddiv_rn(__dsub_rn(x[q], mean[j]), s) : 0.0;
    }
}

__global__ void gmm_init_kernel(const double *__restrict__ z, int d, int K, const uint64_t *__restrict__ rows,
                                double *__restrict__ model)
{
    const GmmLayout L(K, d);
    for (int q = threadIdx.x; q < K * d; q += blockDim.x) {
        const int k = q / d, j = q % d;
        model[L.mu + q] = z[rows[k] * d + j];
    }
    for (int k = threadIdx.x; k < K; k += blockDim.x)
        model[L.w + k] = __ddiv_rn(1.0, (double)K);
}

// ---------------------------------------------------------------------------------------------------------------------
// E-step.  train: per-block partial slab [A moments of every component, then log_lik] (stride A + 1);
// predict: posteriors (nullable) and letters.
struct EStepArgs {
    const double *x;
    uint64_t n;
    int d, K, M;                  // M = (d+1)(d+2)/2 moments per component
    const double *model;          // GmmLayout
    const double *shift;          // train: [d] the moments are taken about (the data's column means)
    int model_in_lds;
    const uint16_t *tab;
    uint64_t chunk;               // frames per block, a multiple of kTile
    const int *state;             // [0] converged (train only; may be NULL)
    double *part;                 // train
    double *post;                 // predict, nullable
    uint8_t *letters;             // predict, nullable
};

__global__ __launch_bounds__(256) void gmm_estep_kernel(EStepArgs a)
{
    if (a.state && a.state[0])
        return;
    extern __shared__ double lds[];
    const int d = a.d, K = a.K, M = a.M, tid = threadIdx.x;
    const int xs_stride = d + 2, ps_stride = K + 1;
    const bool train = a.part != nullptr;
    double *xs = lds;                                   // [kTile][d + 2]; column d = 1
    double *xc = xs + kTile * xs_stride;                // train: [kTile][d + 2], x - shift; column d = 1
    double *ps = xc + (train ? kTile * xs_stride : 0);  // [kTile][K + 1]: log terms, then posteriors
    double *llt = ps + kTile * ps_stride;               // [kTile]
    uint16_t *tab = (uint16_t *)(llt + kTile);          // [M], padded to doubles below
    double *mlds = llt + kTile + (M + 3) / 4;
    const GmmLayout L(K, d);
    const int P = d * (d + 1) / 2;
    for (int m = tid; m < M; m += 256)
        tab[m] = a.tab[m];
    const double *mu = a.model + L.mu, *linv = a.model + L.linv, *logc = a.model + L.logc;
    if (a.model_in_lds) {
        double *lmu = mlds, *llinv = mlds + K * d, *llogc = llinv + K * P;
        for (int q = tid; q < K * d; q += 256) lmu[q] = mu[q];
        for (int q = tid; q < K * P; q += 256) llinv[q] = linv[q];
        for (int q = tid; q < K; q += 256) llogc[q] = logc[q];
        mu = lmu;
        linv = llinv;
        logc = llogc;
    }
    const int A = K * M;
    double *slab = train ? a.part + (size_t)blockIdx.x * (A + 1) : nullptr;
    if (train)
        for (int q = tid; q < A; q += 256)
            slab[q] = 0.0;
    double llacc = 0.0;
    const uint64_t f0 = (uint64_t)blockIdx.x * a.chunk;
    const uint64_t f1 = f0 + a.chunk < a.n ? f0 + a.chunk : a.n;
    __syncthreads();
    for (uint64_t t0 = f0; t0 < f1; t0 += kTile) {
        for (int q = tid; q < kTile * (d + 1); q += 256) {
            const int f = q / (d + 1), j = q % (d + 1);
            const uint64_t g = t0 + f;
            const double v = g < f1 ? (j < d ? a.x[g * d + j] : 1.0) : 0.0;
            xs[f * xs_stride + j] = v;
            if (train)
                xc[f * xs_stride + j] = g < f1 && j < d ? __dsub_rn(v, a.shift[j]) : v;
        }
        __syncthreads();
        {
            const int f = tid % kTile;
            for (int k = tid / kTile; k < K; k += kGroups) {
                const double *m = mu + (size_t)k * d, *li = linv + (size_t)k * P;
                const double *xf = xs + f * xs_stride;
                double maha = 0.0;
                for (int i = 0, r = 0; i < d; ++i) {
                    double y = 0.0;
                    for (int j = 0; j <= i; ++j, ++r)
                        y = __dadd_rn(y, __dmul_rn(li[r], __dsub_rn(xf[j], m[j])));
                    maha = __dadd_rn(maha, __dmul_rn(y, y));
                }
                ps[f * ps_stride + k] = __dsub_rn(logc[k], __dmul_rn(0.5, maha));
            }
        }
        __syncthreads();
        if (tid < kTile) {
            double *p = ps + tid * ps_stride;
            const uint64_t g = t0 + tid;
            if (g < f1) {
                double mx = p[0];
                for (int k = 1; k < K; ++k)
                    mx = fmax(mx, p[k]);
                double s = 0.0;
                for (int k = 0; k < K; ++k)
                    s = __dadd_rn(s, exp(__dsub_rn(p[k], mx)));
                llt[tid] = __dadd_rn(mx, log(s));
                int best = 0;
                double bv = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double r = __ddiv_rn(exp(__dsub_rn(p[k], mx)), s);
                    p[k] = r;
                    if (r > bv) {
                        bv = r;
                        best = k;
                    }
                    if (a.post)
                        a.post[g * K + k] = r;
                }
                if (a.letters)
                    a.letters[g] = (uint8_t)best;
            } else {
                for (int k = 0; k < K; ++k)
                    p[k] = 0.0;
                llt[tid] = 0.0;
            }
        }
        __syncthreads();
        if (train) {
            if (tid == 0)
                for (int f = 0; f < kTile && t0 + f < f1; ++f)
                    llacc = __dadd_rn(llacc, llt[f]);
            for (int q = tid; q < A; q += 256) {
                const int k = q / M, m = q % M;
                const int i = tab[m] & 0xff, j = tab[m] >> 8;
                double s = 0.0;
                for (int f = 0; f < kTile; ++f)
                    s = __dadd_rn(s, __dmul_rn(ps[f * ps_stride + k], __dmul_rn(xc[f * xs_stride + i], xc[f * xs_stride + j])));
                slab[q] = __dadd_rn(slab[q], s);
            }
        }
        __syncthreads();
    }
    if (train && tid == 0)
        slab[A] = llacc;
}

// ---------------------------------------------------------------------------------------------------------------------
// update (one block per component).  it < 0: factor the start (covariances and weights as written);
// it >= 0: iteration `it`'s convergence test and M-step.  state: [0] converged, [1] iterations, [2] factorisation failed;
// llh[it] = the log-likelihood stored before iteration it (llh[0] = 0).
__global__ __launch_bounds__(256) void gmm_update_kernel(double *__restrict__ model, int K, int d, int M,
                                                         const double *__restrict__ part,
                                                         const double *__restrict__ shift, int G, uint64_t n,
                                                         double eps, int it, int *__restrict__ state,
                                                         double *__restrict__ llh)
{
    __shared__ double S[kMaxMoments];
    __shared__ double C[kMaxDim * (kMaxDim + 1)];
    __shared__ double dl[kMaxDim];
    __shared__ int flag;
    const int k = blockIdx.x, tid = threadIdx.x, cs = d + 1;
    const GmmLayout L(K, d);
    const int P = d * (d + 1) / 2, A = K * M;
    double pi;
    if (it >= 0) {
        if (state[0])
            return;
        if (tid == 0) {
            double ll = 0.0;
            for (int g = 0; g < G; ++g)
                ll = __dadd_rn(ll, part[(size_t)g * (A + 1) + A]);
            const double prev = llh[it];
            flag = fabs(__dsub_rn(ll, prev)) < 1e-15;
            if (k == 0) {
                if (flag) {
                    state[0] = 1;
                } else {
                    llh[it + 1] = ll;
                    state[1] = it + 1;
                }
            }
        }
        __syncthreads();
        if (flag)
            return;
        for (int m = tid; m < M; m += 256) {
            double s = 0.0;
            for (int g = 0; g < G; ++g)
                s = __dadd_rn(s, part[(size_t)g * (A + 1) + (size_t)k * M + m]);
            S[m] = s;
        }
        __syncthreads();
        const double Nk = S[M - 1];
        if (Nk == 0.0) {
            if (tid == 0) {
                model[L.w + k] = 0.0;
                model[L.logc + k] = -INFINITY;
            }
            return;
        }
        // the slabs hold moments about c = shift: mu = c + delta, delta = sum r (x - c) / N_k,
        // S = sum r (x - c)(x - c)^T / N_k - delta delta^T + eps I (no cancellation against |c|)
        for (int i = tid; i < d; i += 256) {
            dl[i] = __ddiv_rn(S[P + i], Nk);
            model[L.mu + (size_t)k * d + i] = __dadd_rn(shift[i], dl[i]);
        }
        __syncthreads();
        for (int e = tid; e < P; e += 256) {
            // moment-table order: j-major, i <= j
            int j = 0;
            while ((j + 1) * (j + 2) / 2 <= e)
                ++j;
            const int i = e - j * (j + 1) / 2;
            double c = __dsub_rn(__ddiv_rn(S[e], Nk), __dmul_rn(dl[i], dl[j]));
            if (i == j)
                c = __dadd_rn(c, eps);
            C[i * cs + j] = c;
            C[j * cs + i] = c;
            model[L.cov + (size_t)k * d * d + (size_t)i * d + j] = c;
            model[L.cov + (size_t)k * d * d + (size_t)j * d + i] = c;
        }
        pi = __ddiv_rn(Nk, (double)n);
        if (tid == 0)
            model[L.w + k] = pi;
    } else {
        for (int q = tid; q < d * d; q += 256)
            C[(q / d) * cs + q % d] = model[L.cov + (size_t)k * d * d + q];
        pi = model[L.w + k];
    }
    __syncthreads();
    // Cholesky, right-looking, lower triangle of C in place
    for (int j = 0; j < d; ++j) {
        if (tid == 0) {
            const double v = C[j * cs + j];
            if (!(v > 0.0)) {
                state[2] = 1;
                state[0] = 1;
            }
            C[j * cs + j] = v > 0.0 ? sqrt(v) : 1.0;
        }
        __syncthreads();
        for (int i = j + 1 + tid; i < d; i += 256)
            C[i * cs + j] = __ddiv_rn(C[i * cs + j], C[j * cs + j]);
        __syncthreads();
        const int r = d - 1 - j;           // trailing size
        for (int q = tid; q < r * r; q += 256) {
            const int i = j + 1 + q / r, l = j + 1 + q % r;
            if (l <= i)
                C[i * cs + l] = __dsub_rn(C[i * cs + l], __dmul_rn(C[i * cs + j], C[l * cs + j]));
        }
        __syncthreads();
    }
    // inverse factor, one column per lane (forward substitution), packed rows into S
    for (int c = tid; c < d; c += 256) {
        for (int i = c; i < d; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int j = c; j < i; ++j)
                s = __dsub_rn(s, __dmul_rn(C[i * cs + j], S[j * (j + 1) / 2 + c]));
            S[i * (i + 1) / 2 + c] = __ddiv_rn(s, C[i * cs + i]);
        }
    }
    __syncthreads();
    for (int q = tid; q < P; q += 256)
        model[L.linv + (size_t)k * P + q] = S[q];
    if (tid == 0) {
        double ld = 0.0;
        for (int j = 0; j < d; ++j)
            ld = __dadd_rn(ld, log(C[j * cs + j]));
        model[L.logc + k] = __dsub_rn(log(pi), ld);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// voting experts
__global__ void ngram_encode_kernel(const uint8_t *__restrict__ s, uint32_t N, int n, uint64_t A,
                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ pos)
{
    const uint32_t W = N - n + 1;
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        uint64_t c = 0;
        for (int q = 0; q < n; ++q)
            c = c * A + s[w + q];
        keys[w] = c;
        pos[w] = w;
    }
}

__global__ void ngram_heads_kernel(const uint64_t *__restrict__ keys, uint32_t W, uint32_t *__restrict__ flags)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += gridDim.x * blockDim.x)
        flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// sorted keys + their positions + inclusive scan of the head flags -> rank of every window, distinct keys, head index
__global__ void ngram_runs_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ pos,
                                  const uint32_t *__restrict__ scan, uint32_t W, uint32_t *__restrict__ rank,
                                  uint64_t *__restrict__ ukey, uint32_t *__restrict__ head)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += gridDim.x * blockDim.x) {
        const uint32_t r = scan[i] - 1;
        rank[pos[i]] = r;
        if (i == 0 || keys[i] != keys[i - 1]) {
            ukey[r] = keys[i];
            head[r] = i;
        }
    }
}

__global__ void ngram_counts_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ scan, uint32_t W,
                                    uint32_t *__restrict__ cnt, uint32_t *__restrict__ Dn)
{
    const uint32_t D = scan[W - 1];
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *Dn = D;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < D; r += gridDim.x * blockDim.x)
        cnt[r] = (r + 1 < D ? head[r + 1] : W) - head[r];
}

__device__ __forceinline__ uint32_t lower_bound_u64(const uint64_t *a, uint32_t n, uint64_t v)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// boundary entropy of every distinct n-gram (successors = the (n+1)-grams [g A, g A + A))
__global__ void ngram_entropy_kernel(const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ Dn,
                                     const uint64_t *__restrict__ ukey1, const uint32_t *__restrict__ cnt1,
                                     const uint32_t *__restrict__ Dn1, uint64_t A, double *__restrict__ H)
{
    const uint32_t D = *Dn, D1 = *Dn1;
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < D; u += gridDim.x * blockDim.x) {
        const uint64_t lo = ukey[u] * A;
        const uint32_t b = lower_bound_u64(ukey1, D1, lo);
        uint32_t e = b;
        uint64_t total = 0;
        while (e < D1 && ukey1[e] < lo + A)
            total += cnt1[e++];
        double s = 0.0;
        for (uint32_t q = b; q < e; ++q) {
            const double p = __ddiv_rn((double)cnt1[q], (double)total);
            s = __dadd_rn(s, __dmul_rn(p, log(p)));
        }
        H[u] = -s;
    }
}

// one block per length n = 1 .. d-1: [meanF, stdF, meanH, stdH]
__global__ __launch_bounds__(256) void ngram_stats_kernel(uint32_t N, uint32_t maxN, const uint32_t *__restrict__ cnt,
                                                          const double *__restrict__ H,
                                                          const uint32_t *__restrict__ Dn,
                                                          double *__restrict__ stats)
{
    __shared__ unsigned long long su[256];
    __shared__ double sd[256];
    const int n = blockIdx.x + 1, tid = threadIdx.x;
    const uint32_t D = Dn[n - 1];
    const uint32_t *c = cnt + (size_t)(n - 1) * maxN;
    const double *h = H + (size_t)(n - 1) * maxN;
    unsigned long long s2 = 0;
    double sh = 0.0;
    for (uint32_t u = tid; u < D; u += 256) {
        s2 += (unsigned long long)c[u] * c[u];
        sh = __dadd_rn(sh, h[u]);
    }
    su[tid] = s2;
    sd[tid] = sh;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            su[tid] += su[tid + w];
            sd[tid] = __dadd_rn(sd[tid], sd[tid + w]);
        }
        __syncthreads();
    }
    const double Dd = (double)D;
    const double meanH = __ddiv_rn(sd[0], Dd);
    const unsigned long long S2 = su[0];
    __syncthreads();
    double sv = 0.0;
    for (uint32_t u = tid; u < D; u += 256) {
        const double q = __dsub_rn(h[u], meanH);
        sv = __dadd_rn(sv, __dmul_rn(q, q));
    }
    sd[tid] = sv;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
            sd[tid] = __dadd_rn(sd[tid], sd[tid + w]);
        __syncthreads();
    }
    if (tid == 0) {
        const double S1 = (double)(N - n + 1);
        const double meanF = __ddiv_rn(S1, Dd);
        const double varF = __dsub_rn(__ddiv_rn((double)S2, Dd), __dmul_rn(meanF, meanF));
        const double varH = __ddiv_rn(sd[0], Dd);
        double *o = stats + 4 * (n - 1);
        o[0] = meanF;
        o[1] = varF > 0.0 ? sqrt(varF) : 0.0;
        o[2] = meanH;
        o[3] = varH > 0.0 ? sqrt(varH) : 0.0;
    }
}

__device__ __forceinline__ double zscore(double v, double mean, double sd)
{
    return sd > 0.0 ? __ddiv_rn(__dsub_rn(v, mean), sd) : 0.0;
}

__global__ void vote_kernel(uint32_t N, int depth, uint32_t maxN, const uint32_t *__restrict__ rank,
                            const uint32_t *__restrict__ cnt, const double *__restrict__ H,
                            const double *__restrict__ stats, uint32_t *__restrict__ votesF,
                            uint32_t *__restrict__ votesH)
{
    const uint32_t W = N - depth + 1;
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        int bf = 1, bh = 1;
        double vf = 0.0, vh = 0.0;
        for (int i = 1; i < depth; ++i) {
            const int j = depth - i;
            const double *si = stats + 4 * (i - 1), *sj = stats + 4 * (j - 1);
            const uint32_t ri = rank[(size_t)(i - 1) * maxN + w], rj = rank[(size_t)(j - 1) * maxN + w + i];
            const double zf = __dadd_rn(zscore((double)cnt[(size_t)(i - 1) * maxN + ri], si[0], si[1]),
                                        zscore((double)cnt[(size_t)(j - 1) * maxN + rj], sj[0], sj[1]));
            const double zh = zscore(H[(size_t)(i - 1) * maxN + ri], si[2], si[3]);
            if (i == 1 || zf > vf) {
                vf = zf;
                bf = i;
            }
            if (i == 1 || zh > vh) {
                vh = zh;
                bh = i;
            }
        }
        atomicAdd(votesF + w + bf, 1u);
        atomicAdd(votesH + w + bh, 1u);
    }
}

__global__ void boundary_kernel(uint32_t N, uint32_t t, const uint32_t *__restrict__ vf, const uint32_t *__restrict__ vh,
                                uint32_t *__restrict__ flags)
{
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x) {
        uint32_t f = 0;
        if (p >= 1) {
            const uint32_t v = vf[p] + vh[p], prev = vf[p - 1] + vh[p - 1];
            const uint32_t next = p + 1 < N ? vf[p + 1] + vh[p + 1] : 0u;
            f = (v >= t && v > prev && v >= next) ? 1u : 0u;
        }
        flags[p] = f;
    }
}

__global__ void boundary_pos_kernel(uint32_t N, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ scan,
                                    uint32_t *__restrict__ bpos)
{
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x)
        if (flags[p])
            bpos[scan[p] - 1] = p;
}

// out[0] = segments, out[1 + s] = frames of segment s
__global__ void segment_len_kernel(uint32_t N, const uint32_t *__restrict__ scan, const uint32_t *__restrict__ bpos,
                                   uint32_t *__restrict__ out)
{
    const uint32_t m = scan[N - 1];
    if (blockIdx.x == 0 && threadIdx.x == 0)
        out[0] = m + 1;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s <= m; s += gridDim.x * blockDim.x) {
        const uint32_t a = s == 0 ? 0u : bpos[s - 1], b = s < m ? bpos[s] : N;
        out[1 + s] = b - a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

// a set of device blocks freed together
struct Scratch {
    ssym_ctx *ctx;
    std::vector<void *> blocks;
    explicit Scratch(ssym_ctx *c) : ctx(c) {}
    ~Scratch()
    {
        for (void *p : blocks)
            dev_free(ctx, p);
    }
    template <class T>
    int32_t get(T **p, size_t count)
    {
        void *q = nullptr;
        const int32_t rc = dev_alloc(ctx, &q, count * sizeof(T) > 0 ? count * sizeof(T) : 8);
        if (rc == SSYM_OK)
            blocks.push_back(q);
        *p = (T *)q;
        return rc;
    }
};

#define SSYM_TRY(expr)                         \
    do {                                       \
        const int32_t rc__ = (expr);           \
        if (rc__ != SSYM_OK)                   \
            return rc__;                       \
    } while (0)

static unsigned grid_for(const ssym_ctx *ctx, uint64_t work, unsigned block = 256)
{
    const uint64_t g = (work + block - 1) / block;
    const uint64_t cap = (uint64_t)ctx->num_cus * 8;
    return (unsigned)(g < 1 ? 1 : (g < cap ? g : cap));
}

// frames-per-block chunking of the column statistics and the E-step
static void chunking(const ssym_ctx *ctx, uint64_t n, size_t slab_doubles, int *G, uint64_t *chunk)
{
    uint64_t g = (n + kTile - 1) / kTile;
    g = std::min<uint64_t>(g, (uint64_t)ctx->num_cus * 2);
    g = std::min<uint64_t>(g, std::max<uint64_t>(1, kPartialBudget / (slab_doubles * sizeof(double))));
    g = std::max<uint64_t>(g, 1);
    uint64_t c = (n + g - 1) / g;
    c = (c + kTile - 1) / kTile * kTile;
    *G = (int)((n + c - 1) / std::max<uint64_t>(c, 1));
    if (*G < 1)
        *G = 1;
    *chunk = std::max<uint64_t>(c, kTile);
}

// column statistics of x -> mean (mode 0), sd (mode 1) or the GMM's start covariances (mode 2)
static int32_t column_pass(ssym_ctx *ctx, Scratch &sc, const double *x, uint64_t n, int d, int mode,
                           const double *mean, const uint16_t *tab, double eps, int K, double *out)
{
    const int E = mode == 2 ? d * (d + 1) / 2 : d;
    int G;
    uint64_t chunk;
    chunking(ctx, n, E, &G, &chunk);
    double *part = nullptr;
    SSYM_TRY(sc.get(&part, (size_t)G * E));
    colstats_kernel<<<G, 256, 0, ctx->stream>>>(x, n, d, mode, E, mean, tab, chunk, part);
    colstats_finish_kernel<<<1, 256, 0, ctx->stream>>>(part, G, E, d, mode, n, tab, eps, K, out);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

// x (device) -> z (device), statistics fitted on x
static int32_t standardize_dev(ssym_ctx *ctx, Scratch &sc, const double *x, uint64_t n, int d, double *z)
{
    double *st = nullptr;
    SSYM_TRY(sc.get(&st, 2 * (size_t)d));
    SSYM_TRY(column_pass(ctx, sc, x, n, d, 0, nullptr, nullptr, 0.0, 0, st));
    SSYM_TRY(column_pass(ctx, sc, x, n, d, 1, st, nullptr, 0.0, 0, st + d));
    standardize_kernel<<<grid_for(ctx, n * d), 256, 0, ctx->stream>>>(x, n, d, st, st + d, z);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

// features onto the device (a copy when they are host memory)
static int32_t device_feats(ssym_ctx *ctx, Scratch &sc, const double *feats, uint64_t count, bool on_device,
                            const double **out)
{
    if (on_device) {
        *out = feats;
        return SSYM_OK;
    }
    double *p = nullptr;
    SSYM_TRY(sc.get(&p, count));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(p, feats, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    *out = p;
    return SSYM_OK;
}

static int32_t upload_table(ssym_ctx *ctx, Scratch &sc, int d, uint16_t **tab)
{
    const std::vector<uint16_t> t = moment_table(d);
    SSYM_TRY(sc.get(tab, t.size()));
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(*tab, t.data(), t.size() * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    return SSYM_OK;
}

static size_t estep_lds(int d, int K, int M, bool model_in_lds, bool train)
{
    const GmmLayout L(K, d);
    size_t dbl = (size_t)kTile * (d + 2) * (train ? 2 : 1) + (size_t)kTile * (K + 1) + kTile + (M + 3) / 4;
    if (model_in_lds)
        dbl += L.total - L.mu - (size_t)K * d * d;   // means, inverse factors, log coefficients
    return dbl * sizeof(double);
}

static bool model_fits_lds(int d, int K)
{
    const size_t P = (size_t)d * (d + 1) / 2;
    return ((size_t)K * d + (size_t)K * P + K) * sizeof(double) <= kModelLdsBytes;
}

static int32_t launch_estep(ssym_ctx *ctx, EStepArgs a, int G)
{
    const bool in_lds = model_fits_lds(a.d, a.K);
    a.model_in_lds = in_lds ? 1 : 0;
    const size_t lds = estep_lds(a.d, a.K, a.M, in_lds, a.part != nullptr);
    gmm_estep_kernel<<<G, 256, lds, ctx->stream>>>(a);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

// predict on device data (already standardised when asked): letters (device) and posteriors (device, nullable)
static int32_t predict_dev(ssym_ctx *ctx, Scratch &sc, const ssym_gmm *gmm, const double *z, uint64_t n,
                           double *post, uint8_t *letters)
{
    const int d = (int)gmm->d, K = (int)gmm->K, M = (d + 1) * (d + 2) / 2;
    uint16_t *tab = nullptr;
    SSYM_TRY(upload_table(ctx, sc, d, &tab));
    int G;
    uint64_t chunk;
    chunking(ctx, n, 1, &G, &chunk);
    EStepArgs a{z, n, d, K, M, gmm->dev, nullptr, 0, tab, chunk, nullptr, nullptr, post, letters};
    return launch_estep(ctx, a, G);
}

static bool pow_too_large(uint64_t A, uint32_t depth)
{
    unsigned __int128 v = 1;
    for (uint32_t q = 0; q < depth; ++q) {
        v *= A;
        if (v >= ((unsigned __int128)1 << 63))
            return true;
    }
    return false;
}

// voting experts on device symbols; result words (count, lengths) land in `res` (device, N + 1 words);
// votes (device, nullable) = [frequency expert N + 1][entropy expert N + 1]
static int32_t vote_dev(ssym_ctx *ctx, Scratch &sc, const uint8_t *sym, uint32_t N, uint32_t A, uint32_t depth,
                        uint32_t threshold, uint32_t *res, uint32_t *votes)
{
    hipStream_t st = ctx->stream;
    const uint32_t maxN = N;
    const int dd = (int)depth;
    uint64_t *kA, *kB, *ukey;
    uint32_t *pA, *pB, *flags, *scan, *rank, *cnt, *Dn, *vbuf, *bpos;
    double *H, *stats;
    SSYM_TRY(sc.get(&kA, maxN));
    SSYM_TRY(sc.get(&kB, maxN));
    SSYM_TRY(sc.get(&pA, maxN));
    SSYM_TRY(sc.get(&pB, maxN));
    SSYM_TRY(sc.get(&flags, maxN + 1));
    SSYM_TRY(sc.get(&scan, maxN + 1));
    SSYM_TRY(sc.get(&rank, (size_t)dd * maxN));
    SSYM_TRY(sc.get(&cnt, (size_t)dd * maxN));
    SSYM_TRY(sc.get(&ukey, (size_t)dd * maxN));
    SSYM_TRY(sc.get(&Dn, (size_t)dd));
    SSYM_TRY(sc.get(&H, (size_t)(dd - 1) * maxN));
    SSYM_TRY(sc.get(&stats, 4 * (size_t)(dd - 1)));
    SSYM_TRY(sc.get(&bpos, maxN));
    if (!votes) {
        SSYM_TRY(sc.get(&vbuf, 2 * (size_t)(maxN + 1)));
        votes = vbuf;
    }
    size_t sortBytes = 0, scanBytes = 0;
    SSYM_HIP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes, kA, kB, pA, pB, (int)N, 0, 64, st));
    SSYM_HIP_CHECK(ctx, hipcub::DeviceScan::InclusiveSum(nullptr, scanBytes, flags, scan, (int)N, st));
    void *temp = nullptr;
    size_t tempBytes = std::max(sortBytes, scanBytes);
    SSYM_TRY(sc.get((char **)&temp, tempBytes));
    for (int n = 1; n <= dd; ++n) {
        const uint32_t W = N - n + 1;
        int bits = 0;
        {
            unsigned __int128 v = 1;
            for (int q = 0; q < n; ++q) v *= A;
            while (((unsigned __int128)1 << bits) < v) ++bits;
            bits = std::max(bits, 1);
        }
        const unsigned g = grid_for(ctx, W);
        ngram_encode_kernel<<<g, 256, 0, st>>>(sym, N, n, A, kA, pA);
        size_t tb = tempBytes;
        SSYM_HIP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(temp, tb, kA, kB, pA, pB, (int)W, 0, bits, st));
        ngram_heads_kernel<<<g, 256, 0, st>>>(kB, W, flags);
        tb = tempBytes;
        SSYM_HIP_CHECK(ctx, hipcub::DeviceScan::InclusiveSum(temp, tb, flags, scan, (int)W, st));
        uint32_t *rk = rank + (size_t)(n - 1) * maxN, *ct = cnt + (size_t)(n - 1) * maxN;
        uint64_t *uk = ukey + (size_t)(n - 1) * maxN;
        ngram_runs_kernel<<<g, 256, 0, st>>>(kB, pB, scan, W, rk, uk, flags /* head index, flags are spent */);
        ngram_counts_kernel<<<g, 256, 0, st>>>(flags, scan, W, ct, Dn + (n - 1));
        SSYM_HIP_CHECK(ctx, hipGetLastError());
    }
    for (int n = 1; n < dd; ++n)
        ngram_entropy_kernel<<<grid_for(ctx, N - n + 1), 256, 0, st>>>(
            ukey + (size_t)(n - 1) * maxN, Dn + (n - 1), ukey + (size_t)n * maxN, cnt + (size_t)n * maxN, Dn + n,
            A, H + (size_t)(n - 1) * maxN);
    ngram_stats_kernel<<<dd - 1, 256, 0, st>>>(N, maxN, cnt, H, Dn, stats);
    SSYM_TRY(zero_words(ctx, votes, 2 * (size_t)(maxN + 1) * sizeof(uint32_t)));
    vote_kernel<<<grid_for(ctx, N - dd + 1), 256, 0, st>>>(N, dd, maxN, rank, cnt, H, stats, votes, votes + maxN + 1);
    boundary_kernel<<<grid_for(ctx, N), 256, 0, st>>>(N, threshold, votes, votes + maxN + 1, flags);
    size_t tb = tempBytes;
    SSYM_HIP_CHECK(ctx, hipcub::DeviceScan::InclusiveSum(temp, tb, flags, scan, (int)N, st));
    boundary_pos_kernel<<<grid_for(ctx, N), 256, 0, st>>>(N, flags, scan, bpos);
    segment_len_kernel<<<grid_for(ctx, N), 256, 0, st>>>(N, scan, bpos, res);
    SSYM_HIP_CHECK(ctx, hipGetLastError());
    return SSYM_OK;
}

// validation shared by the voting entry points; *trivial = 1 when no device work is needed (n < depth)
static int32_t vote_args(ssym_ctx *ctx, const char *fn, uint64_t n, uint32_t alphabet, uint32_t depth,
                         const void *out_seg, const uint64_t *n_segments)
{
    if (!out_seg || !n_segments) {
        ctx->err = std::string(fn) + ": NULL buffer";
        return SSYM_E_INVALID;
    }
    if (depth < 2 || alphabet < 2 || alphabet > 256) {
        ctx->err = std::string(fn) + ": need depth >= 2 and 2 <= alphabet <= 256";
        return SSYM_E_INVALID;
    }
    if (pow_too_large(alphabet, depth)) {
        ctx->err = std::string(fn) + ": alphabet^depth must stay below 2^63";
        return SSYM_E_INVALID;
    }
    if (n >= (uint64_t)1 << 31) {
        ctx->err = std::string(fn) + ": at most 2^31 - 1 symbols";
        return SSYM_E_INVALID;
    }
    return SSYM_OK;
}

// the answer without device work: n < depth (no window) -> one segment of n (none when n == 0), no votes
static void vote_trivial(uint64_t n, uint32_t *out_votes, uint64_t *out_seg, uint64_t *n_segments)
{
    if (out_votes)
        for (uint64_t q = 0; q < 2 * (n + 1); ++q)
            out_votes[q] = 0;
    *n_segments = n ? 1 : 0;
    if (n)
        out_seg[0] = n;
}

// device result words -> the caller's segment lengths (one copy, one synchronisation)
static int32_t finish_votes(ssym_ctx *ctx, const uint32_t *res_dev, uint32_t N, const uint32_t *votes_dev,
                            uint32_t *out_votes, uint64_t *out_seg, uint64_t *n_segments)
{
    std::vector<uint32_t> res(N + 1);
    SSYM_HIP_CHECK(ctx, hipMemcpyAsync(res.data(), res_dev, (N + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out_votes)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_votes, votes_dev, 2 * (size_t)(N + 1) * sizeof(uint32_t),
                                           hipMemcpyDeviceToHost, ctx->stream));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t m = res[0];
    if (m < 1 || m > N) {
        ctx->err = "voting: inconsistent segment count";
        return SSYM_E_HIP;
    }
    *n_segments = m;
    for (uint32_t s = 0; s < m; ++s)
        out_seg[s] = res[1 + s];
    return SSYM_OK;
}

}  // namespace ssym

using namespace ssym;

extern "C" {

int32_t ssym_standardize(ssym_ctx *ctx, const double *feats, uint64_t n_frames, uint32_t dim, uint32_t flags,
                         double *out)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (dim == 0 || dim > kMaxDim) {
        ctx->err = "ssym_standardize: need 1 <= dim <= 64";
        return SSYM_E_INVALID;
    }
    if (n_frames == 0)
        return SSYM_OK;
    if (!feats || !out) {
        ctx->err = "ssym_standardize: NULL buffer";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const bool dev = (flags & SSYM_OUT_DEVICE) != 0;
    const uint64_t count = n_frames * dim;
    Scratch sc(ctx);
    const double *x = nullptr;
    SSYM_TRY(device_feats(ctx, sc, feats, count, dev, &x));
    double *z = out;
    if (!dev)
        SSYM_TRY(sc.get(&z, count));
    SSYM_TRY(standardize_dev(ctx, sc, x, n_frames, (int)dim, z));
    if (!dev)
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out, z, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SSYM_OK;
    });
}

int32_t ssym_gmm_train(ssym_ctx *ctx, const double *feats, uint64_t n_frames, uint32_t dim, uint32_t n_components,
                       const uint64_t *init_rows, double eps, uint32_t max_iters, uint32_t flags, ssym_gmm **out)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (!out || !feats || !init_rows) {
        ctx->err = "ssym_gmm_train: NULL buffer";
        return SSYM_E_INVALID;
    }
    *out = nullptr;
    if (dim == 0 || dim > kMaxDim || n_components == 0 || n_components > kMaxK) {
        ctx->err = "ssym_gmm_train: need 1 <= dim <= 64 and 1 <= n_components <= 64";
        return SSYM_E_INVALID;
    }
    if (n_frames < n_components) {
        ctx->err = "ssym_gmm_train: n_frames < n_components";
        return SSYM_E_INVALID;
    }
    if (!(eps >= 0.0) || !std::isfinite(eps)) {
        ctx->err = "ssym_gmm_train: eps must be finite and >= 0";
        return SSYM_E_INVALID;
    }
    for (uint32_t k = 0; k < n_components; ++k)
        if (init_rows[k] >= n_frames) {
            ctx->err = "ssym_gmm_train: init_rows out of range";
            return SSYM_E_INVALID;
        }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int d = (int)dim, K = (int)n_components, M = (d + 1) * (d + 2) / 2, A = K * M;
    const GmmLayout L(K, d);
    Scratch sc(ctx);
    const double *x = nullptr;
    SSYM_TRY(device_feats(ctx, sc, feats, n_frames * dim, (flags & SSYM_OUT_DEVICE) != 0, &x));
    const double *z = x;
    if (flags & SSYM_GMM_STANDARDIZE) {
        double *zz = nullptr;
        SSYM_TRY(sc.get(&zz, n_frames * dim));
        SSYM_TRY(standardize_dev(ctx, sc, x, n_frames, d, zz));
        z = zz;
    }
    ssym_gmm *g = new ssym_gmm();
    g->K = K;
    g->d = d;
    g->eps = eps;
    int32_t rc = dev_alloc(ctx, (void **)&g->dev, L.total * sizeof(double));
    if (rc != SSYM_OK) {
        delete g;
        return rc;
    }
    auto fail = [&](int32_t r) {
        dev_free(ctx, g->dev);
        delete g;
        return r;
    };
    uint16_t *tab = nullptr;
    uint64_t *rows = nullptr;
    double *mean = nullptr, *llh = nullptr, *part = nullptr;
    int *state = nullptr;
    int G;
    uint64_t chunk;
    chunking(ctx, n_frames, (size_t)A + 1, &G, &chunk);
    if ((rc = upload_table(ctx, sc, d, &tab)) != SSYM_OK || (rc = sc.get(&rows, K)) != SSYM_OK ||
        (rc = sc.get(&mean, d)) != SSYM_OK || (rc = sc.get(&llh, (size_t)max_iters + 2)) != SSYM_OK ||
        (rc = sc.get(&state, 4)) != SSYM_OK || (rc = sc.get(&part, (size_t)G * (A + 1))) != SSYM_OK)
        return fail(rc);
    hipError_t e = hipMemcpyAsync(rows, init_rows, K * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
        ctx->err = std::string("ssym_gmm_train: ") + hipGetErrorString(e);
        return fail(SSYM_E_HIP);
    }
    if ((rc = zero_words(ctx, state, 4 * sizeof(int))) != SSYM_OK ||
        (rc = zero_words(ctx, llh, ((size_t)max_iters + 2) * sizeof(double))) != SSYM_OK)
        return fail(rc);
    // start: means = init rows, weights 1 / K, covariances = cov(z) + eps I, factored
    if ((rc = column_pass(ctx, sc, z, n_frames, d, 0, nullptr, nullptr, 0.0, 0, mean)) != SSYM_OK ||
        (rc = column_pass(ctx, sc, z, n_frames, d, 2, mean, tab, eps, K, g->dev + L.cov)) != SSYM_OK)
        return fail(rc);
    gmm_init_kernel<<<1, 256, 0, st>>>(z, d, K, rows, g->dev);
    gmm_update_kernel<<<K, 256, 0, st>>>(g->dev, K, d, M, part, mean, G, n_frames, eps, -1, state, llh);
    // the moments are taken about the column means (mean), so the M-step does not cancel against large offsets
    for (uint32_t it = 0; it < max_iters; ++it) {
        EStepArgs a{z, n_frames, d, K, M, g->dev, mean, 0, tab, chunk, state, part, nullptr, nullptr};
        if ((rc = launch_estep(ctx, a, G)) != SSYM_OK)
            return fail(rc);
        gmm_update_kernel<<<K, 256, 0, st>>>(g->dev, K, d, M, part, mean, G, n_frames, eps, (int)it, state, llh);
    }
    e = hipGetLastError();
    g->host.resize(L.linv);
    int hstate[4] = {0, 0, 0, 0};
    std::vector<double> hllh((size_t)max_iters + 2);
    if (e == hipSuccess)
        e = hipMemcpyAsync(g->host.data(), g->dev, L.linv * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(hstate, state, sizeof(hstate), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(hllh.data(), llh, hllh.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        ctx->err = std::string("ssym_gmm_train: ") + hipGetErrorString(e);
        return fail(SSYM_E_HIP);
    }
    if (hstate[2]) {
        ctx->err = "ssym_gmm_train: a covariance is not positive definite (raise eps or pick other init_rows)";
        return fail(SSYM_E_INVALID);
    }
    g->iters = (uint32_t)hstate[1];
    g->log_lik = hllh[g->iters];
    *out = g;
    return SSYM_OK;
    });
}

int32_t ssym_gmm_get(const ssym_gmm *gmm, double *weights, double *means, double *covs, double *log_lik,
                     uint32_t *iters)
{
    if (!gmm)
        return SSYM_E_INVALID;
    const GmmLayout L((int)gmm->K, (int)gmm->d);
    if (weights)
        std::copy(gmm->host.begin() + L.w, gmm->host.begin() + L.mu, weights);
    if (means)
        std::copy(gmm->host.begin() + L.mu, gmm->host.begin() + L.cov, means);
    if (covs)
        std::copy(gmm->host.begin() + L.cov, gmm->host.begin() + L.linv, covs);
    if (log_lik)
        *log_lik = gmm->log_lik;
    if (iters)
        *iters = gmm->iters;
    return SSYM_OK;
}

int32_t ssym_gmm_destroy(ssym_ctx *ctx, ssym_gmm *gmm)
{
    if (!gmm)
        return SSYM_OK;
    dev_free(ctx, gmm->dev);
    delete gmm;
    return SSYM_OK;
}

int32_t ssym_gmm_predict(ssym_ctx *ctx, const ssym_gmm *gmm, const double *feats, uint64_t n_frames, uint32_t flags,
                         double *out_post, uint8_t *out_letters)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (!gmm) {
        ctx->err = "ssym_gmm_predict: NULL model";
        return SSYM_E_INVALID;
    }
    if (n_frames == 0)
        return SSYM_OK;
    if (!feats || !out_letters) {
        ctx->err = "ssym_gmm_predict: NULL buffer";
        return SSYM_E_INVALID;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool dev = (flags & SSYM_OUT_DEVICE) != 0;
    const int d = (int)gmm->d, K = (int)gmm->K;
    Scratch sc(ctx);
    const double *x = nullptr;
    SSYM_TRY(device_feats(ctx, sc, feats, n_frames * d, dev, &x));
    if (flags & SSYM_GMM_STANDARDIZE) {
        double *zz = nullptr;
        SSYM_TRY(sc.get(&zz, n_frames * d));
        SSYM_TRY(standardize_dev(ctx, sc, x, n_frames, d, zz));
        x = zz;
    }
    double *post = out_post;
    uint8_t *let = out_letters;
    if (!dev) {
        if (out_post)
            SSYM_TRY(sc.get(&post, n_frames * K));
        SSYM_TRY(sc.get(&let, n_frames));
    }
    SSYM_TRY(predict_dev(ctx, sc, gmm, x, n_frames, post, let));
    if (!dev) {
        if (out_post)
            SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_post, post, n_frames * K * sizeof(double), hipMemcpyDeviceToHost, st));
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(out_letters, let, n_frames, hipMemcpyDeviceToHost, st));
    }
    SSYM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return SSYM_OK;
    });
}

int32_t ssym_vote_segments(ssym_ctx *ctx, const uint8_t *symbols, uint64_t n, uint32_t alphabet, uint32_t depth,
                           uint32_t threshold, uint32_t flags, uint32_t *out_votes, uint64_t *out_seg_frames,
                           uint64_t *n_segments)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    SSYM_TRY(vote_args(ctx, "ssym_vote_segments", n, alphabet, depth, out_seg_frames, n_segments));
    if (n && !symbols) {
        ctx->err = "ssym_vote_segments: NULL buffer";
        return SSYM_E_INVALID;
    }
    const bool dev = (flags & SSYM_OUT_DEVICE) != 0;
    if (!dev)
        for (uint64_t q = 0; q < n; ++q)
            if (symbols[q] >= alphabet) {
                ctx->err = "ssym_vote_segments: a symbol is >= alphabet";
                return SSYM_E_INVALID;
            }
    if (n < depth) {
        vote_trivial(n, out_votes, out_seg_frames, n_segments);
        return SSYM_OK;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t N = (uint32_t)n;
    Scratch sc(ctx);
    const uint8_t *s = symbols;
    if (!dev) {
        uint8_t *p = nullptr;
        SSYM_TRY(sc.get(&p, N));
        SSYM_HIP_CHECK(ctx, hipMemcpyAsync(p, symbols, N, hipMemcpyHostToDevice, ctx->stream));
        s = p;
    }
    uint32_t *res = nullptr, *votes = nullptr;
    SSYM_TRY(sc.get(&res, (size_t)N + 1));
    if (out_votes)
        SSYM_TRY(sc.get(&votes, 2 * ((size_t)N + 1)));
    SSYM_TRY(vote_dev(ctx, sc, s, N, alphabet, depth, threshold, res, votes));
    return finish_votes(ctx, res, N, votes, out_votes, out_seg_frames, n_segments);
    });
}

int32_t ssym_partition(ssym_ctx *ctx, const ssym_gmm *gmm, const double *feats, uint64_t n_frames, uint32_t depth,
                       uint32_t threshold, uint32_t flags, uint64_t *out_seg_frames, uint64_t *n_segments)
{
    return guarded(ctx, [&]() -> int32_t {
    if (!ctx)
        return SSYM_E_INVALID;
    if (!gmm) {
        ctx->err = "ssym_partition: NULL model";
        return SSYM_E_INVALID;
    }
    SSYM_TRY(vote_args(ctx, "ssym_partition", n_frames, gmm->K, depth, out_seg_frames, n_segments));
    if (n_frames && !feats) {
        ctx->err = "ssym_partition: NULL buffer";
        return SSYM_E_INVALID;
    }
    if (n_frames < depth) {
        vote_trivial(n_frames, nullptr, out_seg_frames, n_segments);
        return SSYM_OK;
    }
    SSYM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t N = (uint32_t)n_frames;
    const int d = (int)gmm->d;
    Scratch sc(ctx);
    const double *x = nullptr;
    SSYM_TRY(device_feats(ctx, sc, feats, n_frames * d, (flags & SSYM_OUT_DEVICE) != 0, &x));
    if (flags & SSYM_GMM_STANDARDIZE) {
        double *zz = nullptr;
        SSYM_TRY(sc.get(&zz, n_frames * d));
        SSYM_TRY(standardize_dev(ctx, sc, x, n_frames, d, zz));
        x = zz;
    }
    uint8_t *let = nullptr;
    uint32_t *res = nullptr;
    SSYM_TRY(sc.get(&let, N));
    SSYM_TRY(sc.get(&res, (size_t)N + 1));
    SSYM_TRY(predict_dev(ctx, sc, gmm, x, n_frames, nullptr, let));
    SSYM_TRY(vote_dev(ctx, sc, let, N, gmm->K, depth, threshold, res, nullptr));
    return finish_votes(ctx, res, N, nullptr, nullptr, out_seg_frames, n_segments);
    });
}

}  // extern "C"
