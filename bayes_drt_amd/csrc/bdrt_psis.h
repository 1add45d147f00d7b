// bdrt_psis.h -- the steps of Pareto-smoothed importance sampling shared by bdrt_loo.hip (elpd, k-hat) and bdrt_loo_predict.hip
// (the LOO predictive moments): the log-likelihood of a point, the order-preserving key, the radix select of the cutoff, the
// Zhang-Stephens fit and the smoothed tail values; and the predictive sums of bdrt_loo_predict.hip, which bdrt_heldout.hip takes
// under equal weights.  Definitions: tests/psis_numpy.py.  One copy of each, so the kernels give the same cutoff, tail, k-hat
// and sums to the bit.  Compiled with -ffp-contract=off like every includer of bdrt_stats.h.
#pragma once
#include <cfloat>
#include <cmath>
#include <vector>

#include "bdrt_host.h"
#include "bdrt_stats.h"

namespace bdrt {

constexpr int LO_NT = 512;                       // 8 waves
constexpr int LO_NW = LO_NT / 64;
constexpr int LO_MAX_S = 16384;                  // draws per column of either kernel
constexpr int LO_MAX_M = 96;                     // b_j of the Pareto fit: 30 + sqrt(ceil(16384 / 5)) = 87
constexpr int LO_TILE = 32;

// host pieces both entry points use (bdrt_loo.hip)
// tail length M = ceil(min(S / 5, 3 sqrt(S / reff))) per column, as the numpy statement computes it; -1 and the error text
// (in the name of `who`) when a reff is not a positive number
int loo_tail_lengths(const char *who, int S, size_t ncol, const double *reff, std::vector<int> &M);
// The device-pointer cores of the entry points: each enqueues on `stream` and returns; the caller synchronises.
// device [G][S][N] (rows of ld >= N doubles) -> device [G][N][S] (transpose_kernel); -2 when the grid would not fit, -10 on a
// launch error
int loo_transpose_device(const char *who, const double *dIn, double *dT, int G, int S, int N, size_t ld, hipStream_t stream);
// loglik_kernel: dZh, dSg rows of ld doubles of which the N2 from the pointer on count, dz [G][N2] -> dLl [rows][N2 or N2 / 2]
int loo_loglik_device(const double *dZh, const double *dSg, const double *dz, size_t rows, int S, int N2, size_t ld, int pair,
                      double *dLl, hipStream_t stream);
// psis_kernel on T [ncol][S] with tail lengths dM [ncol]: dOut 4 planes of ncol (lpd, elpd_loo, pareto_k, p_waic), dNtail [ncol]
int loo_psis_device(const double *dT, const int *dM, size_t ncol, int S, double *dOut, int *dNtail, hipStream_t stream);
// predict_kernel on the transposed Z_hat and sigma_tot [G][N2][S], dz [G][N2], dM [units]: dOut 6 planes of G N2 (mean, sd, pit,
// mean_post, sd_post, pit_post), then pareto_k [units]; dNtail [units]
int loo_predict_device(const double *dTm, const double *dTs, const double *dz, const int *dM, int G, int S, int N2, int pair,
                       double *dOut, int *dNtail, hipStream_t stream);

// Scratch of one chunk of groups of a LooDraws job (bdrt_host.h) and the steps its two reductions share (bdrt_loo.hip)
struct LooStage {
    DevBuf<double> par, zh, sg, lp;              // the evaluator's outputs for the chunk's rows
    DevBuf<double> z;                            // [gmax][ncols] data rows
    DevBuf<double> ll, T, lik, dg;               // ll, its transpose; reff_mode 2: the likelihood draws, diag_kernel's outputs
    DevBuf<double> out;                          // result planes of the chunk
    DevBuf<int> M, ntail;
    std::vector<int> hM;
    int gmax = 0;                                // groups per chunk
    int alloc(const LooDraws &j, bool predict, size_t out_doubles_per_group);
    int eval(const LooDraws &j, int g0, int gn);
    int loglik_T(const char *who, const LooDraws &j, int gn);
    int tails(const char *who, const LooDraws &j, int g0, int gn, double *reff);
};

// log normal(z | mu, s), c0 = -log(2 pi) / 2; NaN unless s is a positive finite number
__device__ inline double lo_normal_loglik(double z, double mu, double s, double c0)
{
    const double q = (z - mu) / s;
    double v = (c0 - log(s)) - 0.5 * (q * q);
    if (!(s > 0.0) || !isfinite(s)) v = NAN;
    return v;
}

// order-preserving key of a double (no NaN here): larger value <=> larger key
__device__ inline unsigned long long lo_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ inline double lo_unkey(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

__device__ inline double lo_gpinv(double p, double k, double sigma)
{
    if (!(sigma > 0.0)) return NAN;
    double x;
    if (fabs(k) < DBL_EPSILON) x = -log1p(-p);
    else x = expm1(-k * log1p(-p)) / k;
    return x * sigma;
}

// The rank-th largest of col[0 .. S) (LDS), 1 <= rank <= S, by radix select: 8 passes of 8 bits on the key, histogram in LDS,
// equal bins of a wave merged into one atomic.  hist [256], si [>= 2]: LDS.  Called by all LO_NT threads; a barrier stands in
// front of the first read of col, and every thread returns the same value.
__device__ inline double lo_radix_select(const double *col, int S, int rank, int *hist, int *si)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long prefix = 0;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        __syncthreads();
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int base = 0; base < S; base += LO_NT) {
            const int s = base + tid;
            bool act = s < S;
            const unsigned long long key = act ? lo_key(col[s]) : 0ull;
            if (pass > 0) act = act && ((key >> (shift + 8)) == prefix);
            const int bin = (int)((key >> shift) & 255ull);
            const unsigned long long am = __ballot(act);
            if (am) {
                const int first = __ffsll((long long)am) - 1;
                const int b0 = __shfl(bin, first, 64);
                const unsigned long long same = __ballot(act && bin == b0);
                if (act) {
                    if (bin == b0) {
                        if (lane == first) atomicAdd(&hist[b0], __popcll(same));
                    } else {
                        atomicAdd(&hist[bin], 1);
                    }
                }
            }
        }
        __syncthreads();
        if (w == 0) {
            const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const int own = (h0 + h1) + (h2 + h3);
            int suf = own;                                            // elements in the bins of lanes >= this one
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_down(suf, o, 64);
                if (lane + o < 64) suf += t;
            }
            const int above = suf - own;
            if (above < rank && rank <= suf) {                        // exactly one lane
                int acc = above, sel = 4 * lane + 3, left = rank - acc;
                if (rank > acc + h3) {
                    acc += h3; sel = 4 * lane + 2; left = rank - acc;
                    if (rank > acc + h2) {
                        acc += h2; sel = 4 * lane + 1; left = rank - acc;
                        if (rank > acc + h1) { acc += h1; sel = 4 * lane; left = rank - acc; }
                    }
                }
                si[0] = sel; si[1] = left;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | (unsigned long long)si[0];
        rank = si[1];
    }
    return lo_unkey(prefix);
}

// Generalised-Pareto fit (Zhang and Stephens) to y = exp(tail) - ecut of the n > 4 sorted tail values: one wave per b_j, lanes
// over y.  tail, y [n], bj, kj, Lj, wj [LO_MAX_M], sc [1], red [LO_NW]: LDS.  Called by all LO_NT threads behind a barrier
// that published tail; khat and sigma are the same in every thread.
__device__ inline void lo_pareto_fit(const double *tail, double *y, int n, double ecut, double *bj, double *kj, double *Lj,
                                     double *wj, double *sc, double *red, double &khat, double &sigma)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int r = tid; r < n; r += LO_NT) y[r] = exp(tail[r]) - ecut;
    __syncthreads();
    const int m = min(30 + (int)sqrt((double)n), LO_MAX_M);
    const double dn = (double)n;
    if (tid < m) {
        double b = 1.0 - sqrt((double)m / ((double)(tid + 1) - 0.5));
        b /= 3.0 * y[(int)(dn / 4.0 + 0.5) - 1];
        b += 1.0 / y[n - 1];
        bj[tid] = b;
    }
    __syncthreads();
    for (int j = w; j < m; j += LO_NW) {
        const double nb = -bj[j];
        double s = 0.0;
        for (int r = lane; r < n; r += 64) s += log1p(nb * y[r]);
        s = wave_sum(s);
        if (lane == 0) kj[j] = s / dn;
    }
    __syncthreads();
    if (tid < m) Lj[tid] = dn * ((log(-bj[tid] / kj[tid]) - kj[tid]) - 1.0);
    __syncthreads();
    if (tid < m) {
        double s = 0.0;
        const double L = Lj[tid];
        for (int i = 0; i < m; ++i) s += exp(Lj[i] - L);
        wj[tid] = 1.0 / s;
    }
    __syncthreads();
    if (tid == 0) {
        double sw = 0.0, bp = 0.0;
        for (int j = 0; j < m; ++j)
            if (wj[j] >= 10.0 * DBL_EPSILON) sw += wj[j];
        for (int j = 0; j < m; ++j)
            if (wj[j] >= 10.0 * DBL_EPSILON) bp += bj[j] * (wj[j] / sw);
        sc[0] = bp;
    }
    __syncthreads();
    const double bp = sc[0];
    double s = 0.0;
    for (int r = tid; r < n; r += LO_NT) s += log1p(-bp * y[r]);
    const double km = block_sum<LO_NW>(s, red) / dn;
    sigma = -km / bp;
    khat = (dn * km + 5.0) / (dn + 10.0);
}

// smoothed value of the r-th of n sorted tail elements: the log of the fitted quantile at (r + 1/2) / n, at most 0
__device__ inline double lo_smoothed(int r, int n, double khat, double sigma, double ecut)
{
    const double v = log(lo_gpinv(((double)r + 0.5) / (double)n, khat, sigma) + ecut);
    return v > 0.0 ? 0.0 : v;
}

// ---- the equal- and smoothed-weight predictive sums of bdrt_loo_predict.hip, shared with bdrt_heldout.hip (equal weights only)
constexpr int LP_NSUM = 7;                       // denominator + 3 terms x 2 scalars
constexpr int LP_RED = LP_NSUM * LO_NW;          // doubles of reduction scratch

struct PredictArgs {
    const double *Tm, *Ts;                       // [G][N2][S] device: Z_hat and sigma_tot, transposed
    const double *z;                             // [G][N2] device
    const int *M;                                // [units] tail length
    int S, cap, N2, U, pair;                     // cap = ceil(S / 5); U units per fit = pair ? N2 / 2 : N2
    double c0, log_dbl_min;
    double *out;                                 // 6 planes [G][N2]: mean, sd, pit, mean_post, sd_post, pit_post
    double *khat;                                // [units]
    int *ntail;
};

// K sums at once in the order of block_sum: wave butterflies, then the wave partials from wave 0 upward.  red: K * LO_NW doubles
template <int K>
__device__ inline void block_sums(double (&v)[K], double *red)
{
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[k * LO_NW + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = waves_sum<LO_NW>(red + k * LO_NW, 1);
}

// the three terms of one draw and scalar: d = mu - z (centred on the datum: no cancellation), sigma^2 + d^2, Phi((z - mu) / sigma)
__device__ inline void predict_terms(double mu, double sg, double z, double &d, double &e2, double &phi)
{
    d = mu - z;
    e2 = sg * sg + d * d;
    phi = 0.5 * erfc(d / (sg * M_SQRT2));
}

// mean, sd and pit of one scalar from the normalised sums m1 = E d, m2 = E (sigma^2 + d^2), p = E Phi
__device__ inline void predict_write(double *out, size_t plane, size_t e, double z, double m1, double m2, double p)
{
    out[e] = z + m1;
    out[plane + e] = sqrt(m2 - m1 * m1);
    out[2 * plane + e] = p;
}

}  // namespace bdrt
