// bdrt_stats.h -- device pieces shared by the post-sampling statistics: bdrt_post.hip, bdrt_diag.hip, bdrt_rank.hip, bdrt_loo.hip,
// bdrt_loo_predict.hip, bdrt_heldout.hip (the last three through bdrt_psis.h).
//
// Every includer is compiled with -ffp-contract=off (Makefile): the products that accumulate are explicit fma() calls, everything
// else is rounded separately, as in the numpy statements these kernels are held to (tests/diag_numpy.py, rank_numpy.py,
// psis_numpy.py, np.percentile).  No atomics and no data-dependent order in here: every sum has one fixed order, so a column
// gives the same bits alone or in any batch, staged in LDS or streamed from HBM.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace bdrt {

constexpr int STATS_LAGS = 64;                   // lags per autocovariance block of geyer_tau (one per lane)

// ---- reductions in a fixed order: wave butterflies, then the NW wave results added from wave 0 upward by every reader
__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// p[0] + p[stride] + ... + p[(NW - 1) stride], from 0 upward: for NW = 4 this is ((p0 + p1) + p2) + p3
template <int NW>
__device__ inline double waves_sum(const double *p, int stride)
{
    double t = p[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) t += p[i * stride];
    return t;
}

// red: NW doubles of LDS.  The first barrier lets the readers of the reduction before leave red; the same value in every thread
template <int NW>
__device__ inline double block_sum(double v, double *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return waves_sum<NW>(red, 1);
}

template <int NW>
__device__ inline double block_max(double v, double *red)
{
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) t = fmax(t, red[i]);
    return t;
}

// ---- same-direction bitonic network over n positions, any n, NT threads: a partner past the end counts as +inf and never
// moves, so nothing is padded.  cmp_swap(i, q), i < q < n, puts the smaller element at i.  A barrier stands in front of every
// stage and behind the last one.
template <int NT, class F>
__device__ inline void bitonic_any(int n, F cmp_swap)
{
    const int tid = threadIdx.x;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int p = tid; p < (n2 >> 1); p += NT) {
                const int blk = p / j, off = p - blk * j;
                int i, q;
                if (j == (k >> 1)) {
                    i = blk * k + off;
                    q = blk * k + (k - 1 - off);
                } else {
                    i = blk * 2 * j + off;
                    q = i + j;
                }
                if (q < n) cmp_swap(i, q);
            }
        }
    }
    __syncthreads();
}

// ---- numpy.lib.function_base._lerp (numpy >= 1.22): a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5.  Every product and
// sum is rounded separately, as in numpy's element-wise ufuncs; a fused multiply-add would differ in the last bit.
__device__ inline double numpy_lerp(double a, double b, double t)
{
    const double d = b - a;
    const double dt = d * t;
    double r = a + dt;
    if (t >= 0.5) {
        const double omt = 1.0 - t;
        const double dm = d * omt;
        r = b - dm;
    }
    return r;
}

// np.percentile(Y, 100 quant) by numpy's default ('linear') rule from the sorted values get(0) <= ... <= get(n - 1), 0 <= quant
// <= 1: virtual index (n - 1) quant, previous = floor, gamma = virtual - previous, both indices clipped to the array.  (At quant
// = 1 the virtual index is n - 1 exactly, both indices clip to it and gamma is 0.)
template <class Get>
__device__ inline double numpy_quantile(Get get, int n, double quant)
{
    const double virt = (double)(n - 1) * quant;
    const double prev = floor(virt);
    int lo = (int)prev, hi = lo + 1;
    lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
    hi = hi < 0 ? 0 : (hi > n - 1 ? n - 1 : hi);
    return numpy_lerp(get(lo), get(hi), virt - prev);
}

// ---- R-hat over H rows of n draws as chains, no further split: means[H] the row means, css[H] the rows' centred sums of
// squares.  NaN when n < 2.  Serial: every calling thread computes the same value.
__device__ inline double rhat_rows(int H, int n, const double *means, const double *css)
{
    if (n < 2) return NAN;
    double hbar = 0.0, W = 0.0, B = 0.0;
    for (int h = 0; h < H; ++h) hbar += means[h];
    hbar /= (double)H;
    for (int h = 0; h < H; ++h) { const double d = means[h] - hbar; B = fma(d, d, B); }
    B = (double)n * (B / (double)(H - 1));
    for (int h = 0; h < H; ++h) W += css[h] / (double)(n - 1);
    W /= (double)H;
    return sqrt((B / W + (double)(n - 1)) / (double)n);
}

// ---- Geyer's integrated autocorrelation time (initial positive + initial monotone sequence, Stan 2.19; tests/diag_numpy.py
// `ess`) of H chains of n draws: the effective sample size is H n / tau.  Called by all NW * 64 threads of the workgroup.
//   series(h, t)  draw t of chain h, centred by the chain's mean
//   cm, cs        [H] chain means and centred sums of squares
//   part          [NW][STATS_LAGS] LDS, wave partials;  rho [STATS_LAGS] LDS;  sc [2] LDS
// Autocovariances in blocks of 64 lags (one lag per lane, the NW waves split the draw range, their partials added from wave 0
// upward), averaged over the chains; thread 0 walks the pairs of the block, and the loop stops at the block where the positive
// sequence ends.  Returns tau, the same value in every thread; NaN when n < 4 (no pair to walk).
template <int NW, class Series>
__device__ inline double geyer_tau(Series series, int H, int n, const double *cm, const double *cs, double *part, double *rho,
                                   double *sc)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (n < 4) return NAN;
    double mean_var = 0.0;
    for (int h = 0; h < H; ++h) mean_var += (cs[h] / (double)n) * (double)n / (double)(n - 1);
    mean_var /= (double)H;
    double var_plus = mean_var * (double)(n - 1) / (double)n;
    if (H > 1) {
        double mb = 0.0, vb = 0.0;
        for (int h = 0; h < H; ++h) mb += cm[h];
        mb /= (double)H;
        for (int h = 0; h < H; ++h) { const double d = cm[h] - mb; vb = fma(d, d, vb); }
        var_plus += vb / (double)(H - 1);
    }
    const int chunk = (n + NW - 1) / NW, tw0 = min(n, w * chunk), tw1 = min(n, tw0 + chunk);
    double acc_pm = 0.0, prev_pm = 0.0;                               // thread 0: sum of monotone pair sums so far, last one
    for (int k0 = 0;; k0 += STATS_LAGS) {
        const int k = k0 + lane;
        double s = 0.0;
        if (k < n) {
            const int te = min(tw1, n - k);
            for (int h = 0; h < H; ++h)
                for (int t = tw0; t < te; ++t) s = fma(series(h, t), series(h, t + k), s);
        }
        part[w * STATS_LAGS + lane] = s;
        __syncthreads();
        if (tid < STATS_LAGS) {
            const double acov_mean = (waves_sum<NW>(part + tid, STATS_LAGS) / (double)n) / (double)H;
            rho[tid] = 1.0 - (mean_var - acov_mean) / var_plus;
        }
        __syncthreads();
        if (tid == 0) {
            double tau = NAN;
            for (int l = 0; l < STATS_LAGS && !(tau == tau); l += 2) {
                const int jp = (k0 + l) >> 1;                         // pair jp = lags (2 jp, 2 jp + 1)
                const double ev = jp == 0 ? 1.0 : rho[l], od = rho[l + 1];
                const bool cont = (2 * jp + 1 < n - 4) && (ev + od > 0.0);
                if (cont) {
                    const double p = ev + od;
                    const double pm = (jp == 0 || !(p > prev_pm)) ? p : prev_pm;
                    acc_pm += pm;
                    prev_pm = pm;
                } else {
                    const double e = (jp == 0 || ev + od >= 0.0) ? ev : 0.0;
                    const double b = ev > 0.0 ? ev : 0.0;
                    tau = -1.0 + 2.0 * (acc_pm + e) + b;
                }
            }
            const bool done = (tau == tau) || k0 + STATS_LAGS >= n;   // (the pair walk ends before lag n - 2)
            sc[0] = done ? 1.0 : 0.0;
            sc[1] = tau;
        }
        __syncthreads();
        const bool done = sc[0] != 0.0;
        const double tau = sc[1];
        __syncthreads();
        if (done) return tau;
    }
}

}  // namespace bdrt
