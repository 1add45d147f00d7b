// bdrt_loo.hip -- PSIS-LOO and WAIC of HMC draws on the device (include/bdrt.h section (4)).
//
// Model comparison of sampling fits: leave-one-out cross-validation of the posterior by Pareto-smoothed importance sampling
// (Vehtari, Gelman, Gabry 2017) and WAIC.  Definitions: tests/psis_numpy.py (the yardstick).  Every observation is a column of S
// log-likelihoods, one per draw; the draws arrive row-major ([G][S][N]), so columns are strided by N doubles.
//
//   loglik_kernel     ll = log normal(z | Z_hat, sigma_tot) per draw and observation, optionally summed over the real and the
//                     imaginary part of one frequency
//   transpose_kernel  [G][S][N] -> [G][N][S] through a 32 x 33 LDS tile (256-B rows on both sides, conflict-free column reads)
//   psis_kernel       one workgroup (8 waves) per column:
//     1  the column goes to LDS; max, min, log-sum-exp, mean, centred sum of squares        -> lpd, p_waic
//     2  x = min(ll) - ll (the log ratios -ll shifted by their maximum) replaces the column
//     3  the (M+1)-th largest x by radix select (8 passes of 8 bits on the order-preserving 64-bit key; histogram in LDS,
//        equal bins of a wave merged into one atomic); cutoff = max(that, log DBL_MIN)
//     4  one sweep: values above the cutoff are compacted into the tail buffer (<= ceil(S/5)), the others add their terms to
//        the two body sums -- after this the column itself is no longer needed
//     5  bitonic sort of the tail only (same-direction network, any length, no padding stored)
//     6  y = exp(tail) - exp(cutoff) goes where the column was; Zhang-Stephens fit: one wave per b_j, lanes over y
//     7  smoothed tail values (stored behind y), the two tail sums; a tail element's ll is min(ll) minus its sorted x
//        -> elpd_loo, pareto_k, n_tail
//   lik_kernel        exp(ll - max ll) per column of the transposed matrix, for the relative efficiency of reff_mode 2
// Each entry point is a device-pointer core (loo_*_device: enqueue on a stream) and a staging wrapper; bdrt_sampler_loo runs
// the cores on a sampler's draws in chunks of groups (LooStage, loo_of_draws).
// Every sum is a per-thread strided partial, a wave butterfly and the eight wave partials added in order; the compaction order
// (the one thing atomics decide) is erased by the sort.  So a column gives the same bits alone or in any batch.  The reductions
// and the sorting network are bdrt_stats.h's; the log-likelihood of a point, the key, the radix select, the Pareto fit and the
// smoothed tail value are bdrt_psis.h's, shared with bdrt_loo_predict.hip.  Every product and sum is rounded separately, as in
// the numpy statement.
#include <cfloat>
#include <cmath>

#include "bdrt_host.h"
#include "bdrt_psis.h"

namespace bdrt {

// LO_MAX_S draws per column: 128 KiB column + 26 KiB tail + scratch <= 160 KiB of LDS
// Zhat, sig: rows of ld doubles, of which the N2 columns from the pointer on count; z [G][N2]
__global__ __launch_bounds__(256) void loglik_kernel(const double *__restrict__ Zhat, const double *__restrict__ sig,
                                                     const double *__restrict__ z, size_t rows, int S, int N2, size_t ld, int pair,
                                                     double c0, double *__restrict__ out)
{
    // rows = G * S draw rows; one thread per output element
    const int No = pair ? N2 / 2 : N2;
    const size_t total = rows * (size_t)No;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e / No;
        const int j = (int)(e - r * No);
        const size_t g = r / S;
        double acc = 0.0;
        for (int h = 0; h <= pair; ++h) {
            const int c = j + h * No;
            const double v = lo_normal_loglik(z[g * N2 + c], Zhat[r * ld + c], sig[r * ld + c], c0);
            acc = h ? acc + v : v;
        }
        out[e] = acc;
    }
}

// in [G][S][N] (rows of ld >= N doubles) -> out [G][N][S]
__global__ __launch_bounds__(256) void transpose_kernel(const double *__restrict__ in, double *__restrict__ out, int S, int N,
                                                        size_t ld, int tilesS, int tilesN)
{
    __shared__ double tile[LO_TILE][LO_TILE + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;                  // 32 x 8
    size_t b = blockIdx.x;
    const int tn = (int)(b % tilesN); b /= tilesN;
    const int ts = (int)(b % tilesS);
    const size_t g = b / tilesS;
    const double *src = in + g * (size_t)S * ld;
    double *dst = out + g * (size_t)S * N;
    const int s0 = ts * LO_TILE, n0 = tn * LO_TILE;
#pragma unroll
    for (int k = 0; k < LO_TILE; k += 8) {
        const int s = s0 + ty + k, n = n0 + tx;
        if (s < S && n < N) tile[ty + k][tx] = src[(size_t)s * ld + n];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LO_TILE; k += 8) {
        const int n = n0 + ty + k, s = s0 + tx;
        if (s < S && n < N) dst[(size_t)n * S + s] = tile[tx][ty + k];
    }
}

struct LooArgs {
    const double *T;                             // [columns][S] device
    const int *M;                                // [columns] tail length
    int S, cap;                                  // cap = ceil(S / 5): capacity of the tail buffer
    double log_dbl_min, log_S;
    double *lpd, *elpd, *khat, *pwaic;           // [columns] device
    int *ntail;
};

__global__ __launch_bounds__(LO_NT) void psis_kernel(LooArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int S = a.S;
    const size_t c = blockIdx.x;
    double *col = lds;                                                // [S]      ll, then x, then y | smoothed tail
    double *tail = col + S;                                           // [cap]    tail of x, sorted ascending
    double *red = tail + a.cap;                                       // [LO_NW]
    double *bj = red + LO_NW;                                         // [LO_MAX_M] each
    double *kj = bj + LO_MAX_M;
    double *Lj = kj + LO_MAX_M;
    double *wj = Lj + LO_MAX_M;
    double *sc = wj + LO_MAX_M;                                       // [4]
    int *hist = (int *)(sc + 4);                                      // [256]
    int *si = hist + 256;                                             // [4]
    const double *src = a.T + c * (size_t)S;

    // ---- 1: column to LDS; extremes, log-sum-exp, mean and centred sum of squares
    int bad = 0;
    double mx = -INFINITY, mn = INFINITY, sum = 0.0;
    for (int s = tid; s < S; s += LO_NT) {
        const double v = src[s];
        bad |= !isfinite(v);
        col[s] = v;
        mx = fmax(mx, v);
        mn = fmin(mn, v);
        sum += v;
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) { a.lpd[c] = NAN; a.elpd[c] = NAN; a.khat[c] = NAN; a.pwaic[c] = NAN; a.ntail[c] = 0; }
        return;
    }
    mx = block_max<LO_NW>(mx, red);
    mn = -block_max<LO_NW>(-mn, red);
    if (mx == mn) {                                                   // all draws equal: nothing to reweight
        if (tid == 0) { a.lpd[c] = mx; a.elpd[c] = mx; a.khat[c] = INFINITY; a.pwaic[c] = 0.0; a.ntail[c] = 0; }
        return;
    }
    const double mean = block_sum<LO_NW>(sum, red) / (double)S;
    double se = 0.0, sq = 0.0;
    for (int s = tid; s < S; s += LO_NT) {
        const double v = col[s], d = v - mean;
        se += exp(v - mx);
        sq = fma(d, d, sq);
    }
    se = block_sum<LO_NW>(se, red);
    sq = block_sum<LO_NW>(sq, red);
    if (tid == 0) {
        a.lpd[c] = (mx + log(se)) - a.log_S;
        a.pwaic[c] = sq / (double)(S - 1);
    }
    // ---- 2: shifted log ratios
    __syncthreads();
    for (int s = tid; s < S; s += LO_NT) col[s] = mn - col[s];
    // ---- 3: radix select of the (M+1)-th largest
    const double cutoff = fmax(lo_radix_select(col, S, a.M[c] + 1, hist, si), a.log_dbl_min);
    const double ecut = exp(cutoff);
    // ---- 4: compact the tail, sum the body
    __syncthreads();
    if (tid == 0) si[2] = 0;
    __syncthreads();
    double bden = 0.0, bnum = 0.0;
    for (int base = 0; base < S; base += LO_NT) {
        const int s = base + tid;
        const bool in = s < S;
        const double x = in ? col[s] : 0.0;
        const bool up = in && x > cutoff;
        if (in && !up) {
            bden += exp(x - cutoff);
            bnum += exp((x + src[s]) - mn);
        }
        const unsigned long long um = __ballot(up);
        if (um) {
            const int first = __ffsll((long long)um) - 1;
            int pos = 0;
            if (lane == first) pos = atomicAdd(&si[2], __popcll(um));
            pos = __shfl(pos, first, 64) + __popcll(um & ((1ull << lane) - 1ull));
            if (up && pos < a.cap) tail[pos] = x;
        }
    }
    bden = block_sum<LO_NW>(bden, red);
    bnum = block_sum<LO_NW>(bnum, red);                                   // (its barriers also publish tail[] and si[2])
    const int n = min(si[2], a.cap);
    // ---- 5: sort the tail ascending; partners past the end are +inf and never move
    bitonic_any<LO_NT>(n, [&](int i, int q) {
        const double u = tail[i], v = tail[q];
        if (u > v) { tail[i] = v; tail[q] = u; }
    });
    // ---- 6: generalised-Pareto fit to y = exp(tail) - exp(cutoff)
    double khat = INFINITY, sigma = NAN;
    double *y = col, *sm = col + a.cap;                               // 2 cap <= S for S >= 4; else n <= 4 and neither is used
    if (n > 4) lo_pareto_fit(tail, y, n, ecut, bj, kj, Lj, wj, sc, red, khat, sigma);
    // ---- 7: smoothed tail, the tail sums, results
    const bool smooth = n > 4 && isfinite(khat);
    double mt = -INFINITY, ut = -INFINITY;
    for (int r = tid; r < n; r += LO_NT) {
        const double t = tail[r];
        double v = t;
        if (smooth) {
            v = lo_smoothed(r, n, khat, sigma, ecut);
            sm[r] = v;
        }
        mt = fmax(mt, v);
        ut = fmax(ut, v + (mn - t));
    }
    mt = block_max<LO_NW>(mt, red);
    ut = block_max<LO_NW>(ut, red);
    double tden = 0.0, tnum = 0.0;
    for (int r = tid; r < n; r += LO_NT) {
        const double t = tail[r];
        const double v = smooth ? sm[r] : t;
        tden += exp(v - mt);
        tnum += exp((v + (mn - t)) - ut);
    }
    tden = block_sum<LO_NW>(tden, red);
    tnum = block_sum<LO_NW>(tnum, red);
    if (tid == 0) {
        double lden, lnum;
        if (n == 0) {
            lden = cutoff + log(bden);
            lnum = mn + log(bnum);
        } else {
            const double md = fmax(cutoff, mt), mu = fmax(mn, ut);
            lden = md + log(bden * exp(cutoff - md) + tden * exp(mt - md));
            lnum = mu + log(bnum * exp(mn - mu) + tnum * exp(ut - mu));
        }
        a.elpd[c] = lnum - lden;
        a.khat[c] = khat;
        a.ntail[c] = n;
    }
}

// The likelihood draws of `relative_efficiency` (reff_mode 2 of bdrt_sampler_loo): lik = exp(ll - max ll) per column of
// T [columns][S], written in the same layout, so that every column is one group of `chains` chains and one column for
// diag_kernel (unit stride n_draws, row stride 1) and its staging reads run along S.  One wave per column, four columns per
// workgroup: lanes stride the column (coalesced), the maximum is a wave butterfly (bdrt_stats.h; a maximum has one value
// whatever the order), no LDS, no barrier, no atomic.  The second sweep finds the column in L2 (at most 128 KiB).  A NaN
// anywhere makes the maximum NaN, as numpy's max does, and with it the whole column; so does a column of -inf.
constexpr int LK_NT = 256;
__global__ __launch_bounds__(LK_NT) void lik_kernel(const double *__restrict__ T, size_t ncol, int S, double *__restrict__ lik)
{
    const int lane = threadIdx.x & 63;
    const size_t c = (size_t)blockIdx.x * (LK_NT / 64) + (threadIdx.x >> 6);
    if (c >= ncol) return;                                            // (whole waves leave)
    const double *src = T + c * (size_t)S;
    double *dst = lik + c * (size_t)S;
    double mx = -INFINITY;
    int nan = 0;
    for (int s = lane; s < S; s += 64) {
        const double v = src[s];
        nan |= (v != v);
        mx = fmax(mx, v);
    }
    mx = wave_max(mx);
    if (__ballot(nan)) mx = NAN;
    for (int s = lane; s < S; s += 64) dst[s] = exp(src[s] - mx);
}

static size_t loo_lds_bytes(int S, int cap)
{
    return ((size_t)S + cap + LO_NW + 4 * LO_MAX_M + 4) * sizeof(double) + (256 + 4) * sizeof(int);
}

// tail length M = ceil(min(S / 5, 3 sqrt(S / reff))), as the numpy statement computes it (host arithmetic)
int loo_tail_lengths(const char *who, int S, size_t ncol, const double *reff, std::vector<int> &M)
{
    M.resize(ncol);
    const int cap = (S + 4) / 5;
    for (size_t i = 0; i < ncol; ++i) {
        const double r = reff ? reff[i] : 1.0;
        if (!(r > 0.0) || !std::isfinite(r)) { set_error("%s: reff[%zu] = %g is not a positive number", who, i, r); return -1; }
        const double v = std::ceil(std::min((double)S / 5.0, 3.0 * std::sqrt((double)S / r)));
        M[i] = std::max(1, std::min(cap, (int)v));
    }
    return 0;
}

// ---- device-pointer cores: each enqueues on `stream` and returns; the caller synchronises
int loo_transpose_device(const char *who, const double *dIn, double *dT, int G, int S, int N, size_t ld, hipStream_t stream)
{
    const int tilesS = (S + LO_TILE - 1) / LO_TILE, tilesN = (N + LO_TILE - 1) / LO_TILE;
    const size_t tiles = (size_t)G * tilesS * tilesN;
    if (tiles > 0x7fffffffull) { set_error("%s: too many tiles", who); return -2; }
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, dIn, dT, S, N, ld, tilesS, tilesN);
    BDRT_HIP(hipGetLastError());
    return 0;
}

int loo_loglik_device(const double *dZh, const double *dSg, const double *dz, size_t rows, int S, int N2, size_t ld, int pair,
                      double *dLl, hipStream_t stream)
{
    const size_t nout = rows * (pair ? N2 / 2 : N2);
    const unsigned blocks = (unsigned)std::min<size_t>((nout + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(loglik_kernel, dim3(blocks), dim3(256), 0, stream, dZh, dSg, dz, rows, S, N2, ld, pair,
                       -0.5 * std::log(2.0 * M_PI), dLl);
    BDRT_HIP(hipGetLastError());
    return 0;
}

// psis_kernel on T [ncol][S] with the tail lengths dM [ncol]: dOut 4 planes of ncol (lpd, elpd_loo, pareto_k, p_waic), dNtail [ncol]
int loo_psis_device(const double *dT, const int *dM, size_t ncol, int S, double *dOut, int *dNtail, hipStream_t stream)
{
    const int cap = (S + 4) / 5;
    const size_t lds = loo_lds_bytes(S, cap);
    static LdsAttrCache cache;
    BDRT_HIP(cache.ensure(lds, [&]() {
        return hipFuncSetAttribute((const void *)psis_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }));
    LooArgs a;
    a.T = dT; a.M = dM; a.S = S; a.cap = cap;
    a.log_dbl_min = std::log(DBL_MIN); a.log_S = std::log((double)S);
    a.lpd = dOut; a.elpd = dOut + ncol; a.khat = dOut + 2 * ncol; a.pwaic = dOut + 3 * ncol;
    a.ntail = dNtail;
    hipLaunchKernelGGL(psis_kernel, dim3((unsigned)ncol), dim3(LO_NT), lds, stream, a);
    BDRT_HIP(hipGetLastError());
    return 0;
}

// ---- PSIS-LOO of draws that are on the device (bdrt_sampler_loo, bdrt_sampler_loo_predict): chunks of groups
// scratch of one group: the evaluator's outputs (parameters, Z_hat, sigma_tot, lp), its data row, and what the reduction
// stages per draw -- ll and its transpose (LOO), the two transposes (predict), for reff_mode 2 also ll, its transpose (predict)
// and the likelihood matrix.  The per-column results (a few doubles per observation) are not counted.
size_t loo_draws_group_bytes(const LooDraws &j, bool predict)
{
    const size_t S = (size_t)j.chains * j.n_draws, N2 = 2 * (size_t)j.prob->dev.nf, U = j.pair ? j.ncols / 2 : j.ncols;
    const bool aut = j.reff_mode == 2;
    size_t d = S * ((size_t)j.prob->dev.D + 2 * N2 + 1) + (size_t)j.ncols;
    d += predict ? 2 * S * (size_t)j.ncols + (aut ? 3 * S * U : 0) : S * U * (aut ? 3 : 2);
    return d * sizeof(double);
}

// groups per chunk: as many as stay within chunk_bytes (0: LOO_CHUNK_DEFAULT), at least one, and rows that an int counts
static int loo_draws_chunk_groups(const LooDraws &j, bool predict)
{
    const size_t budget = j.chunk_bytes ? j.chunk_bytes : LOO_CHUNK_DEFAULT, S = (size_t)j.chains * j.n_draws;
    const size_t n = std::min(budget / loo_draws_group_bytes(j, predict), ((size_t)1 << 30) / S);
    return (int)std::max<size_t>(1, std::min<size_t>(n, (size_t)j.G));
}

int LooStage::alloc(const LooDraws &j, bool predict, size_t out_doubles_per_group)
{
    gmax = loo_draws_chunk_groups(j, predict);
    const size_t S = (size_t)j.chains * j.n_draws, N2 = 2 * (size_t)j.prob->dev.nf, U = j.pair ? j.ncols / 2 : j.ncols;
    const size_t rows = (size_t)gmax * S;
    const bool aut = j.reff_mode == 2;
    BDRT_HIP(par.alloc(rows * j.prob->dev.D));
    BDRT_HIP(zh.alloc(rows * N2));
    BDRT_HIP(sg.alloc(rows * N2));
    BDRT_HIP(lp.alloc(rows));
    BDRT_HIP(z.alloc((size_t)gmax * j.ncols));
    if (!predict || aut) {
        BDRT_HIP(ll.alloc(rows * U));
        BDRT_HIP(T.alloc(rows * U));
    }
    if (aut) {
        BDRT_HIP(lik.alloc(rows * U));
        BDRT_HIP(dg.alloc(4 * (size_t)gmax * U));
    }
    BDRT_HIP(out.alloc((size_t)gmax * out_doubles_per_group));
    BDRT_HIP(M.alloc((size_t)gmax * U));
    BDRT_HIP(ntail.alloc((size_t)gmax * U));
    return 0;
}

// Z_hat and sigma_tot of the draws of groups [g0, g0 + gn) by the batch evaluator (the launch of bdrt_transformed, on the
// draws where they are), and the groups' data rows, columns [col0, col0 + ncols), side by side in z
int LooStage::eval(const LooDraws &j, int g0, int gn)
{
    Problem &P = *j.prob;
    const size_t S = (size_t)j.chains * j.n_draws, N2 = 2 * (size_t)P.dev.nf;
    if (const int rc = launch_logp_grad(&P, j.draws + (size_t)g0 * S * P.dev.D, nullptr, (int)((size_t)gn * S), 0, lp, nullptr, par, zh, sg,
                                        j.stream))
        return rc;
    for (int g = 0; g < gn; ++g)
        BDRT_HIP(hipMemcpyAsync(z.p + (size_t)g * j.ncols, P.d_Z.p + (size_t)j.spec[g0 + g] * N2 + j.col0, (size_t)j.ncols * sizeof(double),
                                hipMemcpyDeviceToDevice, j.stream));
    return 0;
}

// ll [gn][S][U] of the chunk and its transpose T [gn][U][S]
int LooStage::loglik_T(const char *who, const LooDraws &j, int gn)
{
    const int S = j.chains * j.n_draws, U = j.pair ? j.ncols / 2 : j.ncols;
    const size_t N2 = 2 * (size_t)j.prob->dev.nf;
    if (const int rc = loo_loglik_device(zh.p + j.col0, sg.p + j.col0, z, (size_t)gn * S, S, j.ncols, N2, j.pair, ll, j.stream)) return rc;
    return loo_transpose_device(who, ll, T, gn, S, U, (size_t)U, j.stream);
}

// The relative efficiencies of the chunk's columns go to reff [gn * U] (host) -- reff_mode 0: 1; 1: the caller's; 2: n_eff / S
// of the likelihood draws (lik_kernel on T, then diag_kernel), 1 where that is not a positive number, which is
// loo.relative_efficiency as written -- and the tail lengths that follow from them to M (device).  Mode 2 needs loglik_T first.
int LooStage::tails(const char *who, const LooDraws &j, int g0, int gn, double *reff)
{
    const int S = j.chains * j.n_draws, U = j.pair ? j.ncols / 2 : j.ncols;
    const size_t ncol = (size_t)gn * U;
    if (ncol > 0x7fffffffull) { set_error("%s: too many columns", who); return -2; }
    if (j.reff_mode == 0) std::fill(reff, reff + ncol, 1.0);
    else if (j.reff_mode == 1) std::copy(j.reff_in + (size_t)g0 * U, j.reff_in + (size_t)g0 * U + ncol, reff);
    else {
        hipLaunchKernelGGL(lik_kernel, dim3((unsigned)((ncol + LK_NT / 64 - 1) / (LK_NT / 64))), dim3(LK_NT), 0, j.stream,
                           (const double *)T, ncol, S, (double *)lik);
        BDRT_HIP(hipGetLastError());
        if (const int rc = diagnostics_device(lik, (long)j.n_draws, 1L, nullptr, (int)ncol, j.chains, j.n_draws, 1, dg, dg.p + ncol,
                                              dg.p + 2 * ncol, dg.p + 3 * ncol, j.stream))
            return rc;
        BDRT_HIP(hipMemcpy(reff, dg.p + 2 * ncol, ncol * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ncol; ++i) {
            const double r = reff[i] / (double)S;
            reff[i] = (std::isfinite(r) && r > 0.0) ? r : 1.0;
        }
    }
    if (loo_tail_lengths(who, S, ncol, reff, hM)) return -1;
    return upload(M.p, hM.data(), ncol, j.stream);       // (hM lives until the caller's synchronisation)
}

int loo_of_draws(const LooDraws &j, double *lpd, double *elpd_loo, double *pareto_k, double *p_waic, int *n_tail, double *reff_out)
{
    const char *who = "bdrt_sampler_loo";
    const int S = j.chains * j.n_draws, U = j.pair ? j.ncols / 2 : j.ncols;
    std::vector<double> reff((size_t)j.G * U);
    LooStage st;
    if (const int rc = st.alloc(j, false, 4 * (size_t)U)) return rc;
    for (int g0 = 0; g0 < j.G; g0 += st.gmax) {
        const int gn = std::min(st.gmax, j.G - g0);
        const size_t ncol = (size_t)gn * U, o = (size_t)g0 * U;
        int rc;
        if ((rc = st.eval(j, g0, gn)) || (rc = st.loglik_T(who, j, gn)) || (rc = st.tails(who, j, g0, gn, reff.data() + o)) ||
            (rc = loo_psis_device(st.T, st.M, ncol, S, st.out, st.ntail, j.stream)))
            return rc;
        BDRT_HIP(hipStreamSynchronize(j.stream));
        double *const outs[4] = {lpd + o, elpd_loo + o, pareto_k + o, p_waic + o};
        if (download_planes(st.out, ncol, outs, 4)) return -10;
        BDRT_HIP(hipMemcpy(n_tail + o, st.ntail, ncol * sizeof(int), hipMemcpyDeviceToHost));
    }
    if (reff_out) std::copy(reff.begin(), reff.end(), reff_out);
    return 0;
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_pointwise_loglik(const double *Zhat, const double *sig, const double *z, int G, int S, int N2, int pair,
                          double *ll_out)
{
    if (!Zhat || !sig || !z || !ll_out || G < 1 || S < 1 || N2 < 1 || (pair != 0 && pair != 1) || (pair && (N2 & 1))) {
        set_error("bdrt_pointwise_loglik: bad arguments");
        return -1;
    }
    bind_process_device();
    const size_t rows = (size_t)G * S, nin = rows * N2, nout = rows * (pair ? N2 / 2 : N2);
    DevBuf<double> dZh, dSg, dz, dOut;
    if (upload(dZh, Zhat, nin) || upload(dSg, sig, nin) || upload(dz, z, (size_t)G * N2)) return -10;
    BDRT_HIP(dOut.alloc(nout));
    if (const int rc = loo_loglik_device(dZh, dSg, dz, rows, S, N2, (size_t)N2, pair, dOut, nullptr)) return rc;
    BDRT_HIP(hipDeviceSynchronize());
    BDRT_HIP(hipMemcpy(ll_out, dOut, nout * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int bdrt_psis_loo_max_draws(void) { return LO_MAX_S; }

int bdrt_psis_loo(const double *ll, int G, int S, int N, const double *reff, double *lpd, double *elpd_loo, double *pareto_k,
                  double *p_waic, int *n_tail)
{
    if (!ll || !lpd || !elpd_loo || !pareto_k || !p_waic || !n_tail || G < 1 || S < 2 || N < 1) {
        set_error("bdrt_psis_loo: bad arguments");
        return -1;
    }
    if (S > LO_MAX_S) { set_error("bdrt_psis_loo: %d draws per column, the kernel holds at most %d", S, LO_MAX_S); return -2; }
    const size_t ncol = (size_t)G * N;
    if (ncol > 0x7fffffffull) { set_error("bdrt_psis_loo: too many columns"); return -2; }
    std::vector<int> M;
    if (loo_tail_lengths("bdrt_psis_loo", S, ncol, reff, M)) return -1;
    bind_process_device();
    const size_t nel = ncol * S;
    DevBuf<double> dIn, dT, dOut;
    DevBuf<int> dM, dNtail;
    if (upload(dIn, ll, nel) || upload(dM, M.data(), ncol)) return -10;
    BDRT_HIP(dT.alloc(nel));
    BDRT_HIP(dOut.alloc(4 * ncol));
    BDRT_HIP(dNtail.alloc(ncol));
    if (const int rc = loo_transpose_device("bdrt_psis_loo", dIn, dT, G, S, N, (size_t)N, nullptr)) return rc;
    if (const int rc = loo_psis_device(dT, dM, ncol, S, dOut, dNtail, nullptr)) return rc;
    BDRT_HIP(hipDeviceSynchronize());
    double *const outs[4] = {lpd, elpd_loo, pareto_k, p_waic};
    if (download_planes(dOut, ncol, outs, 4)) return -10;
    BDRT_HIP(hipMemcpy(n_tail, dNtail, ncol * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

