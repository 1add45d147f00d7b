// bdrt_rank.hip -- rank-normalised convergence diagnostics on the device (include/bdrt.h section (4)).
//
// Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021): rank-normalised, folded split R-hat, bulk and tail effective sample
// size, and the ESS / MCSE of the mean, all on the SPLIT chains.  Definitions: tests/rank_numpy.py (the yardstick).  The
// addressing is bdrt_diag.hip's: element (g, m, t, c) of the draws is X[(g*M + m) * unit_stride + t * row_stride + c], and
// expcol flags the columns whose samples are exp(X).
//
// Schedule: one workgroup (8 waves) per (group, column).  With n = N / 2 and H = 2 M split chains ("rows") of n draws, S = H n:
//   1  the S split draws go to LDS (val, row-major [H][n]: row 2m = first n draws of chain m, row 2m + 1 = its last n)
//   2  an index array (16 bit) is sorted by (value, index): any-length bitonic network, partners past the end never move
//   3  q_lo, q_hi (numpy's linear rule) and the median from the sorted order; every sorted position finds the ends of its tie
//      run by two binary searches -> average rank -> z = Phi^-1((r - 3/8) / (S + 1/4)), written to the work series (wrk) in
//      time order
//   4  row means and centred sums of squares of z (one wave per row) -> plain R-hat over the H rows; Geyer's ESS of z
//      (autocovariances in blocks of 64 lags, one lag per lane, the eight waves split the draw range; thread 0 walks the
//      pairs): ess_bulk
//   5  wrk = |val - median|, sorted and ranked again -> z of the folded draws -> R-hat; rhat = the larger of the two
//   6  wrk = 1[val <= q_lo], 1[val <= q_hi], val in turn -> ESS of each: ess_tail = the smaller of the first two, ess_mean;
//      the last pass also gives sd
// LDS per draw: 8 B val + 8 B wrk + 2 B index = 18 B, so RK_MAX_DRAWS = 8192 split draws take 144 KiB, plus 7.6 KiB of scratch.
// No atomics; every sum has a fixed order, so a column gives the same bits alone or in any batch (bdrt_stats.h: the reductions,
// the sorting network, numpy's quantile, R-hat over rows and Geyer's sequence, shared with the other post-sampling statistics).
#include <cmath>

#include "bdrt_host.h"
#include "bdrt_stats.h"

namespace bdrt {

constexpr int RK_NT = 512;                       // 8 waves
constexpr int RK_NW = RK_NT / 64;
constexpr int RK_LAGS = STATS_LAGS;               // lags per block of the autocovariance loop (one per lane)
constexpr int RK_MAX_DRAWS = 8192;               // split draws per column (S)
constexpr int RK_PER = RK_MAX_DRAWS / RK_NT;     // sorted positions per thread
constexpr int RK_MAX_CHAINS = 64;
constexpr int RK_MAX_ROWS = 2 * RK_MAX_CHAINS;
constexpr int RK_SCRATCH = RK_NW * RK_LAGS + 3 * RK_MAX_ROWS + RK_LAGS + 16;   // doubles

struct RankArgs {
    const double *X;
    long unit_stride, row_stride;
    const unsigned char *expcol;                 // [C] device, or null
    int M, N, C;
    double q_lo, q_hi;                           // tail probabilities as numpy's percentile sees them: (100 p) / 100
    double *rhat, *bulk, *tail, *essm, *sd;      // [G x C] device (all null: debug launch)
    double *zout;                                // debug launch: [S] a series of column 0 of group 0, chosen by zwhat:
    int zwhat;                                   // 0 z of the draws, 1 z of the folded draws, 2 the staged draws themselves
};

// idx <- the permutation that sorts key ascending, ties by index
__device__ inline void rk_sort(const double *key, unsigned short *idx, int S)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < S; i += RK_NT) idx[i] = (unsigned short)i;
    bitonic_any<RK_NT>(S, [&](int i, int q) {
        const unsigned short ia = idx[i], ib = idx[q];
        const double u = key[ia], v = key[ib];
        if (u > v || (u == v && ia > ib)) { idx[i] = ib; idx[q] = ia; }
    });
}

// out[i] = z of the average rank of key[i] among all S keys; idx sorts key.  out may be key: every thread holds its z values
// until all keys have been read.  Phi^-1 is the math library's normcdfinv: within 7.6e-16 (relative) of scipy's ndtri over the
// ranks of S = 8 and S = 8000 (profiles/rank_diag/README.md); a Newton step on Phi(z) - p with erfc only made it worse.
__device__ inline void rk_rank_z(const double *key, double *out, const unsigned short *idx, int S)
{
    const int tid = threadIdx.x;
    double zr[RK_PER];
#pragma unroll
    for (int k = 0; k < RK_PER; ++k) {
        const int p = tid + k * RK_NT;
        zr[k] = 0.0;
        if (p < S) {
            const double kv = key[idx[p]];
            int a = 0, b = p;                                         // first position of the tie run
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (key[idx[mid]] < kv) a = mid + 1; else b = mid;
            }
            const int lo = a;
            a = p; b = S - 1;                                         // last position of the tie run
            while (a < b) {
                const int mid = (a + b + 1) >> 1;
                if (key[idx[mid]] > kv) b = mid - 1; else a = mid;
            }
            const double r = 0.5 * (double)(lo + a + 2);              // average of the 1-based ranks lo + 1 ... a + 1
            zr[k] = normcdfinv((r - 0.375) / ((double)S + 0.25));
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RK_PER; ++k) {
        const int p = tid + k * RK_NT;
        if (p < S) out[idx[p]] = zr[k];
    }
    __syncthreads();
}

// Row means cm[H], centred sums of squares cs[H] of the series wrk [H][n], which is centred by row in place; *gq: sum of
// squares about the mean of all entries.  A row of equal values (a chain that did not move: all its z are one tie run) has
// that value as its mean and 0 as its sum of squares, not the rounding of n additions.  Returns whether any entry differs
// from the first (the same value in every thread).
__device__ inline int rk_rows(double *wrk, int H, int n, double *cm, double *cs, double *rs, double *part, double *gq_out)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double v00 = wrk[0];
    int differs = 0;
    for (int h = w; h < H; h += RK_NW) {
        const double *r = wrk + (size_t)h * n;
        const double r0 = r[0];
        double s = 0.0;
        int rowdiff = 0;
        for (int t = lane; t < n; t += 64) {
            const double v = r[t];
            rowdiff |= (v != r0);
            s += v;
        }
        s = wave_sum(s);
        rowdiff = __any(rowdiff);
        differs |= rowdiff | (r0 != v00);
        if (lane == 0) { rs[h] = s; cm[h] = rowdiff ? s / (double)n : r0; }   // a row of equal values: that value, exactly
    }
    differs = __syncthreads_or(differs);
    double tot = 0.0;
    for (int h = 0; h < H; ++h) tot += rs[h];
    const double gmean = tot / (double)(H * n);
    double gq = 0.0;
    for (int h = w; h < H; h += RK_NW) {
        double *r = wrk + (size_t)h * n;
        const double mu = cm[h];
        double q = 0.0;
        for (int t = lane; t < n; t += 64) {
            const double v = r[t];
            const double d = v - mu, e = v - gmean;
            q = fma(d, d, q);
            gq = fma(e, e, gq);
            r[t] = d;
        }
        q = wave_sum(q);
        if (lane == 0) cs[h] = q;
    }
    *gq_out = block_sum<RK_NW>(gq, part);
    __syncthreads();
    return differs;
}

// Geyer's effective sample size of the H rows of wrk as chains, capped at S log10 S; wrk is centred by row, cm / cs are its row
// means and centred sums of squares (rk_rows).  NaN when no entry differs from the first.  The same value in every thread.
__device__ inline double rk_ess(const double *wrk, int H, int n, int differs, const double *cm, const double *cs, double *part,
                                double *rho, double *sc)
{
    if (!differs) return NAN;
    const double tau = geyer_tau<RK_NW>([&](int h, int t) -> double { return wrk[(size_t)h * n + t]; }, H, n, cm, cs, part, rho, sc);
    const double S = (double)(H * n);
    const double e = S / tau;
    return isfinite(e) ? fmin(e, S * log10(S)) : NAN;
}

__device__ inline double rk_nan_max(double a, double b) { return (a != a || b != b) ? NAN : fmax(a, b); }
__device__ inline double rk_nan_min(double a, double b) { return (a != a || b != b) ? NAN : fmin(a, b); }

__global__ __launch_bounds__(RK_NT) void rank_kernel(RankArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int g = blockIdx.y, c = blockIdx.x;
    const int M = a.M, N = a.N, H = 2 * M, n = N / 2, S = H * n;
    double *val = lds;                                                // [S]   the split draws, row-major [H][n]
    double *wrk = val + S;                                            // [S]   work series
    double *part = wrk + S;                                           // [RK_NW][RK_LAGS]   wave partials
    double *cm = part + RK_NW * RK_LAGS;                              // [RK_MAX_ROWS]  row means
    double *cs = cm + RK_MAX_ROWS;                                    // [RK_MAX_ROWS]  row centred sums of squares
    double *rs = cs + RK_MAX_ROWS;                                    // [RK_MAX_ROWS]  row sums
    double *rho = rs + RK_MAX_ROWS;                                   // [RK_LAGS]
    double *sc = rho + RK_LAGS;                                       // [16]  scalars
    unsigned short *idx = (unsigned short *)(sc + 16);                // [S]
    const double *Xg = a.X + (size_t)g * M * a.unit_stride + c;
    const bool ex = a.expcol && a.expcol[c];
    const size_t o = (size_t)g * a.C + c;

    // ---- 1: split draws to LDS
    double v00 = Xg[0];
    if (ex) v00 = exp(v00);
    int nonfinite = 0, differs = 0;
    for (int i = tid; i < S; i += RK_NT) {
        const int h = i / n, t = i - h * n;
        const int m = h >> 1, tt = (h & 1) ? N - n + t : t;
        double v = Xg[(size_t)m * a.unit_stride + (size_t)tt * a.row_stride];
        if (ex) v = exp(v);
        nonfinite |= !isfinite(v);
        differs |= (v != v00);
        val[i] = v;
    }
    nonfinite = __syncthreads_or(nonfinite);
    differs = __syncthreads_or(differs);
    if (!a.rhat && a.zwhat == 2) {
        for (int i = tid; i < S; i += RK_NT) a.zout[i] = val[i];
        return;
    }
    if (nonfinite || !differs) {
        if (a.rhat) {
            if (tid == 0) { a.rhat[o] = NAN; a.bulk[o] = NAN; a.tail[o] = NAN; a.essm[o] = NAN; a.sd[o] = NAN; }
        } else {
            for (int i = tid; i < S; i += RK_NT) a.zout[i] = NAN;
        }
        return;
    }
    // ---- 2, 3: sort, quantiles, z of the draws
    rk_sort(val, idx, S);
    if (tid == 0) {
        const auto sorted = [&](int i) -> double { return val[idx[i]]; };
        sc[8] = numpy_quantile(sorted, S, a.q_lo);                    // np.percentile(Y, 100 p): q_lo, q_hi = (100 p) / 100
        sc[9] = numpy_quantile(sorted, S, a.q_hi);
        sc[10] = (S & 1) ? val[idx[S >> 1]] : (val[idx[(S >> 1) - 1]] + val[idx[S >> 1]]) / 2.0;
    }
    rk_rank_z(val, wrk, idx, S);
    const double q_lo = sc[8], q_hi = sc[9], med = sc[10];
    if (!a.rhat && a.zwhat == 0) {
        for (int i = tid; i < S; i += RK_NT) a.zout[i] = wrk[i];
        return;
    }
    // ---- 4: R-hat and ESS of z
    double gq;
    int df = rk_rows(wrk, H, n, cm, cs, rs, part, &gq);
    const double rhat_z = rhat_rows(H, n, cm, cs);
    const double ess_bulk = rk_ess(wrk, H, n, df, cm, cs, part, rho, sc);
    // ---- 5: folded draws
    __syncthreads();
    for (int i = tid; i < S; i += RK_NT) wrk[i] = fabs(val[i] - med);
    __syncthreads();
    rk_sort(wrk, idx, S);
    rk_rank_z(wrk, wrk, idx, S);
    if (!a.rhat) {
        for (int i = tid; i < S; i += RK_NT) a.zout[i] = wrk[i];
        return;
    }
    rk_rows(wrk, H, n, cm, cs, rs, part, &gq);
    const double rhat_f = rhat_rows(H, n, cm, cs);
    // ---- 6: the two indicator series and the draws themselves
    __syncthreads();
    for (int i = tid; i < S; i += RK_NT) wrk[i] = val[i] <= q_lo ? 1.0 : 0.0;
    __syncthreads();
    df = rk_rows(wrk, H, n, cm, cs, rs, part, &gq);
    const double ess_lo = rk_ess(wrk, H, n, df, cm, cs, part, rho, sc);
    __syncthreads();
    for (int i = tid; i < S; i += RK_NT) wrk[i] = val[i] <= q_hi ? 1.0 : 0.0;
    __syncthreads();
    df = rk_rows(wrk, H, n, cm, cs, rs, part, &gq);
    const double ess_hi = rk_ess(wrk, H, n, df, cm, cs, part, rho, sc);
    __syncthreads();
    for (int i = tid; i < S; i += RK_NT) wrk[i] = val[i];
    __syncthreads();
    df = rk_rows(wrk, H, n, cm, cs, rs, part, &gq);
    const double ess_mean = rk_ess(wrk, H, n, df, cm, cs, part, rho, sc);
    if (tid == 0) {
        a.rhat[o] = rk_nan_max(rhat_z, rhat_f);
        a.bulk[o] = ess_bulk;
        a.tail[o] = rk_nan_min(ess_lo, ess_hi);
        a.essm[o] = ess_mean;
        a.sd[o] = sqrt(gq / (double)(S - 1));
    }
}

static size_t rank_lds_bytes(int S)
{
    return ((size_t)2 * S + RK_SCRATCH) * sizeof(double) + (((size_t)S + 7) & ~(size_t)7) * sizeof(unsigned short);
}

static int rank_check_shape(const char *who, int G, int M, int N, int C, double p_lo, double p_hi)
{
    if (G < 1 || M < 1 || M > RK_MAX_CHAINS || N < 2 || C < 1) { set_error("%s: bad shape", who); return -1; }
    if (!(p_lo > 0.0) || !(p_hi < 1.0) || !(p_lo < p_hi)) { set_error("%s: tail probabilities need 0 < p_lo < p_hi < 1", who); return -1; }
    if ((size_t)2 * M * (N / 2) > (size_t)RK_MAX_DRAWS) {
        set_error("%s: %zu split draws per column, the kernel holds at most %d", who, (size_t)2 * M * (N / 2), RK_MAX_DRAWS);
        return -1;
    }
    return 0;
}

static int rank_launch(RankArgs a, int G, hipStream_t stream)
{
    const size_t lds = rank_lds_bytes(2 * a.M * (a.N / 2));
    static LdsAttrCache cache;
    BDRT_HIP(cache.ensure(lds, [&]() {
        return hipFuncSetAttribute((const void *)rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }));
    double *outs[5] = {a.rhat, a.bulk, a.tail, a.essm, a.sd};
    const double *X0 = a.X;
    const int rc = for_grid_y_chunks(G, [&](int g0, int gn) {
        const size_t o = (size_t)g0 * a.C;
        a.X = X0 + (size_t)g0 * a.M * a.unit_stride;
        if (outs[0]) { a.rhat = outs[0] + o; a.bulk = outs[1] + o; a.tail = outs[2] + o; a.essm = outs[3] + o; a.sd = outs[4] + o; }
        hipLaunchKernelGGL(rank_kernel, dim3(a.C, gn), dim3(RK_NT), lds, stream, a);
    });
    if (rc) return rc;
    BDRT_HIP(hipStreamSynchronize(stream));
    return 0;
}

// device draws -> host results: allocates the outputs (and the flags) on the device, launches, copies back
int rank_diagnostics_to_host(const double *dX, long unit_stride, long row_stride, const unsigned char *is_pos, int G, int M,
                             int N, int C, double p_lo, double p_hi, double *rhat, double *ess_bulk, double *ess_tail,
                             double *ess_mean, double *sd, hipStream_t stream)
{
    if (rank_check_shape("bdrt rank diagnostics", G, M, N, C, p_lo, p_hi)) return -1;
    const size_t gc = (size_t)G * C;
    DevBuf<double> dOut;
    DevBuf<unsigned char> dExp;
    BDRT_HIP(dOut.alloc(5 * gc));
    if (is_pos && upload(dExp, is_pos, (size_t)C)) return -10;
    RankArgs a;
    a.X = dX; a.unit_stride = unit_stride; a.row_stride = row_stride; a.expcol = dExp;
    a.M = M; a.N = N; a.C = C;
    a.q_lo = (100.0 * p_lo) / 100.0; a.q_hi = (100.0 * p_hi) / 100.0;
    a.rhat = dOut; a.bulk = dOut + gc; a.tail = dOut + 2 * gc; a.essm = dOut + 3 * gc; a.sd = dOut + 4 * gc;
    a.zout = nullptr; a.zwhat = 0;
    const int rc = rank_launch(a, G, stream);
    if (rc) return rc;
    double *const outs[5] = {rhat, ess_bulk, ess_tail, ess_mean, sd};
    return download_planes(dOut, gc, outs, 5);
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_rank_max_draws(void) { return RK_MAX_DRAWS; }

int bdrt_rank_diagnostics(const double *X, int G, int M, int N, int C, long ldx, const unsigned char *is_pos, double p_lo,
                          double p_hi, double *rhat, double *ess_bulk, double *ess_tail, double *ess_mean, double *sd)
{
    if (!X || ldx < C) { set_error("bdrt_rank_diagnostics: bad arguments"); return -1; }
    if (rank_check_shape("bdrt_rank_diagnostics", G, M, N, C, p_lo, p_hi)) return -1;
    bind_process_device();
    DevBuf<double> dX;
    if (upload_rows(dX, X, (size_t)G * M * N, ldx, C)) return -10;
    return rank_diagnostics_to_host(dX, (long)N * ldx, ldx, is_pos, G, M, N, C, p_lo, p_hi, rhat, ess_bulk, ess_tail, ess_mean, sd,
                                    nullptr);
}

int bdrt_debug_rank_z(const double *y, int M, int N, int is_pos, int what, double *z_out)
{
    if (!y || !z_out || what < 0 || what > 2) { set_error("bdrt_debug_rank_z: bad arguments"); return -1; }
    if (rank_check_shape("bdrt_debug_rank_z", 1, M, N, 1, 0.05, 0.95)) return -1;
    bind_process_device();
    const size_t nout = (size_t)2 * M * (N / 2);
    const unsigned char flag = is_pos != 0;
    DevBuf<double> dX, dZ;
    DevBuf<unsigned char> dExp;
    if (upload(dX, y, (size_t)M * N) || upload(dExp, &flag, 1)) return -10;
    BDRT_HIP(dZ.alloc(nout));
    RankArgs a;
    a.X = dX; a.unit_stride = N; a.row_stride = 1; a.expcol = dExp;
    a.M = M; a.N = N; a.C = 1;
    a.q_lo = 0.05; a.q_hi = 0.95;
    a.rhat = a.bulk = a.tail = a.essm = a.sd = nullptr;
    a.zout = dZ; a.zwhat = what;
    const int rc = rank_launch(a, 1, nullptr);
    if (rc) return rc;
    BDRT_HIP(hipMemcpy(z_out, dZ, nout * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
