// bdrt_diag.hip -- HMC convergence diagnostics on the device (include/bdrt.h section (4)).
//
// pystan's `check_hmc_diagnostics` / `summary` need, for every flat parameter column, the mean, the sd, the NON-split effective
// sample size (Geyer's initial positive + initial monotone sequence, Stan 2.19) and the split R-hat over the chains of one
// fit.  Definitions: tests/diag_numpy.py (the yardstick).  One launch reduces G groups (a group = the M chains of one
// spectrum) x C columns; element (g, m, t, c) of the draws is X[(g*M + m) * unit_stride + t * row_stride + c], which covers both
// a sampler's device buffer [unit][draw][D] and a host buffer [group][chain][draw][ld] copied to HBM.
//
// Schedule: one workgroup (4 waves) per (group, tile of TC adjacent columns).
//   staging   the tile's M*N*TC values go to LDS in row order (TC adjacent doubles per draw row) when they fit in
//             DG_STAGE_BYTES, otherwise every pass streams them from HBM (same arithmetic, same bits)
//   pass 1    chain sums and split-half sums (thread-strided partials, wave butterflies, the four waves summed in order)
//   pass 2    centred sums of squares of chains, halves and the whole column; the staged series is centred in place
//   pass 3    autocovariances in blocks of 64 lags (one lag per lane, the four waves split the draw range), chain-averaged;
//             thread 0 walks Geyer's pairs of the block and the loop stops at the block where the positive sequence ends
// Every sum has a fixed order, so results repeat bit for bit, and do not depend on TC or on staging (bdrt_stats.h: the
// reductions, R-hat over rows and Geyer's sequence, shared with bdrt_rank.hip).
#include <cmath>

#include "bdrt_host.h"
#include "bdrt_stats.h"

namespace bdrt {

constexpr int DG_NT = 256;                       // 4 waves
constexpr int DG_NW = DG_NT / 64;
constexpr int DG_LAGS = STATS_LAGS;              // lags per block of pass 3 (one per lane)
constexpr int DG_MAX_TC = 8;                     // adjacent columns per workgroup
constexpr int DG_MAX_CHAINS = 64;
constexpr size_t DG_STAGE_BYTES = 64 * 1024;     // two workgroups per CU

struct DiagArgs {
    const double *X;
    long unit_stride, row_stride;
    const unsigned char *expcol;                 // [C] device, or null: columns whose samples are exp(X) (Stan <lower=0>)
    int M, N, C, TC;
    double *mean, *sd, *neff, *rhat;             // [G x C] device
};

template <bool STAGED>
__global__ __launch_bounds__(DG_NT) void diag_kernel(DiagArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = blockIdx.y, c0 = blockIdx.x * a.TC;
    const int tc = min(a.TC, a.C - c0);
    const int M = a.M, N = a.N, MN = M * N, n = N / 2, h2 = N - n;
    const int PW = max(3 * M + 1, DG_LAGS);
    double *stage = lds;                                              // [TC][M*N]        (STAGED)
    double *part = lds + (STAGED ? (size_t)a.TC * MN : 0);           // [4][PW]          wave partials
    double *cm = part + 4 * PW;                                       // [M]              chain means
    double *hm = cm + M;                                              // [2M]             half means (first halves, then second)
    double *cs = hm + 2 * M;                                          // [M]              chain sums, then centred sums of squares
    double *hs = cs + M;                                              // [2M]             half centred sums of squares
    double *rho = hs + 2 * M;                                         // [DG_LAGS]        autocorrelations of the current block
    double *sc = rho + DG_LAGS;                                       // [8]              scalars
    const double *Xg = a.X + (size_t)g * M * a.unit_stride + c0;

    if (STAGED) {
        for (int i = tid; i < MN * tc; i += DG_NT) {
            const int r = i / tc, j = i - r * tc;                     // r = m * N + t
            const int m = r / N, t = r - m * N;
            double v = Xg[(size_t)m * a.unit_stride + (size_t)t * a.row_stride + j];
            if (a.expcol && a.expcol[c0 + j]) v = exp(v);
            stage[(size_t)j * MN + r] = v;
        }
        __syncthreads();
    }
    for (int j = 0; j < tc; ++j) {
        const int c = c0 + j;
        const bool ex = a.expcol && a.expcol[c];
        double *col = stage + (size_t)j * MN;
        auto val = [&](int m, int t) -> double {
            if (STAGED) return col[(size_t)m * N + t];
            const double v = Xg[(size_t)m * a.unit_stride + (size_t)t * a.row_stride + j];
            return ex ? exp(v) : v;
        };
        // ---- pass 1: chain sums, half sums; non-finite and constant-column flags
        const double v00 = val(0, 0);
        int nonfinite = 0, differs = 0;
        for (int m = 0; m < M; ++m) {
            double s = 0.0, s1 = 0.0, s2 = 0.0;
            for (int t = tid; t < N; t += DG_NT) {
                const double v = val(m, t);
                nonfinite |= !isfinite(v);
                differs |= (v != v00);
                s += v;
                if (t < n) s1 += v;
                else if (t >= h2) s2 += v;
            }
            s = wave_sum(s); s1 = wave_sum(s1); s2 = wave_sum(s2);
            if (lane == 0) { part[w * PW + 3 * m] = s; part[w * PW + 3 * m + 1] = s1; part[w * PW + 3 * m + 2] = s2; }
        }
        nonfinite = __syncthreads_or(nonfinite);
        differs = __syncthreads_or(differs);
        if (tid < 3 * M) {
            const double tot = waves_sum<DG_NW>(part + tid, PW);
            const int m = tid / 3, k = tid - 3 * m;
            if (k == 0) { cs[m] = tot; cm[m] = tot / (double)N; }
            else hm[(k - 1) * M + m] = tot / (double)n;
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int m = 0; m < M; ++m) s += cs[m];
            sc[0] = s / (double)MN;
        }
        __syncthreads();
        // ---- pass 2: centred sums of squares (chains, halves, whole column); centre the staged series in place
        const double gmean = sc[0];
        double gq = 0.0;
        for (int m = 0; m < M; ++m) {
            const double mu = cm[m], mu1 = hm[m], mu2 = hm[M + m];
            double q = 0.0, q1 = 0.0, q2 = 0.0;
            for (int t = tid; t < N; t += DG_NT) {
                const double v = val(m, t);
                const double d = v - mu, e = v - gmean;
                q = fma(d, d, q);
                gq = fma(e, e, gq);
                if (t < n) { const double f = v - mu1; q1 = fma(f, f, q1); }
                else if (t >= h2) { const double f = v - mu2; q2 = fma(f, f, q2); }
                if (STAGED) col[(size_t)m * N + t] = d;
            }
            q = wave_sum(q); q1 = wave_sum(q1); q2 = wave_sum(q2);
            if (lane == 0) { part[w * PW + 3 * m] = q; part[w * PW + 3 * m + 1] = q1; part[w * PW + 3 * m + 2] = q2; }
        }
        gq = wave_sum(gq);
        if (lane == 0) part[w * PW + 3 * M] = gq;
        __syncthreads();
        if (tid <= 3 * M) {
            const double tot = waves_sum<DG_NW>(part + tid, PW);
            const int m = tid / 3, k = tid - 3 * m;
            if (tid == 3 * M) sc[1] = tot;
            else if (k == 0) cs[m] = tot;
            else hs[(k - 1) * M + m] = tot;
        }
        __syncthreads();
        // ---- scalars: sd, split R-hat over the 2M halves
        const bool ok = !nonfinite && differs;
        if (tid == 0) {
            const size_t o = (size_t)g * a.C + c;
            a.mean[o] = gmean;
            a.sd[o] = MN > 1 ? sqrt(sc[1] / (double)(MN - 1)) : NAN;
            a.rhat[o] = ok ? rhat_rows(2 * M, n, hm, hs) : NAN;
        }
        // ---- pass 3: autocovariance blocks and Geyer's sequences; the streamed series is centred as it is read
        double tau = NAN;
        if (ok)
            tau = geyer_tau<DG_NW>([&](int m, int t) -> double { return STAGED ? col[(size_t)m * N + t] : val(m, t) - cm[m]; }, M,
                                   N, cm, cs, part, rho, sc + 2);
        if (tid == 0) a.neff[(size_t)g * a.C + c] = (ok && N >= 4) ? (double)MN / tau : NAN;
        __syncthreads();
    }
}

static size_t diag_lds_bytes(bool staged, int TC, int M, int N)
{
    const size_t PW = (size_t)std::max(3 * M + 1, DG_LAGS);
    return ((staged ? (size_t)TC * M * N : 0) + 4 * PW + 6 * (size_t)M + DG_LAGS + 8) * sizeof(double);
}

int diagnostics_device(const double *dX, long unit_stride, long row_stride, const unsigned char *dExp, int G, int M, int N, int C,
                       double *dMean, double *dSd, double *dNeff, double *dRhat, hipStream_t stream)
{
    if (G < 1 || M < 1 || M > DG_MAX_CHAINS || N < 1 || C < 1) { set_error("bdrt diagnostics: bad shape"); return -1; }
    if ((size_t)M * N > (size_t)1 << 30) { set_error("bdrt diagnostics: too many draws per group"); return -1; }
    const size_t per = (size_t)M * N * sizeof(double);
    const bool staged = per <= DG_STAGE_BYTES;
    const int TC = staged ? (int)std::min<size_t>(DG_MAX_TC, DG_STAGE_BYTES / per) : 1;
    const size_t lds = diag_lds_bytes(staged, TC, M, N);
    static LdsAttrCache cache_s, cache_t;
    if (staged)
        BDRT_HIP(cache_s.ensure(lds, [&]() {
            return hipFuncSetAttribute((const void *)diag_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        }));
    else
        BDRT_HIP(cache_t.ensure(lds, [&]() {
            return hipFuncSetAttribute((const void *)diag_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        }));
    const int tiles = (C + TC - 1) / TC;
    const int rc = for_grid_y_chunks(G, [&](int g0, int gn) {
        DiagArgs a;
        a.X = dX + (size_t)g0 * M * unit_stride;
        a.unit_stride = unit_stride; a.row_stride = row_stride; a.expcol = dExp;
        a.M = M; a.N = N; a.C = C; a.TC = TC;
        const size_t o = (size_t)g0 * C;
        a.mean = dMean + o; a.sd = dSd + o; a.neff = dNeff + o; a.rhat = dRhat + o;
        if (staged) hipLaunchKernelGGL(diag_kernel<true>, dim3(tiles, gn), dim3(DG_NT), lds, stream, a);
        else hipLaunchKernelGGL(diag_kernel<false>, dim3(tiles, gn), dim3(DG_NT), lds, stream, a);
    });
    if (rc) return rc;
    BDRT_HIP(hipStreamSynchronize(stream));
    return 0;
}

// device draws -> host results: allocates the outputs (and the flags) on the device, launches, copies back
int diagnostics_to_host(const double *dX, long unit_stride, long row_stride, const unsigned char *is_pos, int G, int M, int N,
                        int C, double *mean, double *sd, double *n_eff, double *rhat, hipStream_t stream)
{
    const size_t gc = (size_t)G * C;
    DevBuf<double> dOut;
    DevBuf<unsigned char> dExp;
    BDRT_HIP(dOut.alloc(4 * gc));
    if (is_pos && upload(dExp, is_pos, (size_t)C)) return -10;
    const int rc = diagnostics_device(dX, unit_stride, row_stride, dExp, G, M, N, C, dOut, dOut + gc, dOut + 2 * gc, dOut + 3 * gc,
                                      stream);
    if (rc) return rc;
    double *const outs[4] = {mean, sd, n_eff, rhat};
    return download_planes(dOut, gc, outs, 4);
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_diagnostics(const double *X, int G, int M, int N, int C, long ldx, const unsigned char *is_pos, double *mean,
                     double *sd, double *n_eff, double *rhat)
{
    if (!X || G < 1 || M < 1 || N < 1 || C < 1 || ldx < C) { set_error("bdrt_diagnostics: bad arguments"); return -1; }
    bind_process_device();
    DevBuf<double> dX;
    if (upload_rows(dX, X, (size_t)G * M * N, ldx, C)) return -10;
    return diagnostics_to_host(dX, (long)N * ldx, ldx, is_pos, G, M, N, C, mean, sd, n_eff, rhat, nullptr);
}

}  // extern "C"
