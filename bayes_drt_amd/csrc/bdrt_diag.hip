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
// Every sum has a fixed order, so results repeat bit for bit, and do not depend on TC or on staging.  This file is compiled
// with -ffp-contract=off: the products that accumulate are explicit fma() calls, everything else is rounded separately.
#include <cmath>

#include "bdrt_host.h"

namespace bdrt {

constexpr int DG_NT = 256;                       // 4 waves
constexpr int DG_LAGS = 64;                      // lags per block of pass 3 (one per lane)
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

__device__ inline double dg_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

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
            s = dg_wave_sum(s); s1 = dg_wave_sum(s1); s2 = dg_wave_sum(s2);
            if (lane == 0) { part[w * PW + 3 * m] = s; part[w * PW + 3 * m + 1] = s1; part[w * PW + 3 * m + 2] = s2; }
        }
        nonfinite = __syncthreads_or(nonfinite);
        differs = __syncthreads_or(differs);
        if (tid < 3 * M) {
            const double tot = ((part[tid] + part[PW + tid]) + part[2 * PW + tid]) + part[3 * PW + tid];
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
            q = dg_wave_sum(q); q1 = dg_wave_sum(q1); q2 = dg_wave_sum(q2);
            if (lane == 0) { part[w * PW + 3 * m] = q; part[w * PW + 3 * m + 1] = q1; part[w * PW + 3 * m + 2] = q2; }
        }
        gq = dg_wave_sum(gq);
        if (lane == 0) part[w * PW + 3 * M] = gq;
        __syncthreads();
        if (tid <= 3 * M) {
            const double tot = ((part[tid] + part[PW + tid]) + part[2 * PW + tid]) + part[3 * PW + tid];
            const int m = tid / 3, k = tid - 3 * m;
            if (tid == 3 * M) sc[1] = tot;
            else if (k == 0) cs[m] = tot;
            else hs[(k - 1) * M + m] = tot;
        }
        __syncthreads();
        // ---- scalars: sd, split R-hat, the variances of n_eff
        if (tid == 0) {
            const size_t o = (size_t)g * a.C + c;
            a.mean[o] = gmean;
            a.sd[o] = MN > 1 ? sqrt(sc[1] / (double)(MN - 1)) : NAN;
            const bool ok = !nonfinite && differs;
            double rh = NAN;
            if (ok && n >= 2) {
                const int H = 2 * M;
                double hbar = 0.0, W = 0.0, B = 0.0;
                for (int h = 0; h < H; ++h) hbar += hm[h];
                hbar /= (double)H;
                for (int h = 0; h < H; ++h) { const double d = hm[h] - hbar; B = fma(d, d, B); }
                B = (double)n * (B / (double)(H - 1));
                for (int h = 0; h < H; ++h) W += hs[h] / (double)(n - 1);
                W /= (double)H;
                rh = sqrt((B / W + (double)(n - 1)) / (double)n);
            }
            a.rhat[o] = rh;
            double mean_var = 0.0;
            for (int m = 0; m < M; ++m) mean_var += (cs[m] / (double)N) * (double)N / (double)(N - 1);
            mean_var /= (double)M;
            double var_plus = mean_var * (double)(N - 1) / (double)N;
            if (M > 1) {
                double mb = 0.0, vb = 0.0;
                for (int m = 0; m < M; ++m) mb += cm[m];
                mb /= (double)M;
                for (int m = 0; m < M; ++m) { const double d = cm[m] - mb; vb = fma(d, d, vb); }
                var_plus += vb / (double)(M - 1);
            }
            sc[2] = mean_var;
            sc[3] = var_plus;
            sc[4] = (ok && N >= 4) ? 1.0 : 0.0;
            if (!(ok && N >= 4)) a.neff[o] = NAN;
        }
        __syncthreads();
        if (sc[4] == 0.0) { __syncthreads(); continue; }
        // ---- pass 3: autocovariance blocks and Geyer's sequences (state in thread 0)
        const double mean_var = sc[2], var_plus = sc[3];
        const int chunk = (N + 3) / 4, tw0 = min(N, w * chunk), tw1 = min(N, tw0 + chunk);
        double acc_pm = 0.0, prev_pm = 0.0;                           // thread 0: sum of monotone pair sums so far, last one
        for (int k0 = 0;; k0 += DG_LAGS) {
            const int k = k0 + lane;
            double s = 0.0;
            if (k < N) {
                const int te = min(tw1, N - k);
                for (int m = 0; m < M; ++m) {
                    if (STAGED) {
                        const double *cc = col + (size_t)m * N;
                        for (int t = tw0; t < te; ++t) s = fma(cc[t], cc[t + k], s);
                    } else {
                        const double mu = cm[m];
                        for (int t = tw0; t < te; ++t) s = fma(val(m, t) - mu, val(m, t + k) - mu, s);
                    }
                }
            }
            part[w * PW + lane] = s;
            __syncthreads();
            if (tid < DG_LAGS) {
                const double S = ((part[tid] + part[PW + tid]) + part[2 * PW + tid]) + part[3 * PW + tid];
                const double acov_mean = (S / (double)N) / (double)M;
                rho[tid] = 1.0 - (mean_var - acov_mean) / var_plus;
            }
            __syncthreads();
            if (tid == 0) {
                double tau = NAN;
                bool done = k0 + DG_LAGS >= N;                        // (never reached: the sequence stops before lag N - 2)
                for (int l = 0; l < DG_LAGS && !(tau == tau); l += 2) {
                    const int jp = (k0 + l) >> 1;                     // pair jp = lags (2 jp, 2 jp + 1)
                    const double ev = jp == 0 ? 1.0 : rho[l], od = rho[l + 1];
                    const bool cont = (2 * jp + 1 < N - 4) && (ev + od > 0.0);
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
                if (tau == tau) done = true;
                if (done) a.neff[(size_t)g * a.C + c] = (double)MN / tau;
                sc[5] = done ? 1.0 : 0.0;
            }
            __syncthreads();
            const bool done = sc[5] != 0.0;
            __syncthreads();
            if (done) break;
        }
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
    for (int g0 = 0; g0 < G; g0 += 65535) {
        const int gn = std::min(G - g0, 65535);
        DiagArgs a;
        a.X = dX + (size_t)g0 * M * unit_stride;
        a.unit_stride = unit_stride; a.row_stride = row_stride; a.expcol = dExp;
        a.M = M; a.N = N; a.C = C; a.TC = TC;
        const size_t o = (size_t)g0 * C;
        a.mean = dMean + o; a.sd = dSd + o; a.neff = dNeff + o; a.rhat = dRhat + o;
        if (staged) hipLaunchKernelGGL(diag_kernel<true>, dim3(tiles, gn), dim3(DG_NT), lds, stream, a);
        else hipLaunchKernelGGL(diag_kernel<false>, dim3(tiles, gn), dim3(DG_NT), lds, stream, a);
        BDRT_HIP(hipGetLastError());
    }
    BDRT_HIP(hipStreamSynchronize(stream));
    return 0;
}

// device draws -> host results: allocates the outputs (and the flags) on the device, launches, copies back
int diagnostics_to_host(const double *dX, long unit_stride, long row_stride, const unsigned char *is_pos, int G, int M, int N,
                        int C, double *mean, double *sd, double *n_eff, double *rhat, hipStream_t stream)
{
    double *dOut = nullptr;
    unsigned char *dExp = nullptr;
    const size_t nb = (size_t)G * C * sizeof(double);
    hipError_t e = hipMalloc((void **)&dOut, 4 * nb);
    if (e == hipSuccess && is_pos) {
        e = hipMalloc((void **)&dExp, (size_t)C);
        if (e == hipSuccess) e = hipMemcpy(dExp, is_pos, (size_t)C, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        hipFree(dOut); hipFree(dExp);
        set_error("bdrt diagnostics: %s", hipGetErrorString(e));
        return -10;
    }
    const size_t gc = (size_t)G * C;
    int rc = diagnostics_device(dX, unit_stride, row_stride, dExp, G, M, N, C, dOut, dOut + gc, dOut + 2 * gc, dOut + 3 * gc,
                                stream);
    double *outs[4] = {mean, sd, n_eff, rhat};
    for (int k = 0; k < 4 && rc == 0; ++k) {
        if (!outs[k]) continue;
        e = hipMemcpy(outs[k], dOut + k * gc, nb, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { set_error("bdrt diagnostics: %s", hipGetErrorString(e)); rc = -10; }
    }
    hipFree(dOut); hipFree(dExp);
    return rc;
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_diagnostics(const double *X, int G, int M, int N, int C, long ldx, const unsigned char *is_pos, double *mean,
                     double *sd, double *n_eff, double *rhat)
{
    if (!X || G < 1 || M < 1 || N < 1 || C < 1 || ldx < C) { set_error("bdrt_diagnostics: bad arguments"); return -1; }
    bind_process_device();
    double *dX = nullptr;
    const size_t nb = ((size_t)G * M * N - 1) * ldx * sizeof(double) + (size_t)C * sizeof(double);
    if (hipMalloc((void **)&dX, nb) != hipSuccess) { set_error("bdrt_diagnostics: hipMalloc(%zu) failed", nb); return -10; }
    if (hipMemcpy(dX, X, nb, hipMemcpyHostToDevice) != hipSuccess) { hipFree(dX); set_error("bdrt_diagnostics: copy failed"); return -10; }
    const int rc = diagnostics_to_host(dX, (long)N * ldx, ldx, is_pos, G, M, N, C, mean, sd, n_eff, rhat, nullptr);
    hipFree(dX);
    return rc;
}

}  // extern "C"
