// bdrt_heldout.hip -- prediction at held-out frequencies and its equal-weight reduction (include/bdrt.h section (4b)).
//
// A fold of a cross-validation is a sampling fit on a training grid; what it says about a frequency it has not seen is the
// equal-weight mixture of the draws' normals there.  Definitions: tests/heldout_numpy.py (the yardstick); DESIGN.md 3.5g.
//
//   heldout_kernel         Z_hat and sigma_tot of constrained parameter rows [B][D] at H frequencies that are not on the problem's
//                          grid: per block v = A_test x (series) or conj(v) / |v|^2 (parallel), + Rinf + i w induc, then the error
//                          model of lik_point<false> (bdrt_model_terms.h).  A tall, skinny GEMM -- rows x K by K x 2H -- with a
//                          pointwise epilogue, on the VALU: at 2H <= 34 columns the 16 x 16 x 4 fp64 MFMA would pad H = 1 to a
//                          sixteenth of its tile and moves no more flop per cycle than v_fma_f64 does.  Whether HBM
//                          or LDS bandwidth bounds the loop has not been measured.  A workgroup takes R rows: the x part of
//                          each row goes to LDS once, in runs of consecutive doubles (rows of XS doubles, XS odd: conflict-free
//                          across rows), the prediction rows go to LDS as (re, im) pairs [k][h], one 16-byte read per k; a thread
//                          owns one (row, frequency), two accumulators per block, k ascending, every step an explicit fma.  So a
//                          row's result depends on nothing but the row: the same bits alone or anywhere in any batch.
//   heldout_reduce_kernel  one workgroup per (group, unit), on the transposed Z_hat and sigma_tot [G][N2][S]: the unit's
//                          log-likelihoods as predict_kernel forms them, lpd as psis_kernel sums it, mean, sd and pit as
//                          predict_kernel's equal-weight sums -- the same statements in the same order (bdrt_psis.h,
//                          bdrt_stats.h), hence the same bits; no select, no sort, no Pareto fit.
// bdrt_sampler_heldout runs both on a sampler's draws in chunks of groups (heldout_of_draws), as loo_of_draws does; the loop
// itself (heldout_of_draws_with) takes the reduction from its caller, so that bdrt_heldout_mix.hip runs its own through it.
#include <cfloat>
#include <cmath>

#include "bdrt_host.h"
#include "bdrt_psis.h"

namespace bdrt {

constexpr int HO_NT = 256;
constexpr size_t HO_LDS_SOFT = 64 * 1024;        // two workgroups per CU while the tile allows it
constexpr size_t HO_LDS_MAX = 160 * 1024;

struct HeldoutArgs {
    const double *par;                           // [B][D] constrained parameters (bdrt_transformed's params)
    size_t B;
    const double *w;                             // [H] 2 pi f
    const double *A;                             // per block [2H][K_b] row-major (real rows, then imaginary rows), block after block
    int H, R, XS, sumK;                          // R rows per workgroup, rows of XS doubles in LDS
    double *Zh, *Sg;                             // [B][2H]
};

__global__ __launch_bounds__(HO_NT) void heldout_kernel(const DevProblem *__restrict__ Pp, HeldoutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const DevProblem &P = *Pp;
    const int tid = threadIdx.x, H = a.H, D = P.D;
    double *As = lds;                                                 // [sumK][H][2]
    double *Xs = As + 2 * (size_t)a.sumK * H;                         // [R][XS]  x_b * x_scale, block after block
    double *Sc = Xs + (size_t)a.R * a.XS;                             // [R][6]   Rinf_raw, induc_raw, the four error raws
    const size_t r0 = (size_t)blockIdx.x * a.R;
    const int nr = (int)min((size_t)a.R, a.B - r0);
    const double *rows = a.par + r0 * (size_t)D;
    int koff = 0;
    size_t aoff = 0;
    for (int b = 0; b < P.nblocks; ++b) {
        const int K = P.blk[b].K, ox = P.blk[b].o_x;
        const double xs = P.blk[b].x_scale;
        const double *Ab = a.A + aoff;
        for (int i = tid; i < H * K; i += HO_NT) {
            const int h = i / K, k = i - h * K;
            double *d = As + 2 * ((size_t)(koff + k) * H + h);
            d[0] = Ab[i];
            d[1] = Ab[(size_t)H * K + i];
        }
        for (int i = tid; i < nr * K; i += HO_NT) {
            const int r = i / K, k = i - r * K;
            Xs[(size_t)r * a.XS + koff + k] = rows[(size_t)r * D + ox + k] * xs;
        }
        koff += K;
        aoff += 2 * (size_t)H * K;
    }
    for (int i = tid; i < nr * 6; i += HO_NT) {
        const int r = i / 6, q = i - 6 * r;
        Sc[i] = rows[(size_t)r * D + (q < 2 ? q : P.o_err + (q - 2))];
    }
    __syncthreads();
    const double smin2 = P.sigma_min * P.sigma_min;
    for (int item = tid; item < nr * H; item += HO_NT) {
        const int r = item / H, h = item - r * H;
        const double *x = Xs + (size_t)r * a.XS;
        double zr = 0.0, zi = 0.0;
        int k0 = 0;
        for (int b = 0; b < P.nblocks; ++b) {
            const int K = P.blk[b].K;
            const double *Ak = As + 2 * ((size_t)k0 * H + h);
            double yr = 0.0, yi = 0.0;
            for (int k = 0; k < K; ++k) {
                const double xv = x[k0 + k];
                yr = fma(Ak[0], xv, yr);
                yi = fma(Ak[1], xv, yi);
                Ak += 2 * H;
            }
            if (P.blk[b].is_parallel) {                               // conj(v) / |v|^2
                const double idn = 1.0 / (yr * yr + yi * yi);
                zr += yr * idn;
                zi += -yi * idn;
            } else {
                zr += yr;
                zi += yi;
            }
            k0 += K;
        }
        const double *s = Sc + 6 * r;
        const double s_res = 0.05 * s[2], a_p = 0.05 * s[3], a_r = 0.05 * s[4], a_i = 0.05 * s[5];
        zr += 100.0 * s[0];
        zi += (s[1] * P.induc_scale) * a.w[h];
        const double c0 = s_res * s_res + smin2, ap2 = a_p * a_p, ar2 = a_r * a_r, ai2 = a_i * a_i;
        const double common = ar2 * zr * zr + ai2 * zi * zi;
        const double s2_re = c0 + ap2 * zr * zr + common, s2_im = c0 + ap2 * zi * zi + common;
        const size_t e = (r0 + r) * 2 * (size_t)H + h;
        a.Zh[e] = zr;
        a.Zh[e + H] = zi;
        a.Sg[e] = sqrt(s2_re);
        a.Sg[e + H] = sqrt(s2_im);
    }
}

struct HeldoutReduceArgs {
    const double *Tm, *Ts;                       // [G][N2][S] device: Z_hat and sigma_tot, transposed
    const double *z;                             // [G][N2] device
    int S, N2, U, pair;
    double c0, log_S;
    double *out;                                 // 3 planes [G][N2]: mean, sd, pit
    double *lpd;                                 // [G][U]
};

__global__ __launch_bounds__(LO_NT) void heldout_reduce_kernel(HeldoutReduceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int S = a.S, nh = a.pair + 1;
    const size_t c = blockIdx.x, g = c / a.U;
    const int j = (int)(c - g * a.U);
    double *col = lds;                                                // [S] the unit's log-likelihoods
    double *red = col + S;                                            // [LP_RED]
    const size_t plane = (size_t)gridDim.x / a.U * a.N2;              // G N2
    const size_t e0 = g * a.N2 + j, e1 = e0 + a.U;                    // the unit's scalars (e1: pairs only)
    const double *mu0 = a.Tm + e0 * S, *sg0 = a.Ts + e0 * S;
    const double *mu1 = a.Tm + e1 * S, *sg1 = a.Ts + e1 * S;
    const double z0 = a.z[e0], z1 = a.pair ? a.z[e1] : 0.0;

    // ---- log-likelihoods to LDS, extremes (predict_kernel, step 1)
    int bad = 0;
    double mx = -INFINITY, mn = INFINITY;
    for (int s = tid; s < S; s += LO_NT) {
        double v = lo_normal_loglik(z0, mu0[s], sg0[s], a.c0);
        if (a.pair) v = v + lo_normal_loglik(z1, mu1[s], sg1[s], a.c0);
        bad |= !isfinite(v);
        col[s] = v;
        mx = fmax(mx, v);
        mn = fmin(mn, v);
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid < 3 * nh) a.out[(size_t)(tid / nh) * plane + ((tid % nh) ? e1 : e0)] = NAN;
        if (tid == 0) a.lpd[c] = NAN;
        return;
    }
    mx = block_max<LO_NW>(mx, red);
    mn = -block_max<LO_NW>(-mn, red);
    // ---- the equal-weight sums (predict_kernel, step 4; its slot 0, the denominator of the smoothed weights, has no use here)
    double eq[LP_NSUM - 1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = tid; s < S; s += LO_NT) {
        double d0, q0, p0, d1 = 0.0, q1 = 0.0, p1 = 0.0;
        predict_terms(mu0[s], sg0[s], z0, d0, q0, p0);
        if (a.pair) predict_terms(mu1[s], sg1[s], z1, d1, q1, p1);
        eq[0] += d0; eq[1] += q0; eq[2] += p0;
        eq[3] += d1; eq[4] += q1; eq[5] += p1;
    }
    block_sums<LP_NSUM - 1>(eq, red);
    const double dS = (double)S;
    const bool second = tid == 1;                                     // thread h writes scalar h of the unit
    if (tid < nh) {
        const double m1 = (second ? eq[3] : eq[0]) / dS, m2 = (second ? eq[4] : eq[1]) / dS, p = (second ? eq[5] : eq[2]) / dS;
        predict_write(a.out, plane, second ? e1 : e0, second ? z1 : z0, m1, m2, p);
    }
    // ---- lpd = logsumexp(ll) - log S (psis_kernel, step 1)
    if (mx == mn) {
        if (tid == 0) a.lpd[c] = mx;
        return;
    }
    double se = 0.0;
    for (int s = tid; s < S; s += LO_NT) se += exp(col[s] - mx);
    se = block_sum<LO_NW>(se, red);
    if (tid == 0) a.lpd[c] = (mx + log(se)) - a.log_S;
}

// ---- device-pointer cores: each enqueues on `stream` and returns; the caller synchronises
// dPar [B][D], dW [H] (2 pi f), dA (packed as HeldoutArgs::A) -> dZh, dSg [B][2H]
int heldout_transformed_device(const char *who, Problem &P, const double *dPar, size_t B, const double *dW, const double *dA, int H,
                               double *dZh, double *dSg, hipStream_t stream, bool allow_outliers)
{
    if (P.dev.outlier_mode && !allow_outliers) {
        set_error("%s: outlier error models are refused: a held-out point has no sigma_out of its own", who);
        return -2;
    }
    if (B == 0) return 0;
    int sumK = 0;
    for (int b = 0; b < P.dev.nblocks; ++b) sumK += P.dev.blk[b].K;
    const int XS = sumK | 1;
    const size_t bytesA = 2 * (size_t)sumK * H * sizeof(double), row = ((size_t)XS + 6) * sizeof(double);
    int R = 64;
    while (R > 1 && bytesA + R * row > HO_LDS_SOFT) R >>= 1;
    const size_t lds = bytesA + R * row;
    if (lds > HO_LDS_MAX) {
        set_error("%s: %d held-out frequencies x %d basis functions do not fit the LDS of a CU", who, H, sumK);
        return -2;
    }
    const size_t grid = (B + R - 1) / R;
    if (grid > 0x7fffffffull) { set_error("%s: too many rows", who); return -2; }
    static LdsAttrCache cache;
    BDRT_HIP(cache.ensure(lds, [&]() {
        return hipFuncSetAttribute((const void *)heldout_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }));
    HeldoutArgs a;
    a.par = dPar; a.B = B; a.w = dW; a.A = dA; a.H = H; a.R = R; a.XS = XS; a.sumK = sumK; a.Zh = dZh; a.Sg = dSg;
    hipLaunchKernelGGL(heldout_kernel, dim3((unsigned)grid), dim3(HO_NT), lds, stream, (const DevProblem *)P.d_dev, a);
    BDRT_HIP(hipGetLastError());
    return 0;
}

// dTm, dTs [G][N2][S], dz [G][N2] -> dOut: 3 planes of G N2 (mean, sd, pit), then lpd [G U]
int heldout_reduce_device(const double *dTm, const double *dTs, const double *dz, int G, int S, int N2, int pair, double *dOut,
                          hipStream_t stream)
{
    const int U = pair ? N2 / 2 : N2;
    const size_t units = (size_t)G * U, nsc = (size_t)G * N2, lds = ((size_t)S + LP_RED) * sizeof(double);
    static LdsAttrCache cache;
    BDRT_HIP(cache.ensure(lds, [&]() {
        return hipFuncSetAttribute((const void *)heldout_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }));
    HeldoutReduceArgs a;
    a.Tm = dTm; a.Ts = dTs; a.z = dz; a.S = S; a.N2 = N2; a.U = U; a.pair = pair;
    a.c0 = -0.5 * std::log(2.0 * M_PI); a.log_S = std::log((double)S);
    a.out = dOut; a.lpd = dOut + 3 * nsc;
    hipLaunchKernelGGL(heldout_reduce_kernel, dim3((unsigned)units), dim3(LO_NT), lds, stream, a);
    BDRT_HIP(hipGetLastError());
    return 0;
}

// host copies of the held-out grid -> device: w = 2 pi f [H] and the packed prediction rows
int heldout_upload_grid(const Problem &P, const double *freq, int H, const double *A, DevBuf<double> &dW, DevBuf<double> &dA)
{
    std::vector<double> w((size_t)H);
    for (int h = 0; h < H; ++h) w[h] = 2.0 * M_PI * freq[h];
    size_t sumK = 0;
    for (int b = 0; b < P.dev.nblocks; ++b) sumK += (size_t)P.dev.blk[b].K;
    if (upload(dW, w.data(), (size_t)H) || upload(dA, A, 2 * (size_t)H * sumK)) return -10;
    return 0;
}

int heldout_check_grid(const char *who, const double *freq, int H)
{
    for (int h = 0; h < H; ++h)
        if (!std::isfinite(freq[h]) || !(freq[h] > 0.0)) { set_error("%s: freq_test[%d] = %g is not a positive number", who, h, freq[h]); return -1; }
    return 0;
}

// what one group adds to a chunk's scratch: per draw row the parameters, lp, Z_hat and sigma_tot at the 2H held-out columns and
// the two transposes of the part
static size_t heldout_group_bytes(const LooDraws &j, int H)
{
    const size_t S = (size_t)j.chains * j.n_draws;
    return (S * ((size_t)j.prob->dev.D + 1 + 4 * (size_t)H + 2 * (size_t)j.ncols) + 4 * (size_t)j.ncols) * sizeof(double);
}

// The held-out reduction of draws that are on the device.  j: the job of the LOO reductions with pair, col0, ncols counted in the
// 2H held-out columns (reff_* unused); z_test [G][2H] on the host.  Outputs on the host: lpd [G][U], mean, sd, pit [G][ncols].
int heldout_of_draws(const LooDraws &j, const double *freq, int H, const double *A, const double *z_test, double *lpd, double *mean,
                     double *sd, double *pit)
{
    return heldout_of_draws_with("bdrt_sampler_heldout", j, freq, H, A, z_test, false,
                                 [&](const double *dTm, const double *dTs, const double *dz, int gn, int S, double *dOut) {
                                     return heldout_reduce_device(dTm, dTs, dz, gn, S, j.ncols, j.pair, dOut, j.stream);
                                 }, lpd, mean, sd, pit);
}

// the same with the reduction of a chunk's groups left to the caller (bdrt_heldout_mix.hip has another); allow_outliers: sg is then
// the base scale
int heldout_of_draws_with(const char *who, const LooDraws &j, const double *freq, int H, const double *A, const double *z_test,
                          bool allow_outliers, const HeldoutReduceFn &reduce, double *lpd, double *mean, double *sd, double *pit)
{
    Problem &P = *j.prob;
    BDRT_HIP(hipSetDevice(P.device));
    const int S = j.chains * j.n_draws, U = j.pair ? j.ncols / 2 : j.ncols;
    const size_t N2 = 2 * (size_t)H;
    const size_t budget = j.chunk_bytes ? j.chunk_bytes : LOO_CHUNK_DEFAULT;
    const size_t fit = std::min(budget / heldout_group_bytes(j, H), ((size_t)1 << 30) / (size_t)S);
    const int gmax = (int)std::max<size_t>(1, std::min<size_t>(fit, (size_t)j.G));
    const size_t rows = (size_t)gmax * S;
    std::vector<double> zpart((size_t)j.G * j.ncols);
    for (int g = 0; g < j.G; ++g) std::copy(z_test + g * N2 + j.col0, z_test + g * N2 + j.col0 + j.ncols, zpart.begin() + (size_t)g * j.ncols);
    DevBuf<double> dW, dA, dz, par, lp, zh, sg, Tm, Ts, out;
    if (heldout_upload_grid(P, freq, H, A, dW, dA) || upload(dz, zpart.data(), zpart.size())) return -10;
    BDRT_HIP(par.alloc(rows * P.dev.D));
    BDRT_HIP(lp.alloc(rows));
    BDRT_HIP(zh.alloc(rows * N2));
    BDRT_HIP(sg.alloc(rows * N2));
    BDRT_HIP(Tm.alloc(rows * j.ncols));
    BDRT_HIP(Ts.alloc(rows * j.ncols));
    BDRT_HIP(out.alloc((size_t)gmax * (3 * (size_t)j.ncols + U)));
    for (int g0 = 0; g0 < j.G; g0 += gmax) {
        const int gn = std::min(gmax, j.G - g0);
        const size_t units = (size_t)gn * U, nsc = (size_t)gn * j.ncols, o = (size_t)g0 * U, osc = (size_t)g0 * j.ncols;
        if (nsc > 0x7fffffffull) { set_error("%s: too many observations", who); return -2; }
        int rc;
        if ((rc = launch_logp_grad(&P, j.draws + (size_t)g0 * S * P.dev.D, nullptr, (int)((size_t)gn * S), 0, lp, nullptr, par, nullptr, nullptr,
                                   j.stream)) ||
            (rc = heldout_transformed_device(who, P, par, (size_t)gn * S, dW, dA, H, zh, sg, j.stream, allow_outliers)) ||
            (rc = loo_transpose_device(who, zh.p + j.col0, Tm, gn, S, j.ncols, N2, j.stream)) ||
            (rc = loo_transpose_device(who, sg.p + j.col0, Ts, gn, S, j.ncols, N2, j.stream)) ||
            (rc = reduce(Tm, Ts, dz.p + osc, gn, S, out)))
            return rc;
        BDRT_HIP(hipStreamSynchronize(j.stream));
        double *const outs[3] = {mean + osc, sd + osc, pit + osc};
        if (download_planes(out, nsc, outs, 3)) return -10;
        BDRT_HIP(hipMemcpy(lpd + o, out.p + 3 * nsc, units * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_heldout_transformed(bdrt_problem *p, const double *params, int B, const double *freq_test, int H, const double *A_test,
                             double *Z_hat, double *sigma_tot)
{
    if (!p || !params || !freq_test || !A_test || !Z_hat || !sigma_tot || B < 0 || H < 1) {
        set_error("bdrt_heldout_transformed: bad arguments");
        return -1;
    }
    Problem &P = p->impl;
    if (P.dev.outlier_mode) {
        set_error("bdrt_heldout_transformed: outlier error models are refused: a held-out point has no sigma_out of its own");
        return -2;
    }
    if (heldout_check_grid("bdrt_heldout_transformed", freq_test, H)) return -1;
    if (B == 0) return 0;
    BDRT_HIP(hipSetDevice(P.device));
    const size_t nz = (size_t)B * 2 * H;
    DevBuf<double> dW, dA, dPar, dZh, dSg;
    if (heldout_upload_grid(P, freq_test, H, A_test, dW, dA) || upload(dPar, params, (size_t)B * P.dev.D)) return -10;
    BDRT_HIP(dZh.alloc(nz));
    BDRT_HIP(dSg.alloc(nz));
    if (const int rc = heldout_transformed_device("bdrt_heldout_transformed", P, dPar, (size_t)B, dW, dA, H, dZh, dSg, P.stream, false)) return rc;
    if (download(Z_hat, dZh.p, nz, P.stream) || download(sigma_tot, dSg.p, nz, P.stream)) return -10;
    BDRT_HIP(hipStreamSynchronize(P.stream));
    return 0;
}

int bdrt_heldout_reduce(const double *Zhat, const double *sig, const double *z, int G, int S, int N2, int pair, double *lpd,
                        double *mean, double *sd, double *pit)
{
    if (!Zhat || !sig || !z || !lpd || !mean || !sd || !pit || G < 1 || S < 2 || N2 < 1 || (pair != 0 && pair != 1) ||
        (pair && (N2 & 1))) {
        set_error("bdrt_heldout_reduce: bad arguments");
        return -1;
    }
    if (S > LO_MAX_S) { set_error("bdrt_heldout_reduce: %d draws per unit, the kernel holds at most %d", S, LO_MAX_S); return -2; }
    const int U = pair ? N2 / 2 : N2;
    const size_t units = (size_t)G * U, nsc = (size_t)G * N2, nel = nsc * S;
    if (nsc > 0x7fffffffull) { set_error("bdrt_heldout_reduce: too many observations"); return -2; }
    bind_process_device();
    DevBuf<double> dIn, dTm, dTs, dz, dOut;
    if (upload(dz, z, nsc)) return -10;
    BDRT_HIP(dTm.alloc(nel));
    BDRT_HIP(dTs.alloc(nel));
    BDRT_HIP(dIn.alloc(nel));
    BDRT_HIP(hipMemcpy(dIn, Zhat, nel * sizeof(double), hipMemcpyHostToDevice));
    if (const int rc = loo_transpose_device("bdrt_heldout_reduce", dIn, dTm, G, S, N2, (size_t)N2, nullptr)) return rc;
    BDRT_HIP(hipMemcpy(dIn, sig, nel * sizeof(double), hipMemcpyHostToDevice));      // (stream order: behind the first transpose)
    if (const int rc = loo_transpose_device("bdrt_heldout_reduce", dIn, dTs, G, S, N2, (size_t)N2, nullptr)) return rc;
    BDRT_HIP(dOut.alloc(3 * nsc + units));
    if (const int rc = heldout_reduce_device(dTm, dTs, dz, G, S, N2, pair, dOut, nullptr)) return rc;
    BDRT_HIP(hipDeviceSynchronize());
    double *const outs[3] = {mean, sd, pit};
    if (download_planes(dOut, nsc, outs, 3)) return -10;
    BDRT_HIP(hipMemcpy(lpd, dOut + 3 * nsc, units * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
