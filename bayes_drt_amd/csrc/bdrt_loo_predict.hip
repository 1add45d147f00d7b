// bdrt_loo_predict.hip -- PSIS-LOO predictive checks of HMC draws on the device (include/bdrt.h section (4)).
//
// The likelihood is `Z ~ normal(Z_hat, sigma_tot)`, so the leave-one-out predictive distribution of a scalar observation is a
// mixture of the draws' normals under the Pareto-smoothed importance weights of its unit (one scalar, or the real and the
// imaginary part of one frequency left out together).  Its mean, its sd and its cdf at the datum (the LOO-PIT) are weighted
// sums over the draws; the same sums with equal weights are the in-sample posterior predictive.  Definitions:
// tests/loo_predict_numpy.py (the yardstick).  Z_hat and sigma_tot arrive row-major ([G][S][N2]) and are transposed to
// [G][N2][S] (bdrt_loo.hip's transpose_kernel), so the draws of a scalar are contiguous.
//
//   predict_kernel    one workgroup (8 waves) per unit:
//     1  the unit's log-likelihoods, formed with the arithmetic of loglik_kernel, go to LDS; max and min
//     2  x = min(ll) - ll replaces them
//     3  the (M+1)-th largest x by radix select; cutoff = max(that, log DBL_MIN)                    (bdrt_psis.h)
//     4  one sweep: draws above the cutoff leave their draw INDEX in the tail buffer (<= ceil(S/5) ints), the others add their
//        raw-weight terms to the body sums -- the denominator and, per scalar, d = mu - z, sigma^2 + d^2 and Phi(-d / sigma);
//        every draw adds the same three terms to the equal-weight sums
//     5  the tail's x values are gathered through registers into the head of the column, which is dead from here on; the tail
//        is sorted by (value, draw index): the stable order of the numpy statement, and a total order, so the compaction order
//        (the one thing atomics decide) is erased
//     6  Zhang-Stephens fit and smoothed tail values                                                (bdrt_psis.h)
//     7  the tail sums gather mu and sigma of each tail draw by its index; normalise and write
// LDS: the column [S] (later tail | y | smoothed tail, 3 ceil(S/5) <= S), the tail indices, scratch: 148 772 B at S = 16 384,
// so the draw limit is bdrt_psis_loo's.  Every sum is a per-thread strided partial, a wave butterfly and the eight wave partials
// added in order (bdrt_stats.h), so a unit gives the same bits alone or in any batch.  Cutoff, tail and k-hat are those of
// psis_kernel on bdrt_pointwise_loglik's output to the bit: the steps are one copy in bdrt_psis.h.
#include <cfloat>
#include <cmath>

#include "bdrt_host.h"
#include "bdrt_psis.h"

namespace bdrt {

constexpr int LP_STAGE = (((LO_MAX_S + 4) / 5) + LO_NT - 1) / LO_NT;         // tail values a thread holds in step 5: 7
__global__ __launch_bounds__(LO_NT) void predict_kernel(PredictArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int S = a.S, nh = a.pair + 1;
    const size_t c = blockIdx.x, g = c / a.U;
    const int j = (int)(c - g * a.U);
    double *col = lds;                                                // [S]      ll, then x, then tail | y | smoothed tail
    double *red = col + S;                                            // [LP_RED]
    double *bj = red + LP_RED;                                        // [LO_MAX_M] each
    double *kj = bj + LO_MAX_M;
    double *Lj = kj + LO_MAX_M;
    double *wj = Lj + LO_MAX_M;
    double *sc = wj + LO_MAX_M;                                       // [4]
    int *hist = (int *)(sc + 4);                                      // [256]
    int *si = hist + 256;                                             // [4]
    int *idx = si + 4;                                                // [cap]    draw indices of the tail
    const size_t plane = (size_t)gridDim.x / a.U * a.N2;              // G N2
    const size_t e0 = g * a.N2 + j, e1 = e0 + a.U;                    // the unit's scalars (e1: pairs only)
    const double *mu0 = a.Tm + e0 * S, *sg0 = a.Ts + e0 * S;
    const double *mu1 = a.Tm + e1 * S, *sg1 = a.Ts + e1 * S;
    const double z0 = a.z[e0], z1 = a.pair ? a.z[e1] : 0.0;

    // ---- 1: log-likelihoods to LDS; extremes
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
        if (tid < 6 * nh) a.out[(size_t)(tid / nh) * plane + ((tid % nh) ? e1 : e0)] = NAN;
        if (tid == 0) { a.khat[c] = NAN; a.ntail[c] = 0; }
        return;
    }
    mx = block_max<LO_NW>(mx, red);
    mn = -block_max<LO_NW>(-mn, red);
    const bool flat = mx == mn;                                       // all draws equal: the weights stay equal
    // ---- 2, 3: shifted log ratios, cutoff
    double cutoff = 0.0, ecut = 1.0;
    if (!flat) {
        __syncthreads();
        for (int s = tid; s < S; s += LO_NT) col[s] = mn - col[s];
        cutoff = fmax(lo_radix_select(col, S, a.M[c] + 1, hist, si), a.log_dbl_min);
        ecut = exp(cutoff);
    }
    // ---- 4: tail indices, body sums, equal-weight sums
    __syncthreads();
    if (tid == 0) si[2] = 0;
    __syncthreads();
    double body[LP_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, eq[LP_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int base = 0; base < S; base += LO_NT) {
        const int s = base + tid;
        const bool in = s < S;
        const double x = (in && !flat) ? col[s] : 0.0;
        const bool up = in && !flat && x > cutoff;
        if (in) {
            double d0, q0, p0, d1 = 0.0, q1 = 0.0, p1 = 0.0;
            predict_terms(mu0[s], sg0[s], z0, d0, q0, p0);
            if (a.pair) predict_terms(mu1[s], sg1[s], z1, d1, q1, p1);
            eq[1] += d0; eq[2] += q0; eq[3] += p0;
            eq[4] += d1; eq[5] += q1; eq[6] += p1;
            if (!up && !flat) {
                const double wt = exp(x - cutoff);
                body[0] += wt;
                body[1] += wt * d0; body[2] += wt * q0; body[3] += wt * p0;
                body[4] += wt * d1; body[5] += wt * q1; body[6] += wt * p1;
            }
        }
        const unsigned long long um = __ballot(up);
        if (um) {
            const int first = __ffsll((long long)um) - 1;
            int pos = 0;
            if (lane == first) pos = atomicAdd(&si[2], __popcll(um));
            pos = __shfl(pos, first, 64) + __popcll(um & ((1ull << lane) - 1ull));
            if (up && pos < a.cap) idx[pos] = s;
        }
    }
    block_sums<LP_NSUM>(eq, red);
    const double dS = (double)S;
    const bool second = tid == 1;                                     // thread h writes scalar h of the unit
    const size_t eh = second ? e1 : e0;
    const double zh = second ? z1 : z0;
    if (tid < nh) {
        const double m1 = (second ? eq[4] : eq[1]) / dS, m2 = (second ? eq[5] : eq[2]) / dS, p = (second ? eq[6] : eq[3]) / dS;
        predict_write(a.out + 3 * plane, plane, eh, zh, m1, m2, p);
        if (flat) predict_write(a.out, plane, eh, zh, m1, m2, p);
    }
    if (flat) {
        if (tid == 0) { a.khat[c] = INFINITY; a.ntail[c] = 0; }
        return;
    }
    block_sums<LP_NSUM>(body, red);                                   // (its barriers also publish idx[] and si[2])
    const int n = min(si[2], a.cap);
    // ---- 5: the tail's values to the head of the column, through registers; sort by (value, draw index)
    double *tail = col, *y = col + a.cap, *sm = col + 2 * a.cap;      // 3 cap <= S for S >= 6; else n <= 4: y, sm not used
    {
        double stage[LP_STAGE];
#pragma unroll
        for (int k = 0; k < LP_STAGE; ++k) {
            const int r = tid + k * LO_NT;
            stage[k] = r < n ? col[idx[r]] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LP_STAGE; ++k) {
            const int r = tid + k * LO_NT;
            if (r < n) tail[r] = stage[k];
        }
    }
    bitonic_any<LO_NT>(n, [&](int i, int q) {
        const double u = tail[i], v = tail[q];
        const int iu = idx[i], iv = idx[q];
        if (u > v || (u == v && iu > iv)) { tail[i] = v; tail[q] = u; idx[i] = iv; idx[q] = iu; }
    });
    // ---- 6: generalised-Pareto fit to y = exp(tail) - exp(cutoff)
    double khat = INFINITY, sigma = NAN;
    if (n > 4) lo_pareto_fit(tail, y, n, ecut, bj, kj, Lj, wj, sc, red, khat, sigma);
    // ---- 7: smoothed tail, the tail sums, results
    const bool smooth = n > 4 && isfinite(khat);
    double mt = -INFINITY;
    for (int r = tid; r < n; r += LO_NT) {
        double v = tail[r];
        if (smooth) {
            v = lo_smoothed(r, n, khat, sigma, ecut);
            sm[r] = v;
        }
        mt = fmax(mt, v);
    }
    mt = block_max<LO_NW>(mt, red);
    double tl[LP_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = tid; r < n; r += LO_NT) {
        const int s = idx[r];
        const double wt = exp((smooth ? sm[r] : tail[r]) - mt);
        double d0, q0, p0, d1 = 0.0, q1 = 0.0, p1 = 0.0;
        predict_terms(mu0[s], sg0[s], z0, d0, q0, p0);
        if (a.pair) predict_terms(mu1[s], sg1[s], z1, d1, q1, p1);
        tl[0] += wt;
        tl[1] += wt * d0; tl[2] += wt * q0; tl[3] += wt * p0;
        tl[4] += wt * d1; tl[5] += wt * q1; tl[6] += wt * p1;
    }
    block_sums<LP_NSUM>(tl, red);
    if (tid < nh) {
        // body weights are exp(x - cutoff), tail weights exp(v - mt): both on the larger scale (n = 0: mt = -inf, st = 0)
        const double md = fmax(cutoff, mt), sb = exp(cutoff - md), st = n ? exp(mt - md) : 0.0;
        const double den = body[0] * sb + tl[0] * st;
        const double b1 = second ? body[4] : body[1], b2 = second ? body[5] : body[2], b3 = second ? body[6] : body[3];
        const double t1 = second ? tl[4] : tl[1], t2 = second ? tl[5] : tl[2], t3 = second ? tl[6] : tl[3];
        predict_write(a.out, plane, eh, zh, (b1 * sb + t1 * st) / den, (b2 * sb + t2 * st) / den, (b3 * sb + t3 * st) / den);
    }
    if (tid == 0) { a.khat[c] = khat; a.ntail[c] = n; }
}

static size_t predict_lds_bytes(int S, int cap)
{
    return ((size_t)S + LP_RED + 4 * LO_MAX_M + 4) * sizeof(double) + (256 + 4 + (size_t)cap) * sizeof(int);
}
static_assert(((size_t)LO_MAX_S + LP_RED + 4 * LO_MAX_M + 4) * 8 + (256 + 4 + (LO_MAX_S + 4) / 5) * 4 <= 160 * 1024,
              "predict_kernel: the column and the tail indices of LO_MAX_S draws must fit the LDS of a CU");

int loo_predict_device(const double *dTm, const double *dTs, const double *dz, const int *dM, int G, int S, int N2, int pair,
                       double *dOut, int *dNtail, hipStream_t stream)
{
    const int U = pair ? N2 / 2 : N2, cap = (S + 4) / 5;
    const size_t units = (size_t)G * U, nsc = (size_t)G * N2, lds = predict_lds_bytes(S, cap);
    static LdsAttrCache cache;
    BDRT_HIP(cache.ensure(lds, [&]() {
        return hipFuncSetAttribute((const void *)predict_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }));
    PredictArgs a;
    a.Tm = dTm; a.Ts = dTs; a.z = dz; a.M = dM;
    a.S = S; a.cap = cap; a.N2 = N2; a.U = U; a.pair = pair;
    a.c0 = -0.5 * std::log(2.0 * M_PI); a.log_dbl_min = std::log(DBL_MIN);
    a.out = dOut; a.khat = dOut + 6 * nsc; a.ntail = dNtail;
    hipLaunchKernelGGL(predict_kernel, dim3((unsigned)units), dim3(LO_NT), lds, stream, a);
    BDRT_HIP(hipGetLastError());
    return 0;
}

int loo_predict_of_draws(const LooDraws &j, double *mean, double *sd, double *pit, double *mean_post, double *sd_post,
                         double *pit_post, double *pareto_k, int *n_tail, double *reff_out)
{
    const char *who = "bdrt_sampler_loo_predict";
    const int S = j.chains * j.n_draws, U = j.pair ? j.ncols / 2 : j.ncols;
    const size_t N2 = 2 * (size_t)j.prob->dev.nf;
    std::vector<double> reff((size_t)j.G * U);
    LooStage st;
    DevBuf<double> Tm, Ts;
    if (const int rc = st.alloc(j, true, 6 * (size_t)j.ncols + U)) return rc;
    BDRT_HIP(Tm.alloc((size_t)st.gmax * S * j.ncols));
    BDRT_HIP(Ts.alloc((size_t)st.gmax * S * j.ncols));
    for (int g0 = 0; g0 < j.G; g0 += st.gmax) {
        const int gn = std::min(st.gmax, j.G - g0);
        const size_t units = (size_t)gn * U, nsc = (size_t)gn * j.ncols, o = (size_t)g0 * U, osc = (size_t)g0 * j.ncols;
        if (nsc > 0x7fffffffull) { set_error("%s: too many observations", who); return -2; }
        int rc;
        if ((rc = st.eval(j, g0, gn)) || (j.reff_mode == 2 && (rc = st.loglik_T(who, j, gn))) ||
            (rc = st.tails(who, j, g0, gn, reff.data() + o)) ||
            (rc = loo_transpose_device(who, st.zh.p + j.col0, Tm, gn, S, j.ncols, N2, j.stream)) ||
            (rc = loo_transpose_device(who, st.sg.p + j.col0, Ts, gn, S, j.ncols, N2, j.stream)) ||
            (rc = loo_predict_device(Tm, Ts, st.z, st.M, gn, S, j.ncols, j.pair, st.out, st.ntail, j.stream)))
            return rc;
        BDRT_HIP(hipStreamSynchronize(j.stream));
        double *const outs[6] = {mean + osc, sd + osc, pit + osc, mean_post + osc, sd_post + osc, pit_post + osc};
        if (download_planes(st.out, nsc, outs, 6)) return -10;
        BDRT_HIP(hipMemcpy(pareto_k + o, st.out.p + 6 * nsc, units * sizeof(double), hipMemcpyDeviceToHost));
        BDRT_HIP(hipMemcpy(n_tail + o, st.ntail, units * sizeof(int), hipMemcpyDeviceToHost));
    }
    if (reff_out) std::copy(reff.begin(), reff.end(), reff_out);
    return 0;
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_psis_predict_max_draws(void) { return LO_MAX_S; }

int bdrt_psis_predict(const double *Zhat, const double *sig, const double *z, int G, int S, int N2, int pair, const double *reff,
                      double *mean, double *sd, double *pit, double *mean_post, double *sd_post, double *pit_post,
                      double *pareto_k, int *n_tail)
{
    if (!Zhat || !sig || !z || !mean || !sd || !pit || !mean_post || !sd_post || !pit_post || !pareto_k || !n_tail || G < 1 ||
        S < 2 || N2 < 1 || (pair != 0 && pair != 1) || (pair && (N2 & 1))) {
        set_error("bdrt_psis_predict: bad arguments");
        return -1;
    }
    if (S > LO_MAX_S) { set_error("bdrt_psis_predict: %d draws per unit, the kernel holds at most %d", S, LO_MAX_S); return -2; }
    const int U = pair ? N2 / 2 : N2;
    const size_t units = (size_t)G * U, nsc = (size_t)G * N2, nel = nsc * S;
    if (nsc > 0x7fffffffull) { set_error("bdrt_psis_predict: too many observations"); return -2; }
    std::vector<int> M;
    if (loo_tail_lengths("bdrt_psis_predict", S, units, reff, M)) return -1;
    bind_process_device();
    DevBuf<double> dIn, dTm, dTs, dz, dOut;
    DevBuf<int> dM, dNtail;
    if (upload(dz, z, nsc) || upload(dM, M.data(), units)) return -10;
    BDRT_HIP(dTm.alloc(nel));
    BDRT_HIP(dTs.alloc(nel));
    BDRT_HIP(dIn.alloc(nel));
    BDRT_HIP(hipMemcpy(dIn, Zhat, nel * sizeof(double), hipMemcpyHostToDevice));
    if (const int rc = loo_transpose_device("bdrt_psis_predict", dIn, dTm, G, S, N2, (size_t)N2, nullptr)) return rc;
    BDRT_HIP(hipMemcpy(dIn, sig, nel * sizeof(double), hipMemcpyHostToDevice));      // (stream order: behind the first transpose)
    if (const int rc = loo_transpose_device("bdrt_psis_predict", dIn, dTs, G, S, N2, (size_t)N2, nullptr)) return rc;
    BDRT_HIP(dOut.alloc(6 * nsc + units));
    BDRT_HIP(dNtail.alloc(units));
    if (const int rc = loo_predict_device(dTm, dTs, dz, dM, G, S, N2, pair, dOut, dNtail, nullptr)) return rc;
    BDRT_HIP(hipDeviceSynchronize());
    double *const outs[6] = {mean, sd, pit, mean_post, sd_post, pit_post};
    if (download_planes(dOut, nsc, outs, 6)) return -10;
    BDRT_HIP(hipMemcpy(pareto_k, dOut + 6 * nsc, units * sizeof(double), hipMemcpyDeviceToHost));
    BDRT_HIP(hipMemcpy(n_tail, dNtail, units * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
