// bdrt_heldout_mix.hip -- prediction at held-out frequencies under the outlier error models (include/bdrt.h section (4c)).
//
// A held-out point has no sigma_out of its own, but the prior of sigma_out is fixed by data, not by parameters, so what a draw
// says about a new observation is its normal with sigma_out integrated over that prior: a scale mixture of normals, the same for
// every draw and every point.  The integral is a fixed table of Q nodes y_j and weights w_j that the host builds once per
// problem (loo.sigma_out_prior_table).  Definitions: tests/heldout_mix_numpy.py (the yardstick); DESIGN.md 3.5h.
//
//   heldout_kernel (bdrt_heldout.hip) gives mu = Z_hat and the base scale s_b = sigma_tot without sigma_out; only its wrappers
//                          refuse the outlier models, and the entries here pass allow_outliers.
//   heldout_mix_reduce_kernel  one workgroup per (group, unit), on the transposed Z_hat and base sigma [G][N2][S], the table in
//                          LDS as (y_j^2, w_j) pairs.  Per draw s and scalar c, with e = z - mu, v_j = s_b^2 + y_j^2:
//                              m_s   = sum_j w_j N(z | mu, v_j)      (pair, shared y: the product of the two normals under one sum;
//                                                                     pair, independent y: the product of two sums)
//                              Phi_s = sum_j w_j Phi(e / sqrt(v_j))
//                          m_s is kept as its logarithm: every exponent is taken relative to the one at the largest node, which
//                          bounds them all, so the sum over j holds a term equal to w_j / sqrt(v_j) and cannot underflow whatever
//                          the residual.  Then lpd = logsumexp_s(log m_s) - log S as heldout_reduce_kernel sums it, mean and sd
//                          from predict_terms' sums with E[y^2] added to the second moment, pit = mean_s Phi_s.
//                          Work split: P = 2^lp adjacent lanes share one draw and stride over the nodes (P: the largest power of
//                          two <= 64 with P S <= LO_NT and P <= Q; P = 1 from 257 draws on), an xor butterfly over the P lanes
//                          closes the sum over j.  The sums over draws always run in heldout_reduce_kernel's order -- thread t
//                          takes draws t, t + LO_NT, ... (for P > 1 through 2 S doubles of LDS), then block_sums -- so with the
//                          table (y = 0, w = 1) every sum has heldout_reduce_kernel's bits.  A unit's result depends on its own
//                          rows, S, Q and the table only: the same bits alone or in any batch.  The table reads are broadcasts
//                          (all lanes of a draw group at P = 1 read one address); whether the loop is bound by the transcendental
//                          sequences (sqrt, two divisions, exp, erfc per node and scalar) or by LDS has not been measured.
// bdrt_sampler_heldout_mix (bdrt_sampler.hip) runs both on a sampler's draws in chunks of groups (heldout_mix_of_draws), as
// heldout_of_draws does.
#include <cfloat>
#include <cmath>

#include "bdrt_host.h"
#include "bdrt_psis.h"

namespace bdrt {

constexpr int HM_MAX_Q = 512;
constexpr size_t HM_LDS_MAX = 160 * 1024;

struct HeldoutMixArgs {
    const double *Tm, *Ts;                       // [G][N2][S] device: Z_hat and the base sigma, transposed
    const double *z;                             // [G][N2] device
    const double *tab;                           // [Q][2] device: y_j^2, w_j
    int S, N2, U, pair, joint, Q, lp;            // joint: a pair unit whose two scalars share y; 2^lp lanes per draw
    double c0, log_S, ey2, y2max;
    double *out;                                 // 3 planes [G][N2]: mean, sd, pit
    double *lpd;                                 // [G][U]
};

// the sum of v over the 2^lp adjacent lanes of a draw; the same value in each of them
__device__ inline double hm_group_sum(double v, int lp)
{
    for (int o = (1 << lp) >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(LO_NT) void heldout_mix_reduce_kernel(HeldoutMixArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int S = a.S, Q = a.Q, nh = a.pair + 1, lp = a.lp, P = 1 << lp;
    const size_t c = blockIdx.x, g = c / a.U;
    const int u = (int)(c - g * a.U);
    double *tab = lds;                                                // [Q][2]
    double *col = tab + 2 * Q;                                        // [S] log m_s
    double *red = col + S;                                            // [LP_RED]
    double *pp = red + LP_RED;                                        // [2][S] Phi_s of the two scalars (P > 1 only)
    const size_t plane = (size_t)gridDim.x / a.U * a.N2;              // G N2
    const size_t e0 = g * a.N2 + u, e1 = e0 + a.U;                    // the unit's scalars (e1: pairs only)
    const double *mu0 = a.Tm + e0 * S, *sg0 = a.Ts + e0 * S;
    const double *mu1 = a.Tm + e1 * S, *sg1 = a.Ts + e1 * S;
    const double z0 = a.z[e0], z1 = a.pair ? a.z[e1] : 0.0;
    for (int i = tid; i < 2 * Q; i += LO_NT) tab[i] = a.tab[i];
    __syncthreads();

    // ---- per draw: the sums over the table
    const int jp = tid & (P - 1), slot = tid >> lp, nslot = LO_NT >> lp;
    int bad = 0;
    double eq[LP_NSUM - 1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int sb = 0; sb < S; sb += nslot) {
        const bool act = sb + slot < S;
        const int s = act ? sb + slot : S - 1;                        // (idle lanes repeat the last draw: the butterfly is whole)
        const double m0 = mu0[s], b0 = sg0[s], m1 = a.pair ? mu1[s] : 0.0, b1 = a.pair ? sg1[s] : 1.0;
        const double r0 = z0 - m0, d0 = m0 - z0, r1 = z1 - m1, d1 = m1 - z1;
        const double v0 = b0 * b0, v1 = b1 * b1;
        const double qt0 = r0 / sqrt(v0 + a.y2max), qt1 = r1 / sqrt(v1 + a.y2max);
        const double ct0 = -0.5 * (qt0 * qt0), ct1 = -0.5 * (qt1 * qt1);      // the largest exponents
        double a0 = 0.0, a1 = 0.0, p0 = 0.0, p1 = 0.0;
        for (int j = jp; j < Q; j += P) {
            const double y2 = tab[2 * j], w = tab[2 * j + 1];
            const double s0 = sqrt(v0 + y2);
            const double q0 = r0 / s0, i0 = 1.0 / s0;
            const double x0 = -0.5 * (q0 * q0);
            p0 += w * (0.5 * erfc(d0 / (s0 * M_SQRT2)));
            if (a.pair) {
                const double s1 = sqrt(v1 + y2);
                const double q1 = r1 / s1, i1 = 1.0 / s1;
                const double x1 = -0.5 * (q1 * q1);
                p1 += w * (0.5 * erfc(d1 / (s1 * M_SQRT2)));
                if (a.joint) {
                    a0 += w * ((i0 * i1) * exp((x0 + x1) - (ct0 + ct1)));
                } else {
                    a0 += w * (i0 * exp(x0 - ct0));
                    a1 += w * (i1 * exp(x1 - ct1));
                }
            } else {
                a0 += w * (i0 * exp(x0 - ct0));
            }
        }
        a0 = hm_group_sum(a0, lp);
        a1 = hm_group_sum(a1, lp);
        p0 = hm_group_sum(p0, lp);
        p1 = hm_group_sum(p1, lp);
        double v;
        if (a.joint) v = ((a.c0 + a.c0) + log(a0)) + (ct0 + ct1);
        else {
            v = (a.c0 + log(a0)) + ct0;
            if (a.pair) v = v + ((a.c0 + log(a1)) + ct1);
        }
        if (!(b0 > 0.0) || !isfinite(b0) || !(b1 > 0.0) || !isfinite(b1)) v = NAN;
        if (act && jp == 0) {
            bad |= !isfinite(v);
            col[s] = v;
            if (P > 1) { pp[s] = p0; pp[S + s] = p1; }
            else { eq[2] += p0; eq[5] += p1; }
        }
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid < 3 * nh) a.out[(size_t)(tid / nh) * plane + ((tid % nh) ? e1 : e0)] = NAN;
        if (tid == 0) a.lpd[c] = NAN;
        return;
    }
    // ---- the sums over draws, in heldout_reduce_kernel's order
    double mx = -INFINITY, mn = INFINITY;
    for (int s = tid; s < S; s += LO_NT) {
        const double v = col[s];
        mx = fmax(mx, v);
        mn = fmin(mn, v);
        double d0, q0, f0, d1 = 0.0, q1 = 0.0, f1 = 0.0;
        predict_terms(mu0[s], sg0[s], z0, d0, q0, f0);
        if (a.pair) predict_terms(mu1[s], sg1[s], z1, d1, q1, f1);
        eq[0] += d0; eq[1] += q0;
        eq[3] += d1; eq[4] += q1;
        if (P > 1) { eq[2] += pp[s]; eq[5] += pp[S + s]; }
    }
    mx = block_max<LO_NW>(mx, red);
    mn = -block_max<LO_NW>(-mn, red);
    block_sums<LP_NSUM - 1>(eq, red);
    const double dS = (double)S;
    const bool second = tid == 1;                                     // thread h writes scalar h of the unit
    if (tid < nh) {
        const double m1 = (second ? eq[3] : eq[0]) / dS, m2 = (second ? eq[4] : eq[1]) / dS, p = (second ? eq[5] : eq[2]) / dS;
        predict_write(a.out, plane, second ? e1 : e0, second ? z1 : z0, m1, m2 + a.ey2, p);
    }
    // ---- lpd = logsumexp(log m) - log S (heldout_reduce_kernel)
    if (mx == mn) {
        if (tid == 0) a.lpd[c] = mx;
        return;
    }
    double se = 0.0;
    for (int s = tid; s < S; s += LO_NT) se += exp(col[s] - mx);
    se = block_sum<LO_NW>(se, red);
    if (tid == 0) a.lpd[c] = (mx + log(se)) - a.log_S;
}

// ---- the table: checks, (y^2, w) pairs to the device, the largest y^2
struct MixTable {
    DevBuf<double> d;
    int Q = 0, shared = 0;
    double ey2 = 0.0, y2max = 0.0;
};

static int mix_table(const char *who, const double *y, const double *w, int Q, int shared, double ey2, MixTable &t)
{
    if (!y || !w || Q < 1 || (shared != 0 && shared != 1)) { set_error("%s: bad arguments", who); return -1; }
    if (Q > HM_MAX_Q) { set_error("%s: a table of %d nodes, the kernel holds at most %d", who, Q, HM_MAX_Q); return -2; }
    if (!(ey2 >= 0.0)) { set_error("%s: E[y^2] = %g is not a non-negative number", who, ey2); return -1; }
    std::vector<double> h(2 * (size_t)Q);
    t.y2max = 0.0;
    for (int j = 0; j < Q; ++j) {
        if (!std::isfinite(y[j]) || y[j] < 0.0 || !std::isfinite(w[j]) || w[j] < 0.0) {
            set_error("%s: node %d (y = %g, w = %g) is not a pair of non-negative numbers", who, j, y[j], w[j]);
            return -1;
        }
        h[2 * j] = y[j] * y[j];
        h[2 * j + 1] = w[j];
        t.y2max = std::max(t.y2max, h[2 * j]);
    }
    if (!std::isfinite(t.y2max)) { set_error("%s: the largest node overflows when squared", who); return -1; }
    if (upload(t.d, h.data(), h.size())) return -10;
    t.Q = Q; t.shared = shared; t.ey2 = ey2;
    return 0;
}

// lanes per draw (log2): the largest power of two <= 64 with P S <= LO_NT and P <= Q
static int mix_lanes_log2(int S, int Q)
{
    int lp = 0;
    while (lp < 6 && (2 << lp) * (long)S <= LO_NT && (2 << lp) <= Q) ++lp;
    return lp;
}

static size_t mix_lds_bytes(int S, int Q)
{
    return ((size_t)S + 2 * (size_t)Q + LP_RED + (mix_lanes_log2(S, Q) ? 2 * (size_t)S : 0)) * sizeof(double);
}

// dTm, dTs [G][N2][S], dz [G][N2] -> dOut: 3 planes of G N2 (mean, sd, pit), then lpd [G U]; enqueues on `stream` and returns
static int heldout_mix_reduce_device(const char *who, const double *dTm, const double *dTs, const double *dz, int G, int S, int N2,
                                     int pair, const MixTable &t, double *dOut, hipStream_t stream)
{
    const int U = pair ? N2 / 2 : N2;
    const size_t units = (size_t)G * U, nsc = (size_t)G * N2, lds = mix_lds_bytes(S, t.Q);
    if (lds > HM_LDS_MAX) {
        set_error("%s: %d draws and %d nodes need %zu bytes of LDS, a CU has %zu", who, S, t.Q, lds, HM_LDS_MAX);
        return -2;
    }
    if (units > 0x7fffffffull) { set_error("%s: too many units", who); return -2; }
    static LdsAttrCache cache;
    BDRT_HIP(cache.ensure(lds, [&]() {
        return hipFuncSetAttribute((const void *)heldout_mix_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }));
    HeldoutMixArgs a;
    a.Tm = dTm; a.Ts = dTs; a.z = dz; a.tab = t.d; a.S = S; a.N2 = N2; a.U = U; a.pair = pair; a.joint = pair && t.shared;
    a.Q = t.Q; a.lp = mix_lanes_log2(S, t.Q);
    a.c0 = -0.5 * std::log(2.0 * M_PI); a.log_S = std::log((double)S); a.ey2 = t.ey2; a.y2max = t.y2max;
    a.out = dOut; a.lpd = dOut + 3 * nsc;
    hipLaunchKernelGGL(heldout_mix_reduce_kernel, dim3((unsigned)units), dim3(LO_NT), lds, stream, a);
    BDRT_HIP(hipGetLastError());
    return 0;
}

// heldout_of_draws with the mixture reduce (heldout_of_draws_with): j as there; y, w [Q] and ey2: the table of sigma_out's prior; shared: one y per frequency
int heldout_mix_of_draws(const LooDraws &j, const double *freq, int H, const double *A, const double *z_test, int shared,
                         const double *y, const double *w, int Q, double ey2, double *lpd, double *mean, double *sd, double *pit)
{
    const char *who = "bdrt_sampler_heldout_mix";
    BDRT_HIP(hipSetDevice(j.prob->device));
    MixTable t;
    if (int rc = mix_table(who, y, w, Q, shared, ey2, t)) return rc;
    return heldout_of_draws_with(who, j, freq, H, A, z_test, true,
                                 [&](const double *dTm, const double *dTs, const double *dz, int gn, int S, double *dOut) {
                                     return heldout_mix_reduce_device(who, dTm, dTs, dz, gn, S, j.ncols, j.pair, t, dOut, j.stream);
                                 }, lpd, mean, sd, pit);
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_heldout_mix_max_nodes(void) { return HM_MAX_Q; }

int bdrt_heldout_mix_transformed(bdrt_problem *p, const double *params, int B, const double *freq_test, int H, const double *A_test,
                                 double *Z_hat, double *sigma_base)
{
    const char *who = "bdrt_heldout_mix_transformed";
    if (!p || !params || !freq_test || !A_test || !Z_hat || !sigma_base || B < 0 || H < 1) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    Problem &P = p->impl;
    if (!P.dev.outlier_mode) {
        set_error("%s: the problem has no outlier error model: bdrt_heldout_transformed is the entry for it", who);
        return -2;
    }
    if (heldout_check_grid(who, freq_test, H)) return -1;
    if (B == 0) return 0;
    BDRT_HIP(hipSetDevice(P.device));
    const size_t nz = (size_t)B * 2 * H;
    DevBuf<double> dW, dA, dPar, dZh, dSg;
    if (heldout_upload_grid(P, freq_test, H, A_test, dW, dA) || upload(dPar, params, (size_t)B * P.dev.D)) return -10;
    BDRT_HIP(dZh.alloc(nz));
    BDRT_HIP(dSg.alloc(nz));
    if (const int rc = heldout_transformed_device(who, P, dPar, (size_t)B, dW, dA, H, dZh, dSg, P.stream, true)) return rc;
    if (download(Z_hat, dZh.p, nz, P.stream) || download(sigma_base, dSg.p, nz, P.stream)) return -10;
    BDRT_HIP(hipStreamSynchronize(P.stream));
    return 0;
}

int bdrt_heldout_mix_reduce(const double *Zhat, const double *sig_base, const double *z, int G, int S, int N2, int pair, int shared,
                            const double *y, const double *w, int Q, double ey2, double *lpd, double *mean, double *sd, double *pit)
{
    const char *who = "bdrt_heldout_mix_reduce";
    if (!Zhat || !sig_base || !z || !lpd || !mean || !sd || !pit || G < 1 || S < 2 || N2 < 1 || (pair != 0 && pair != 1) ||
        (pair && (N2 & 1))) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    if (S > LO_MAX_S) { set_error("%s: %d draws per unit, the kernel holds at most %d", who, S, LO_MAX_S); return -2; }
    const int U = pair ? N2 / 2 : N2;
    const size_t units = (size_t)G * U, nsc = (size_t)G * N2, nel = nsc * S;
    if (nsc > 0x7fffffffull) { set_error("%s: too many observations", who); return -2; }
    bind_process_device();
    MixTable t;
    if (int rc = mix_table(who, y, w, Q, shared, ey2, t)) return rc;
    DevBuf<double> dIn, dTm, dTs, dz, dOut;
    if (upload(dz, z, nsc)) return -10;
    BDRT_HIP(dTm.alloc(nel));
    BDRT_HIP(dTs.alloc(nel));
    BDRT_HIP(dIn.alloc(nel));
    BDRT_HIP(hipMemcpy(dIn, Zhat, nel * sizeof(double), hipMemcpyHostToDevice));
    if (const int rc = loo_transpose_device(who, dIn, dTm, G, S, N2, (size_t)N2, nullptr)) return rc;
    BDRT_HIP(hipMemcpy(dIn, sig_base, nel * sizeof(double), hipMemcpyHostToDevice)); // (stream order: behind the first transpose)
    if (const int rc = loo_transpose_device(who, dIn, dTs, G, S, N2, (size_t)N2, nullptr)) return rc;
    BDRT_HIP(dOut.alloc(3 * nsc + units));
    if (const int rc = heldout_mix_reduce_device(who, dTm, dTs, dz, G, S, N2, pair, t, dOut, nullptr)) return rc;
    BDRT_HIP(hipDeviceSynchronize());
    double *const outs[3] = {mean, sd, pit};
    if (download_planes(dOut, nsc, outs, 3)) return -10;
    BDRT_HIP(hipMemcpy(lpd, dOut + 3 * nsc, units * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
