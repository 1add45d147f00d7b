// bdrt_model_terms.h -- the pointwise terms of the model's log-posterior, stated once for the one-chain evaluators:
// solo_eval (bdrt_solo.h), wide1_eval (bdrt_solo_wide.h), wave_eval and wave_eval_nb (bdrt_wave.h).
//
// Model code: the reference's Series / Parallel / Series-Parallel / Series-2Parallel Stan programs (+- pos, +- outliers), in the
// lean arithmetic of the sampler (lean_exp / lean_rcp / lean_log, no division).  The 16-chain tiles (bdrt_tile_s1.h, bdrt_tile_hw.h,
// logp_grad_tile) and the streamed evaluator (bdrt_big.h) state the same model in their own loops.
//
// Everything here takes and returns VALUES: the loads, stores, reductions and the thread mapping stay with the caller.  The units
// that include this are built with -ffp-contract=fast, which picks the product it fuses into a sum of two products by context;
// where that choice is open, the expression is written with an explicit fma() (the fusion the evaluators had before they shared
// this text), so that a term gives the same bits in every evaluator and instantiation.
#pragma once
#include "bdrt_device.h"

namespace bdrt {

// ---- scalar parameters: Rinf_raw, induc_raw, sigma_res_raw, alpha_prop/re/im_raw (index 0..5), then the d's ---------------------------
// priors: std_normal on the six raws, inv_gamma(5, 5) on the d's (st = log of the strength); the caller adds jac * st, the log-Jacobian of
// the lower = 0 transform.  (Two functions and the choice between them at the call site: one function with the choice inside is
// simplified on its own before it is inlined, and solo_eval's kernels then spill more.)
__device__ __forceinline__ double raw_prior_lp(double sraw) { return -0.5 * sraw * sraw; }
__device__ __forceinline__ double strength_prior_lp(double sraw, double st) { return -6.0 * st - 5.0 * lean_rcp(sraw); }
// d lp / d theta of global scalar sidx (< 6); t: its sum over the rows (lik_sums, slot sidx)
__device__ __forceinline__ double scalar_grad(const DevProblem &P, int sidx, double sraw, double t, double jac)
{
    double dl;
    if (sidx == 0) dl = 100.0 * t;
    else if (sidx == 1) dl = P.induc_scale * t;
    else dl = 0.05 * 2.0 * (0.05 * sraw) * t;
    return sraw * (dl - sraw) + jac;
}
// d lp / d theta of a penalty strength d_i; sv: sum over k of v_i[k]^2 / ups[k]^2
__device__ __forceinline__ double strength_grad(double sraw, double sv, double jac)
{
    return -0.5 * sraw * sv - 6.0 + 5.0 * lean_rcp(sraw) + jac;
}

// ---- likelihood -----------------------------------------------------------------------------------------------------------------------
struct LikConsts { double Rinf, induc, c0, ap2, ar2, ai2; };
struct LikPoint { double lp, gzr, gzi, h_re, h_im; };
struct LikSums { double R, L, H, Hz2, Hzr2, Hzi2; };

// once per evaluation, from the six constrained global scalars
__device__ __forceinline__ LikConsts lik_consts(const DevProblem &P, double r_Rinf, double r_induc, double r_res, double r_prop,
                                                double r_re, double r_im)
{
    LikConsts c;
    c.Rinf = 100.0 * r_Rinf; c.induc = r_induc * P.induc_scale;
    const double s_res = 0.05 * r_res, a_p = 0.05 * r_prop, a_r = 0.05 * r_re, a_i = 0.05 * r_im;
    c.c0 = fma(s_res, s_res, P.sigma_min * P.sigma_min);
    c.ap2 = a_p * a_p; c.ar2 = a_r * a_r; c.ai2 = a_i * a_i;
    return c;
}
// one frequency: Z_hat = (zr, zi) with Rinf and the inductance in it, measured (zre, zim).  OM: sigma_out enters the variances
// (without it nothing is added: x + 0.0 does not fold)
template <bool OM>
__device__ __forceinline__ LikPoint lik_point(const LikConsts &c, double zr, double zi, double zre, double zim, double so_re = 0.0,
                                              double so_im = 0.0)
{
    LikPoint p;
    const double common = c.ar2 * zr * zr + c.ai2 * zi * zi;
    double s2_re = c.c0 + c.ap2 * zr * zr + common, s2_im = c.c0 + c.ap2 * zi * zi + common;
    if constexpr (OM) { s2_re += so_re * so_re; s2_im += so_im * so_im; }
    const double e_re = zre - zr, e_im = zim - zi;
    const double prod = s2_re * s2_im, ip = lean_rcp(prod);
    const double w_re = s2_im * ip, w_im = s2_re * ip;
    p.lp = -0.5 * lean_log(prod) - 0.5 * e_re * e_re * w_re - 0.5 * e_im * e_im * w_im;
    p.h_re = -0.5 * w_re + 0.5 * e_re * e_re * w_re * w_re;
    p.h_im = -0.5 * w_im + 0.5 * e_im * e_im * w_im * w_im;
    p.gzr = e_re * w_re + 2.0 * zr * (p.h_re * (c.ap2 + c.ar2) + p.h_im * c.ar2);
    p.gzi = e_im * w_im + 2.0 * zi * (p.h_im * (c.ap2 + c.ai2) + p.h_re * c.ai2);
    return p;
}
// the row's terms of the six sums behind the gradients of the global scalars (slot order of scalar_grad)
__device__ __forceinline__ LikSums lik_sums(const LikPoint &p, double zr, double zi, double wn)
{
    LikSums s;
    s.R = p.gzr; s.L = p.gzi * wn; s.H = p.h_re + p.h_im; s.Hz2 = p.h_re * zr * zr + p.h_im * zi * zi;
    s.Hzr2 = (p.h_re + p.h_im) * zr * zr; s.Hzi2 = (p.h_re + p.h_im) * zi * zi;
    return s;
}

// ---- outlier error model: two parameters per row, r = exp(t); mode 1 the Stan files' form (sigma_out = raw x scale), mode 2 one per part
struct OutlierSigma { double re, im; };
struct OutlierTerms { double g0, g1, lp; };

__device__ __forceinline__ OutlierSigma outlier_sigma(int mode, double r0, double r1)
{
    OutlierSigma s;
    if (mode == 1) s.re = s.im = 0.05 * r0 * r1;
    else { s.re = 0.05 * r0; s.im = 0.05 * r1; }
    return s;
}
// gradients of the row's two parameters and its share of lp
__device__ __forceinline__ OutlierTerms outlier_terms(const DevProblem &P, int mode, double jac, double t0, double t1, double r0, double r1,
                                                      const OutlierSigma &so, const LikPoint &p)
{
    OutlierTerms o;
    if (mode == 1) {
        const double dso = 2.0 * so.re * (p.h_re + p.h_im), ir1 = lean_rcp(r1);
        o.g0 = r0 * (0.05 * r1 * dso - P.so_lambda) + jac;
        o.g1 = 0.05 * r0 * r1 * dso - (P.so_alpha + 1.0) + P.so_beta * ir1 + jac;
        o.lp = -P.so_lambda * r0 - (P.so_alpha + 1.0) * t1 - P.so_beta * ir1 + jac * (t0 + t1);
    } else {
        o.g0 = r0 * (0.05 * 2.0 * so.re * p.h_re - P.so_lambda) + jac;
        o.g1 = r1 * (0.05 * 2.0 * so.im * p.h_im - P.so_lambda) + jac;
        o.lp = -P.so_lambda * (r0 + r1) + jac * (t0 + t1);
    }
    return o;
}

// ---- parallel (admittance) block: Z_hat_p = conj(Y) / |Y|^2 (Parallel_modelcode.txt:47) ------------------------------------------------
__device__ __forceinline__ void parallel_fwd(double yr, double yi, double &zr, double &zi)
{
    const double idn = lean_rcp(yr * yr + yi * yi);
    zr += yr * idn;
    zi += -yi * idn;
}
// (rr, ri) = g_Zhat -> J^T g_Zhat, the operand of A^T (the block's scale is the caller's)
__device__ __forceinline__ void parallel_bwd(double yr, double yi, double &rr, double &ri)
{
    const double dn = yr * yr + yi * yi, id2 = lean_rcp(dn * dn);
    const double dd = (yi * yi - yr * yr) * id2, doff = 2.0 * yr * yi * id2;
    const double gr_ = rr, gi_ = ri;
    rr = gr_ * dd + gi_ * doff;
    ri = -gr_ * doff + gi_ * dd;
}

// ---- ups prior at basis function k -------------------------------------------------------------------------------------------------------
// v_i = (L_i x)[k], d_i the penalty strengths, tu = theta_ups[k], uu = ups[k] = 0.15 exp(tu), um2 .. up2 = ups[k - 2 .. k + 2]
struct UpsPrior { double gup, w0, w1, w2, sv0, sv1, sv2; };

// the 512-thread evaluators (solo_eval, wide1_eval): adds the thread's share to lp, term by term in the order they always had.
// (wave_eval and wave_eval_nb state these terms with every neighbour accumulation as an explicit fma, in their own loops.)
__device__ __forceinline__ UpsPrior ups_prior_k(const DevProblem &P, double jac, double v0, double v1, double v2, double d0, double d1,
                                                double d2, double tu, double uu, double um2, double um1, double up1, double up2, int k, int K,
                                                double &lp)
{
    UpsPrior r;
    const double iu = lean_rcp(uu), iu2 = iu * iu;
    const double q2 = d0 * v0 * v0 + d1 * v1 * v1 + d2 * v2 * v2;
    const double ir = 0.15 * iu;                           // 1 / ups_raw
    lp += -(tu + LOG_015) - 0.5 * q2 * iu2 - (P.ups_alpha + 1.0) * tu - P.ups_beta * ir + jac * tu;
    r.sv0 = v0 * v0 * iu2; r.sv1 = v1 * v1 * iu2; r.sv2 = v2 * v2 * iu2;
    double gu = -iu + q2 * iu2 * iu;
    if (k >= 1 && k + 1 < K) {                             // dups centred at k
        const double du = 0.5 * (uu - 0.5 * (um1 + up1)) * iu;
        lp += -0.5 * du * du;
        gu += -du * 0.25 * (um1 + up1) * iu2;
    }
    if (k >= 2) {                                          // k is the right neighbour of centre k-1
        const double i0 = lean_rcp(um1);
        const double du = 0.5 * (um1 - 0.5 * (um2 + uu)) * i0;
        gu += du * 0.25 * i0;
    }
    if (k + 2 < K) {                                       // k is the left neighbour of centre k+1
        const double i0 = lean_rcp(up1);
        const double du = 0.5 * (up1 - 0.5 * (uu + up2)) * i0;
        gu += du * 0.25 * i0;
    }
    r.gup = uu * gu - (P.ups_alpha + 1.0) + P.ups_beta * ir + jac;
    r.w0 = -d0 * v0 * iu2; r.w1 = -d1 * v1 * iu2; r.w2 = -d2 * v2 * iu2;
    return r;
}

}  // namespace bdrt
