/*
 * bdrt.h -- C ABI of libbdrt.so, the MI355X (gfx950) hot path of bayes-drt.
 *
 * The reference (jdhuang-csm/bayes-drt) has no FFI: its hot path is reached from Python through three
 * internal seams of bayes_drt.inversion.Inverter:
 *   (1) construct_A / construct_L / construct_M          bayes_drt/matrices.py:120, :268, :366
 *   (2) StanModel.optimizing / StanModel.sampling        bayes_drt/inversion.py:1216, :1218-1221 (pystan 2.19.1.1)
 *   (3) cvxopt.solvers.qp via Inverter._convex_opt       bayes_drt/inversion.py:1043-1067
 * Each entry point below replaces one of those calls; the ctypes binding a maintainer would add is shown
 * in INTEGRATION.md and implemented in bayes_drt_amd/_lib.py.
 *
 * Conventions: all arrays are C-contiguous fp64 unless stated; the caller owns every buffer passed in;
 * the library copies inputs to HBM at bdrt_problem_create and owns device memory until bdrt_problem_destroy.
 * Functions return 0 on success, a negative code on error (text via bdrt_last_error()).  A non-finite or
 * rejected log-density is NOT an error: lp = -inf for that row.
 * Host-pointer entry points move data over PCIe; the *_dev entry points take device pointers (HBM-resident
 * inputs) and a hipStream_t (passed as void*).
 */
#ifndef BDRT_H
#define BDRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDRT_MAX_BLOCKS 3

/* integrand ids: bayes_drt/matrices.py:27-117 get_A_func */
enum {
    BDRT_KERNEL_DRT = 0,              /* matrices.py:45-52 */
    BDRT_KERNEL_DDT_BLOCK_PLANAR = 1, /* matrices.py:59-70 */
    BDRT_KERNEL_DDT_BLOCK_SPHER = 2,  /* matrices.py:72-80 */
    BDRT_KERNEL_DDT_TRANS_PLANAR = 3  /* matrices.py:83-92 */
};

/* basis function ids: bayes_drt/matrices.py:8-24 get_basis_func */
enum {
    BDRT_BASIS_GAUSSIAN = 0,          /* matrices.py:12-13 (the only one Inverter accepts, inversion.py:38-39) */
    BDRT_BASIS_COLE_COLE = 1,         /* matrices.py:15-17, 0 < epsilon < 1 */
    BDRT_BASIS_ZIC = 2                /* matrices.py:19-21, epsilon unused */
};

/* ---- (1) matrix construction ------------------------------------------------------------------ */

/* replaces construct_A (matrices.py:120-265).  out: [nf x k] row-major.  part 0=real 1=imag.
 * dist_series: 1 integrate Z_D, 0 integrate 1/Z_D (DDT).  toeplitz=1: first column + first row only
 * (matrices.py:213-242), returns -2 if r[0]!=c[0] (matrices.py:239-241). */
int bdrt_build_A(const double *freq, int nf, const double *tau, int k, double eps, int kernel_id, int part,
                 int dist_series, int use_ct, double k_ct, int toeplitz, double *out);
/* construct_A with another basis function (the `basis` argument of matrices.py:120); bdrt_build_A = gaussian */
int bdrt_build_A_basis(const double *freq, int nf, const double *tau, int k, double eps, int kernel_id, int part,
                       int dist_series, int use_ct, double k_ct, int toeplitz, int basis_id, double *out);
/* replaces construct_L (matrices.py:268-325) in the collocated form Inverter calls it (frequencies = 1/(2 pi tau),
 * inversion.py:2302-2307); coef4 weights derivative orders 0..3.  out: [k x k] */
int bdrt_build_L(const double *tau, int k, double eps, const double *coef4, double *out);
/* construct_L as the function is written: any `frequencies` against any `tau`, out [nf x k]; freq == NULL: collocated
 * (nf == k).  basis_id: gaussian, or Zic with order 0 only (matrices.py:316-318); Cole-Cole has no derivative there. */
int bdrt_build_L_rect(const double *freq, int nf, const double *tau, int k, double eps, const double *coef4, int basis_id,
                      double *out);
/* replaces construct_M (matrices.py:366-411); coef3 weights orders 0..2.  out: [k x k] */
int bdrt_build_M(const double *tau, int k, double eps, const double *coef3, int toeplitz, double *out);

/* ---- (2) the Stan model: data block, log-posterior + gradient, optimizing, sampling -------------- */

/* The Stan `data` block of the model families in bayes_drt/stan_model_files/ (SURVEY.md 8(a) S1-S6),
 * as assembled by Inverter._prep_stan_data (inversion.py:1684-2122), written as "blocks":
 *   Series(_pos)            1 series block                         Series_modelcode.txt
 *   Parallel                1 parallel block, use_x_sum=0          Parallel_modelcode.txt
 *   Series-Parallel(_pos)   series + 1 parallel, use_x_sum=1       Series-Parallel_modelcode.txt
 *   Series-2Parallel(_pos)  series + 2 parallel, use_x_sum=1       Series-2Parallel_modelcode.txt
 *   *_outliers              outlier_mode 1 (Series: raw[nf],scale[nf]) or 2 (stacked raw[2nf])
 * Parameter order = Stan declaration order: Rinf_raw, induc_raw, x blocks, sigma_res_raw, alpha_prop_raw,
 * alpha_re_raw, alpha_im_raw, [sigma_out_raw(, sigma_out_scale)], ups blocks, (d0,d1,d2) blocks. */
typedef struct {
    int nf;                                /* measured frequencies (Stan N/2)                          */
    int nblocks;
    int K[BDRT_MAX_BLOCKS];
    int is_parallel[BDRT_MAX_BLOCKS];
    int nonneg[BDRT_MAX_BLOCKS];           /* vector<lower=0> x (parallel blocks are always lower=0)   */
    double x_scale[BDRT_MAX_BLOCKS];       /* xp_scale                                                 */
    const double *A[BDRT_MAX_BLOCKS];      /* [2nf x K] stacked [A_re ; A_im]                          */
    const double *L0[BDRT_MAX_BLOCKS];     /* [K x K], mode-scaled as in inversion.py:1725-1737        */
    const double *L1[BDRT_MAX_BLOCKS];
    const double *L2[BDRT_MAX_BLOCKS];
    const double *freq;                    /* [nf]                                                     */
    int n_spectra;                         /* spectra sharing the grids (multi-spectrum batch)         */
    const double *Z;                       /* [n_spectra x 2nf] stacked [Z' ; Z''] per spectrum        */
    double sigma_min, ups_alpha, ups_beta, induc_scale;
    int outlier_mode;
    double so_lambda, so_alpha, so_beta;
    int use_x_sum;
    double x_sum_invscale;
} bdrt_dat;

typedef struct bdrt_problem bdrt_problem;

bdrt_problem *bdrt_problem_create(const bdrt_dat *dat);   /* NULL on error */
void bdrt_problem_destroy(bdrt_problem *p);
int bdrt_num_params(const bdrt_problem *p);               /* D: length of the unconstrained vector */
/* diagnostics: which 16-column tile evaluator bdrt_logp_grad / the sampler use for this problem.  0 dense L (MFMA), 1 banded
 * Toeplitz L (generic tile), 2 one-block fast tile with the A fragments streamed from L2, 3 general half-wave tile (several
 * blocks), 4 one-block fast tile with the A operands from an LDS-resident Toeplitz generator table (A_re, A_im exactly
 * Toeplitz -- equal log spacing of the frequencies and of tau --, nf, K >= 32; env BDRT_STREAM_A=1 at bdrt_problem_create forces 2), 5 a problem beyond the
 * LDS budget of all of these (more than 128 frequencies, ~200 basis functions per distribution ...): the streamed evaluator, one
 * workgroup per point, vectors in an HBM workspace -- slow but working, the reference takes any grid (inversion.py:2127-2209);
 * env BDRT_BIG=1 at bdrt_problem_create forces it */
int bdrt_problem_evaluator(const bdrt_problem *p);
/* is_pos[D]: 1 where the Stan parameter is declared <lower=0> (log transform) */
int bdrt_param_is_pos(const bdrt_problem *p, unsigned char *is_pos);
/* replace the measured spectra of an existing problem (same grids): Z [n_spectra x 2nf] */
int bdrt_problem_set_Z(bdrt_problem *p, const double *Z, int n_spectra);

/* log_prob + gradient on the unconstrained scale for B points (Stan's log_prob_grad, evaluated by pystan
 * inside optimizing/sampling: inversion.py:1216-1221).  theta [B x D]; spec[B] selects the spectrum of each
 * row (NULL: all 0); jacobian 1 = sampling, 0 = optimizing; lp [B]; grad [B x D]. */
int bdrt_logp_grad(bdrt_problem *p, const double *theta, const int *spec, int B, int jacobian, double *lp,
                   double *grad);
/* same with device pointers (inputs already in HBM); stream = hipStream_t */
int bdrt_logp_grad_dev(bdrt_problem *p, const double *d_theta, const int *d_spec, int B, int jacobian, double *d_lp,
                       double *d_grad, void *stream);
/* constrained parameters + transformed parameters (Stan `transformed parameters` block) for B points:
 * params [B x D] (constrained), Z_hat [B x 2nf], sigma_tot [B x 2nf]; any output may be NULL */
int bdrt_transformed(bdrt_problem *p, const double *theta, const int *spec, int B, double *params, double *Z_hat,
                     double *sigma_tot);

/* replaces StanModel.optimizing (inversion.py:1216): L-BFGS on the unconstrained scale, no Jacobian.
 * One optimisation per row of init (n_fits rows, spectrum spec[i]); every log_prob+grad is evaluated on the GPU. */
typedef struct {
    int max_iter;           /* Stan `iter` (inversion.py:1077: 50000): cap on L-BFGS iterations          */
    int history;            /* 5                                                                         */
    double init_alpha;      /* 1e-3                                                                      */
    double tol_obj;         /* 1e-12                                                                     */
    double tol_rel_obj;     /* 1e4  (x machine eps)                                                      */
    double tol_grad;        /* 1e-8                                                                      */
    double tol_rel_grad;    /* 1e7  (x machine eps)                                                      */
    double tol_param;       /* 1e-8                                                                      */
    /* second-order polish (not in Stan; bdrt_newton.h): after at most lbfgs_before_newton L-BFGS iterations a
     * damped Newton iteration with the full Hessian (2D batched gradient evaluations per step) runs until
     * |grad|_inf < newton_tol.  newton_max_iter = 0 gives the plain Stan-style L-BFGS.                   */
    int newton_max_iter;    /* 2000                                                                      */
    int lbfgs_before_newton;/* 0 (measured: L-BFGS iterations before the Newton iteration only add time)    */
    double newton_tol;      /* 1e-8                                                                      */
} bdrt_opt_options;
typedef struct {
    int iterations;         /* L-BFGS iterations                                                         */
    int n_evals;            /* log_prob+grad evaluations, all phases                                     */
    int return_code;        /* 0 converged, 1 iteration cap, 2 damping exhausted, <0 failure             */
    double lp;
    double grad_norm;       /* 2-norm                                                                    */
    int newton_iterations;
    double grad_inf;        /* max-norm at the returned point                                            */
} bdrt_opt_report;
void bdrt_opt_defaults(bdrt_opt_options *o);
int bdrt_optimize(bdrt_problem *p, const double *init_theta, const int *spec, int n_fits, const bdrt_opt_options *opts,
                  double *theta_out, bdrt_opt_report *reports);

/* replaces StanModel.sampling (inversion.py:1218-1221): NUTS, diagonal metric, Stan-2.19 style adaptation.
 * The whole transition loop runs on the GPU (one workgroup per 16 chains); the host only relaunches. */
typedef struct {
    double adapt_delta;     /* 0.9  (inversion.py:1221)                  */
    double adapt_t0;        /* 10   (inversion.py:1221)                  */
    double adapt_gamma;     /* 0.05                                      */
    double adapt_kappa;     /* 0.75                                      */
    int max_treedepth;      /* 10                                        */
    int init_buffer;        /* 75                                        */
    int term_buffer;        /* 50                                        */
    int base_window;        /* 25                                        */
    double init_radius;     /* 2: U(-2,2) on the unconstrained scale     */
    double max_deltaH;      /* 1000                                      */
    double stepsize0;       /* 1                                         */
} bdrt_nuts_control;
typedef struct {
    int64_t n_leapfrog;     /* log_prob+grad evaluations (leapfrogs)     */
    int n_divergent;        /* post-warm-up                              */
    int n_max_treedepth;    /* post-warm-up iterations that hit the cap  */
    double stepsize;        /* adapted step size                         */
    double mean_accept;     /* mean accept_stat post-warm-up             */
} bdrt_chain_diag;
/* bdrt_sampler_create checks the control block the way Stan's services do: adapt_delta in (0,1); adapt_gamma, adapt_kappa,
 * adapt_t0, stepsize0, max_deltaH > 0; init_radius >= 0; window sizes >= 0; max_treedepth in [1,10]; NaN fails every check. */
void bdrt_nuts_defaults(bdrt_nuts_control *c);

typedef struct bdrt_sampler bdrt_sampler;
/* n_units chains; unit u samples spectrum spec[u] (NULL: 0) with RNG stream (seed, chain_id[u]) (NULL: u);
 * init_theta [n_units x D] or NULL (random U(-r,r), retried until finite).
 * Size limits (NULL + bdrt_last_error beyond them): D <= 864 parameters for problems on the LDS-resident evaluators
 * (bdrt_problem_evaluator 0..4: twenty-seven elements per lane of a chain's half-wave), D <= 8192 for problems on the streamed
 * evaluator (code 5: every row in HBM, up to sixteen elements per thread of the cooperative stage).  Stan has no limit
 * (reference bayes_drt/inversion.py:2127-2209); evaluation and MAP have none here either. */
bdrt_sampler *bdrt_sampler_create(bdrt_problem *p, int n_units, const int *spec, const int *chain_id, int warmup,
                                  int n_draws, uint64_t seed, const double *init_theta, const bdrt_nuts_control *ctrl);
void bdrt_sampler_destroy(bdrt_sampler *s);
/* advance every unfinished chain by at most `rounds` leapfrogs (one launch, asynchronous on `stream`);
 * *all_done is set when every chain has produced warmup+n_draws iterations (requires a sync: pass NULL to skip) */
int bdrt_sampler_advance(bdrt_sampler *s, int rounds, int *all_done);
int bdrt_sampler_sync(bdrt_sampler *s);
/* run to completion */
int bdrt_sampler_run(bdrt_sampler *s);
/* draws [n_units x n_draws x D] unconstrained; diag [n_units]; either may be NULL */
int bdrt_sampler_results(bdrt_sampler *s, double *draws_unconstrained, double *lp, bdrt_chain_diag *diag);
/* run to completion.  A run that starts on the 16-chains-per-workgroup kernel (more than four chains per CU) hands its last
 * live chains to the one-chain-per-workgroup kernel once that finishes them sooner (BDRT_TAIL_MIGRATION=0 forbids it);
 * bdrt_sampler_tail_units tells how many chains were handed over (0: none). */
int bdrt_sampler_tail_units(bdrt_sampler *s);
/* A run with more than 16 units per CU re-packs its live chains into fewer 16-chain workgroups whenever 1/16 of the
 * workgroups can be dropped (finished chains), so that the MFMA tiles stay full until fewer than 16 live chains per CU are left;
 * the chains continue bit for bit.  Number of such re-packings so far (BDRT_COMPACTION=0 disables them). */
int bdrt_sampler_compactions(bdrt_sampler *s);
/* which kernel advances the chains now: 0 sixteen chains per workgroup (bdrt_nuts.hip), 1 one chain per workgroup with its
 * state in LDS (bdrt_solo.h: few chains of the single-DRT family), 2 one chain per workgroup, general block model
 * (bdrt_solo_wide.h: few chains of any other model on log-uniform grids), 3 one chain per WAVEFRONT (bdrt_wave.h: the single-DRT
 * family while more than 2.5 and at most 8 chains per CU are running: chosen per launch by the number of live chains), 4 one
 * chain per workgroup on the streamed evaluator of a problem beyond the LDS budget (bdrt_big.h) */
int bdrt_sampler_kind(bdrt_sampler *s);
/* total leapfrogs executed so far, summed over chains (device counter) */
int64_t bdrt_sampler_total_leapfrogs(bdrt_sampler *s);
/* HIP-event time (ms) and launch count of the NUTS kernel accumulated since creation / last reset */
int bdrt_sampler_kernel_time(bdrt_sampler *s, double *ms_total, int64_t *n_launches, int reset);
/* phase profile of the NUTS kernel (development aid): cycles32[0..9] = phases of the log-posterior tile, [10..16] =
 * NUTS stages, summed over workgroups since the last call; enable != 0 switches the in-kernel clock reads on */
int bdrt_sampler_phase_profile(bdrt_sampler *s, int enable, long long *cycles32);
/* convenience: create + run + results.  draws [n_units x n_draws x D] */
int bdrt_sample(bdrt_problem *p, int n_units, const int *spec, const int *chain_id, int warmup, int n_draws,
                uint64_t seed, const double *init_theta, const bdrt_nuts_control *ctrl, double *draws, double *lp,
                bdrt_chain_diag *diag);

/* ---- (3) ridge: Gram matrices and the box-constrained QP (replaces _convex_opt, inversion.py:1043-1067) -- */
/* P = WA_re^T WA_re + WA_im^T WA_im + L2mat ; q = -(WA_re^T WZ_re + WA_im^T WZ_im) + L1vec  (inversion.py:1045-1052)
 * WA [2nf x n] stacked; WZ [2nf]; P [n x n]; q [n]  */
int bdrt_gram(const double *WA, const double *WZ, int nrows, int n, const double *L2mat, const double *L1vec, double *P,
              double *q);
/* min 1/2 x^T P x + q^T x  s.t. x >= lo (lo[i] = -inf allowed): primal-dual interior point with cvxopt-like
 * tolerances (abstol 1e-7, reltol 1e-6, feastol 1e-7).  Returns iterations (>=0) or <0. */
int bdrt_qp_box(const double *P, const double *q, const double *lo, int n, double *x, double *primal_objective);
/* The Gram matrices of ng spectra that share the unweighted A [R x n] (row-major) and differ in their row weights w [ng][R] and
 * targets t [ng][R] (Inverter.ridge_fit_many: the weighting schemes depend on Z), in one launch over (tile, tile, group):
 *   G[g] = sum_r (w_gr A_ri)(w_gr A_rj),  q[g] = -sum_r (w_gr A_ri)(w_gr t_gr) + L1vec     (L1vec [n] or NULL, shared)
 * G [ng][n][n], q [ng][n]; either may be NULL (t is needed for q only).  The operands are the rounded products w_gr * A_ri, in
 * the row order and the groups of four rows per MFMA of the single-spectrum entry, so that every group equals
 * bdrt_gram(diag(w_g) A, diag(w_g) t_g, R, n, NULL, L1vec, ...) bit for bit. */
int bdrt_gram_batch(const double *A, int R, int n, const double *w, const double *t, int ng, const double *L1vec, double *G,
                    double *q);
/* The same solver on the GPU for a batch of nb problems that share n and lo (one workgroup per problem, KKT matrix
 * factored in LDS): P [nb][n][n], q [nb][n], x [nb][n], primal_objective [nb] or NULL, iterations [nb] or NULL.
 * This is what Inverter.ridge_fit / ridge_ReImCV call (reference inversion.py:1043-1067 inside the loops at :560-740 and
 * :902-945); bdrt_qp_box above is the host implementation of the identical algorithm, kept as the checker.
 * Returns 0, or <0 (-3: a KKT matrix was not positive definite, -4: iteration limit). */
int bdrt_qp_box_batch(const double *P, const double *q, const double *lo, int n, int nb, double *x,
                      double *primal_objective, int *iterations);

/* The whole hierarchical ridge fit of Inverter.ridge_fit (reference inversion.py:518-740) for a batch of nb independent
 * fits in ONE launch (one workgroup per fit): the hyper-lambda outer loop -- lambda update (:947-983), penalty matrix
 * (:695-700), the QP of _convex_opt (:1043-1067), convergence test (:730-736) -- runs on the device.  ridge_ReImCV
 * (:902-945) is one call with nb = 2 x len(lambdas).
 *   unknowns: n (series: [R_inf, L/1e-4, x[K]], off = 2; parallel: x[K], off = 0)
 *   G [ng][n][n], qbase [ng][n]: Gram matrices WA^T WA and q = -WA^T WZ + L1_vec of the ng distinct data parts
 *     (Re-Im CV: real part, imaginary part); gsel[nb] picks one per fit
 *   base [3][n][n]: padded M0, M1, M2 (penalty 1 = 'integral') or L_o^T L_o (penalty 0 = 'discrete');
 *     Ls [3][K][n]: the padded L_o themselves (discrete only)
 *   lambda0[nb]; lam0s[nb][3], betas[nb][3]: (2a-2)/(2b) resp. (2a-1)/(2b) and 2a of the reference's prior terms (:608-628)
 *   per iteration, from the previous coefficients x:
 *     discrete:  lambda_o = 1 / ((L_o x)^2 / (beta_o - 1) + 1 / lam0_o)            (:947-954), or with hl_fbeta > 0
 *                lambda_o = lambda0 / ((L_o x)^2 / (max (L_o x)^2 * hl_fbeta) + 1)  (:956-964); 1 for the off leading unknowns
 *     integral:  c = factor_o x (100, 10, 1), C_j = sum_{r != j} c_r sqrt(lambda_r) M_rj c_j, d = c^2 diag(M) + 2b,
 *                lambda = (C^2 - sign(C) C sqrt(4 d (2a-2) + C^2) + 2 d (2a-2)) / (2 d^2), floored at 1e-15  (:973-983)
 *     P = G + sum_o reg_ord[o] sqrt(lambda_o) base_o sqrt(lambda_o);  x = argmin 1/2 x'Px + q'x, x >= lo
 *     stop when mean |(x - x_prev) / x_prev| < xtol (entry 1 -- the inductance -- excluded for the fits on data part g
 *     when bit g of zero_delta1 is set: the reference zeroes it when the inductance is not fitted or only the real part is,
 *     :733-734, so in a Re-Im cross-validation the real-part fits exclude it and the imaginary-part fits do not)
 *   hyper_lambda = 0: one QP with lambda = lambda0 (ordinary ridge).
 * Outputs: coef [nb][n], lam [nb][3][n], cost = 1/2 x'Px + q'x, fun = the QP's primal objective, iters (outer iterations),
 * flags (bit 0 converged, bit 2 a QP reached its iteration limit); optional per-iteration history (all four or none):
 * hist_coef [nb][max_iter][n], hist_lam [nb][max_iter][3][n], hist_fun / hist_cost [nb][max_iter]. */
typedef struct {
    int n, K, off;
    int penalty;            /* 0 discrete, 1 integral */
    int max_iter;
    int hyper_lambda;
    int zero_delta1;        /* bdrt_ridge only.  bit g: fits with gsel == g leave entry 1 out of the convergence test (g < 31) */
    double xtol;
    double hl_fbeta;        /* bdrt_ridge only.  <= 0: analytic discrete update */
    double reg_ord[3];
} bdrt_ridge_options;
int bdrt_ridge(const bdrt_ridge_options *opt, int nb, int ng, const double *G, const double *qbase, const int *gsel,
               const double *base, const double *Ls, const double *lo, const double *lambda0, const double *lam0s,
               const double *betas, const double *x0, double *coef, double *lam, double *cost, double *fun, int *iters,
               int *flags, double *hist_coef, double *hist_lam, double *hist_fun, double *hist_cost);
/* The same fits with one flag per data part and one hl_fbeta per fit instead of the two option fields (which this entry does not
 * read): zero_delta1_g [ng] (non-zero: the fits on data part g leave entry 1 out of the convergence test; any ng),
 * hl_fbeta_b [nb] (<= 0: the analytic update).  bdrt_ridge expands its bit mask and its scalar and calls this entry. */
int bdrt_ridge_ex(const bdrt_ridge_options *opt, const unsigned char *zero_delta1_g, const double *hl_fbeta_b, int nb, int ng,
                  const double *G, const double *qbase, const int *gsel, const double *base, const double *Ls, const double *lo,
                  const double *lambda0, const double *lam0s, const double *betas, const double *x0, double *coef, double *lam,
                  double *cost, double *fun, int *iters, int *flags, double *hist_coef, double *hist_lam, double *hist_fun,
                  double *hist_cost);

/* ---- (4) posterior post-processing on the device ------------------------------------
 * Replaces the numpy reductions applied to the HMC draws right after `sampling`:
 *   np.percentile(samples, q, axis=0)            reference bayes_drt/inversion.py:2560 (coef_percentile), :2702
 *                                                (predict_Z from Z_hat), :3068/:3085 (predict_Rp), :3096-3113 (predict_sigma)
 *   np.percentile(x_samples @ A.T + offsets, ..) reference inversion.py:2716-2735 (predict_Z on new frequencies)
 *
 * out[nq x ncols] (row-major) = percentile q[t] (0..100, numpy's default 'linear' rule, same lerp formula) over the
 * `rows` samples of every column of Y, where Y = X (Phi == NULL, ncols = K) or Y = X Phi^T + bias (Phi is [M x K]
 * row-major, bias [M] or NULL, ncols = M).  X is [rows x K] with row stride ldx >= K (doubles).  A column that
 * contains a NaN yields NaN (numpy behaviour).  Columns of up to 16384 samples are sorted in LDS, longer ones in an HBM
 * scratch buffer (np.percentile has no row limit either). */
int bdrt_percentiles(const double *X, int rows, int K, long ldx, const double *Phi, int M, const double *bias,
                     const double *q, int nq, double *out);
/* The same on the draws a sampler holds on the device (unconstrained parameters theta): samples = all draws of units
 * [unit_lo, unit_hi), columns [col0, col0 + ncols) of theta.  The draws are not copied to the host. */
int bdrt_sampler_percentiles(bdrt_sampler *s, int unit_lo, int unit_hi, int col0, int ncols, const double *Phi, int M,
                             const double *bias, const double *q, int nq, double *out);

/* Per-spectrum posterior summary on the CONSTRAINED scale (what the reference reduces fit['x'], fit['Rinf'], ... to:
 * np.mean(..., axis=0) inversion.py:2517-2519 and np.percentile(..., q, axis=0) :2560): samples = all draws of units
 * [unit_lo, unit_hi); <lower=0> parameters are exp(theta).  mean [D] (may be NULL), pct [nq x D].  This is what a
 * multi-GPU run gathers instead of raw draws. */
int bdrt_sampler_summary(bdrt_sampler *s, int unit_lo, int unit_hi, const double *q, int nq, double *mean, double *pct);
/* the same reduction on host-resident draws X [rows x K] (row stride ldx): is_pos[K] flags the exp() columns (NULL: none) */
int bdrt_summary(const double *X, int rows, int K, long ldx, const unsigned char *is_pos, const double *q, int nq,
                 double *mean, double *pct);
/* HMC convergence diagnostics (pystan's `summary` / `check_hmc_diagnostics`; definitions: tests/diag_numpy.py): for every
 * column, over the chains of one group (a group = the chains of one spectrum), the mean and sd (ddof = 1) of all draws, the
 * non-split effective sample size n_eff (Geyer's initial positive + monotone sequence, Stan 2.19) and the split R-hat.
 * A column with a non-finite draw, or whose draws are all equal, gives n_eff = Rhat = NaN; N < 4 draws give n_eff = NaN.
 * Bit-reproducible (fixed summation order); both entry points run the same kernel, so equal draws give equal bits.
 * Draws of units [unit_lo, unit_hi) of a sampler, on the CONSTRAINED scale (<lower=0> parameters are exp(theta)), grouped by
 * chains_per_group consecutive units: G = (unit_hi - unit_lo) / chains_per_group groups x D columns.  Outputs [G x D]
 * (any may be NULL).  The draws are not copied to the host. */
int bdrt_sampler_diagnostics(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, double *mean, double *sd,
                             double *n_eff, double *rhat);
/* the same reduction on host-resident draws X [G groups][M chains][N draws][C columns], rows of stride ldx >= C doubles;
 * is_pos[C] flags the exp() columns (NULL: none); outputs [G x C].  M <= 64. */
int bdrt_diagnostics(const double *X, int G, int M, int N, int C, long ldx, const unsigned char *is_pos, double *mean,
                     double *sd, double *n_eff, double *rhat);
/* Rank-normalised diagnostics (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; definitions: tests/rank_numpy.py), all on
 * the SPLIT chains Y: chain m gives rows 2m (its first n = N / 2 draws) and 2m + 1 (its last n; an odd N drops the middle
 * draw).  Per column: rhat, the larger of the plain R-hat over the 2M rows of the rank-normalised draws z and of the
 * rank-normalised folded draws |Y - median|; ess_bulk, Geyer's ESS (as n_eff above, 2M chains of n draws) of z; ess_tail, the
 * smaller ESS of the indicators 1[Y <= q], q the p_lo and p_hi quantiles of Y (numpy's linear rule); ess_mean, the ESS of Y;
 * sd of Y (ddof = 1).  Every ESS is capped at S log10 S, S = 2M n.  A column with a non-finite draw, or whose draws are all
 * equal, gives NaN in all five; n < 4 gives NaN ESS, n < 2 NaN rhat; a constant indicator series gives ess_tail = NaN.
 * Outputs [G x C] (any may be NULL).  M <= 64, N >= 2, 0 < p_lo < p_hi < 1 and S <= bdrt_rank_max_draws() (8192), else -1.
 * Bit-reproducible, and a column's results do not depend on what else is in the launch.  Layouts as bdrt_diagnostics /
 * bdrt_sampler_diagnostics; the sampler's draws are not copied to the host. */
int bdrt_rank_diagnostics(const double *X, int G, int M, int N, int C, long ldx, const unsigned char *is_pos, double p_lo,
                          double p_hi, double *rhat, double *ess_bulk, double *ess_tail, double *ess_mean, double *sd);
int bdrt_sampler_rank_diagnostics(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, double p_lo, double p_hi,
                                  double *rhat, double *ess_bulk, double *ess_tail, double *ess_mean, double *sd);
int bdrt_rank_max_draws(void);
/* Model comparison of sampling fits: PSIS-LOO (Vehtari, Gelman, Gabry 2017) and WAIC; definitions: tests/psis_numpy.py.
 * Pointwise log-likelihood of `Z ~ normal(Z_hat, sigma_tot)`: Zhat, sig [G][S][N2] and z [G][N2] on the host (G fits, S draws,
 * N2 = 2 Nf scalar observations).  pair = 0: ll_out [G][S][N2]; pair = 1: ll_out [G][S][N2 / 2], column i = columns i and
 * i + N2 / 2 added (real and imaginary part of one frequency).  A non-positive or non-finite sig gives NaN. */
int bdrt_pointwise_loglik(const double *Zhat, const double *sig, const double *z, int G, int S, int N2, int pair,
                          double *ll_out);
/* Per column of ll [G][S][N] (host; a column = the S log-likelihoods of one observation): lpd = log mean exp(ll), elpd_loo
 * with Pareto-smoothed importance weights, the Pareto shape pareto_k of the weights' tail (inf when at most 4 ratios lie
 * above the cutoff: raw weights), p_waic = var(ll) (ddof = 1) and n_tail, the number of smoothed ratios; outputs [G][N].
 * reff [G][N]: relative efficiency of each column's draws (NULL: 1); tail length M = ceil(min(S / 5, 3 sqrt(S / reff))).
 * A column with a non-finite value gives NaN (n_tail 0), that column only.  2 <= S <= bdrt_psis_loo_max_draws() (-2 above).
 * Bit-reproducible, and a column's results do not depend on what else is in the launch. */
int bdrt_psis_loo(const double *ll, int G, int S, int N, const double *reff, double *lpd, double *elpd_loo, double *pareto_k,
                  double *p_waic, int *n_tail);
int bdrt_psis_loo_max_draws(void);
/* PSIS-LOO predictive checks; definitions: tests/loo_predict_numpy.py.  A unit is one scalar observation (pair = 0, U = N2
 * units per fit) or the real and the imaginary part of one frequency left out together (pair = 1, U = N2 / 2: scalars i and
 * i + N2 / 2).  The unit's log-likelihoods, Pareto-smoothed weights, pareto_k and n_tail are those of bdrt_pointwise_loglik +
 * bdrt_psis_loo to the bit (reff [G][U] or NULL).  Per scalar, outputs [G][N2]: mean and sd of the leave-one-out predictive
 * distribution (the weighted mixture of the draws' normals) and pit, its cdf at the datum; mean_post, sd_post, pit_post: the
 * same with equal weights (the in-sample posterior predictive).  Among equal log ratios in the tail the draw with the smaller
 * index gets the smaller smoothed weight.  A unit with a non-finite log-likelihood gives NaN in all of its outputs (n_tail 0);
 * one whose log-likelihoods are all equal keeps equal weights (pareto_k inf, n_tail 0).  Zhat, sig, z as above on the host.
 * 2 <= S <= bdrt_psis_predict_max_draws() (-2 above).  Bit-reproducible, and a unit's results do not depend on the launch. */
int bdrt_psis_predict(const double *Zhat, const double *sig, const double *z, int G, int S, int N2, int pair, const double *reff,
                      double *mean, double *sd, double *pit, double *mean_post, double *sd_post, double *pit_post,
                      double *pareto_k, int *n_tail);
int bdrt_psis_predict_max_draws(void);
/* The same two reductions on the draws a sampler holds on the device: neither the draws nor Z_hat, sigma_tot or the
 * log-likelihoods travel; only the per-observation results come back.  A group is chains_per_group consecutive units of
 * [unit_lo, unit_hi) that sampled ONE spectrum; its S = chains_per_group * n_draws rows are in the order the host path sees
 * them, chain-major.  2 <= S <= bdrt_psis_loo_max_draws() (-2 above).  Per chunk of groups the batch evaluator (the launch of
 * bdrt_transformed, without spec) gives Z_hat and sigma_tot of the rows where they are, and the kernels of
 * bdrt_pointwise_loglik, bdrt_psis_loo / bdrt_psis_predict reduce them against the data of a group: the problem's own device
 * copy of the group's spectrum, scalar observations [col0, col0 + ncols) of the 2 Nf (the real half, the imaginary half or
 * all; pair = 1 needs all).  U = ncols / 2 (pair = 1) or ncols units per group.
 *   reff_mode 0: reff = 1.  1: reff_in [G][U] (host).  2: the relative efficiency of the likelihood draws: per unit
 *     n_eff(exp(ll - max ll)) / S with chains_per_group chains (the kernel of bdrt_diagnostics), 1 where that is not a positive
 *     finite number.  reff_out [G][U] (may be NULL) returns what was used in every mode.
 *   chunk_bytes: one chunk's device scratch -- per draw row the parameters, Z_hat, sigma_tot, lp and what the reduction stages
 *     (bdrt_sampler_loo_group_bytes per group) -- stays within it; 0: 1 GiB.  A group that alone exceeds it is a chunk of one.
 * Outputs on the host as bdrt_psis_loo's [G][U] and bdrt_psis_predict's ([G][ncols] per scalar, [G][U] per unit).  With
 * reff_mode 0 and 1 every output equals the host-staged entry points on the downloaded draws bit for bit (a row's Z_hat and
 * sigma_tot do not depend on its place in the evaluator's launch; a column's results do not depend on the launch). */
int bdrt_sampler_loo(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0, int ncols, int reff_mode,
                     const double *reff_in, size_t chunk_bytes, double *lpd, double *elpd_loo, double *pareto_k, double *p_waic,
                     int *n_tail, double *reff_out);
int bdrt_sampler_loo_predict(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0, int ncols,
                             int reff_mode, const double *reff_in, size_t chunk_bytes, double *mean, double *sd, double *pit,
                             double *mean_post, double *sd_post, double *pit_post, double *pareto_k, int *n_tail, double *reff_out);
/* device bytes one group adds to a chunk of the two entry points above (predict != 0: of bdrt_sampler_loo_predict); 0: bad arguments */
size_t bdrt_sampler_loo_group_bytes(bdrt_sampler *s, int chains_per_group, int pair, int ncols, int reff_mode, int predict);
/* ---- (4b) held-out frequencies: exact leave-out refits and K-fold cross-validation -----
 * Definitions: tests/heldout_numpy.py.  A fold is a sampling fit on a training grid; these entries say what its draws predict
 * at H frequencies that are not on it.  Outlier error models are refused (-2): a held-out point has no sigma_out of its own.
 *
 * Z_hat and sigma_tot [B][2H] (real halves, then imaginary halves) of B rows of constrained parameters, params [B][D] in the
 * layout bdrt_transformed writes, at freq_test [H] (Hz, positive).  A_test: the prediction rows, per block [2H][K_b] row-major
 * (real rows, then imaginary rows), block after block.  Block flags, x_scale, induc_scale and sigma_min are the problem's.
 * A row's result does not depend on its place in the launch. */
int bdrt_heldout_transformed(bdrt_problem *p, const double *params, int B, const double *freq_test, int H, const double *A_test,
                             double *Z_hat, double *sigma_tot);
/* The predictive of held-out units under equal weights: Zhat, sig [G][S][N2] and z [G][N2] on the host, units as in
 * bdrt_psis_predict (pair).  lpd [G][U] = logsumexp_s(ll_s) - log S, equal to bdrt_psis_loo's lpd on bdrt_pointwise_loglik's
 * output to the bit; mean, sd, pit [G][N2] equal bdrt_psis_predict's mean_post, sd_post, pit_post to the bit.  No Pareto fit is
 * run.  A unit with a non-finite log-likelihood gives NaN in its outputs, that unit only.  2 <= S <= bdrt_psis_loo_max_draws()
 * (-2 above). */
int bdrt_heldout_reduce(const double *Zhat, const double *sig, const double *z, int G, int S, int N2, int pair, double *lpd,
                        double *mean, double *sd, double *pit);
/* Both on the draws a sampler holds, in chunks of groups as bdrt_sampler_loo: per chunk the batch evaluator gives the
 * constrained parameters of the rows, bdrt_heldout_transformed's kernel their Z_hat and sigma_tot at freq_test, and
 * bdrt_heldout_reduce's kernel the results against z_test [G][2H] (host), scalar columns [col0, col0 + ncols) of the 2H (the
 * real half, the imaginary half or all; pair = 1 needs all).  Outputs on the host: lpd [G][U], mean, sd, pit [G][ncols]; each
 * equals the two host-staged entries on the downloaded draws bit for bit.  chunk_bytes: 0: 1 GiB. */
int bdrt_sampler_heldout(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0, int ncols,
                         size_t chunk_bytes, const double *freq_test, int H, const double *A_test, const double *z_test, double *lpd,
                         double *mean, double *sd, double *pit);
/* ---- (4c) held-out frequencies under the outlier error models: sigma_out integrated over its prior -----
 * Definitions: tests/heldout_mix_numpy.py.  The prior of sigma_out is fixed by data, so the predictive of a frequency the fit has
 * not seen is the draw's normal with sigma_out integrated over that prior.  The integral is a table the caller supplies: nodes
 * y [Q] (>= 0) and weights w [Q] (>= 0, summing to 1) with sum_j w_j f(y_j) ~ E f(sigma_out), 1 <= Q <= bdrt_heldout_mix_max_nodes()
 * (-2 above), and ey2 = E[sigma_out^2] (+inf allowed).  shared = 1: the real and the imaginary scalar of a frequency have one
 * sigma_out (outlier_mode 1); 0: one each (outlier_mode 2).  The entries of (4b) keep refusing these models.
 *
 * bdrt_heldout_transformed for a problem WITH an outlier model (-2 without one): sigma_base is sigma_tot without sigma_out. */
int bdrt_heldout_mix_max_nodes(void);
int bdrt_heldout_mix_transformed(bdrt_problem *p, const double *params, int B, const double *freq_test, int H, const double *A_test,
                                 double *Z_hat, double *sigma_base);
/* Zhat, sig_base [G][S][N2], z [G][N2] as in bdrt_heldout_reduce.  Per draw s and scalar, with v_j = sig_base^2 + y_j^2:
 * m_s = sum_j w_j N(z | Zhat, v_j); a pair unit takes the product of the two normals under one sum (shared) or the product of the
 * two sums; lpd [G][U] = log(mean_s m_s), formed from log m_s so that no residual underflows it; mean [G][N2] as in
 * bdrt_heldout_reduce; sd^2 = that entry's sd^2 + ey2; pit = mean_s sum_j w_j Phi((z - Zhat) / sqrt(v_j)), per scalar.  With the
 * table Q = 1, y = 0, w = 1, ey2 = 0 mean, sd and pit have bdrt_heldout_reduce's bits and lpd agrees to rounding.  A unit's
 * result depends on its own rows, S and the table only.  A unit with a non-finite term gives NaN, that unit only.
 * 2 <= S <= bdrt_psis_loo_max_draws() (-2 above). */
int bdrt_heldout_mix_reduce(const double *Zhat, const double *sig_base, const double *z, int G, int S, int N2, int pair, int shared,
                            const double *y, const double *w, int Q, double ey2, double *lpd, double *mean, double *sd, double *pit);
/* Both on the draws a sampler holds, chunked by groups exactly as bdrt_sampler_heldout; each output equals the two host-staged
 * entries on the downloaded draws bit for bit.  -2 for a problem without an outlier model. */
int bdrt_sampler_heldout_mix(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0, int ncols,
                             size_t chunk_bytes, const double *freq_test, int H, const double *A_test, const double *z_test, int shared,
                             const double *y, const double *w, int Q, double ey2, double *lpd, double *mean, double *sd, double *pit);
/* ---- (4d) power-scaling prior and likelihood sensitivity -----
 * Kallioinen, Paananen, Buerkner, Vehtari 2023; definitions: tests/powerscale_numpy.py.  Per fit of S = chains * n_draws draws:
 * the components L_lik = the sum of the pointwise log-likelihoods of scalar observations [col0, col0 + ncols) of the 2 Nf and
 * L_pri = lp0 - L_lik, lp0 the log density without the Jacobian term against the fit's spectrum; four weight vectors, the
 * Pareto-smoothed normalised importance weights of (alpha - 1) L at reff = 1 in the order (prior, alpha_lo), (prior, alpha_hi),
 * (likelihood, alpha_lo), (likelihood, alpha_hi); per constrained parameter (the D columns bdrt_transformed writes) and weight
 * vector cjs2, the squared cumulative Jensen-Shannon distance (base 2, in [0, 1]) between the column's ECDF and the re-weighted
 * one, the larger of the value on the distribution and on the survival functions; ties are ordered by draw index.
 * Outputs on the host: cjs2 [G][D][4], pareto_k and n_tail [G][4] (inf and the raw weights when at most 4 ratios lie above the
 * cutoff or the component is constant).  A component with a non-finite entry gives NaN in its weights, its pareto_k and its
 * cjs2 (n_tail 0); a column with a non-finite value NaN; a constant column 0.  0 < alpha_lo < 1 < alpha_hi.
 * 2 <= S <= bdrt_powerscale_max_draws() (8192; -2 above).  Bit-reproducible, and a fit's results do not depend on what else is in
 * the call or on chunk_bytes (one chunk's device scratch, as in bdrt_sampler_loo; 0: 1 GiB).
 *
 * On host draws: theta [G * S][D] unconstrained, chain-major per fit; spec [G] (NULL: 0) the spectrum of each fit.
 * L_out [G][2][S] (may be NULL): L_pri, L_lik. */
int bdrt_powerscale_max_draws(void);
int bdrt_powerscale(bdrt_problem *p, const double *theta, const int *spec, int G, int chains, int n_draws, int col0, int ncols,
                    double alpha_lo, double alpha_hi, size_t chunk_bytes, double *cjs2, double *pareto_k, int *n_tail, double *L_out);
/* The same on the draws a sampler holds, groups as in bdrt_sampler_loo: nothing but the result planes crosses the bus.  Every
 * output equals bdrt_powerscale on the downloaded draws bit for bit. */
int bdrt_sampler_powerscale(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int col0, int ncols, double alpha_lo,
                            double alpha_hi, size_t chunk_bytes, double *cjs2, double *pareto_k, int *n_tail);
/* device pointer of the draws [n_units x n_draws x D] (unconstrained), valid until bdrt_sampler_destroy: lets a
 * collective library (RCCL) gather draws without a host round trip.  Synchronises the sampler's stream. */
const double *bdrt_sampler_draws_dev(bdrt_sampler *s);

/* ---- misc ----------------------------------------------------------------------------------------- */
const char *bdrt_last_error(void);
int bdrt_device_count(void);
int bdrt_set_device(int dev);
const char *bdrt_version(void);

/* ---- debug (tests): pieces of the optimizer at one point ------------------------------------------------
 * The closed-form Hessian of the log-posterior (optimize mode: no Jacobian term) at the unconstrained point theta [D] for
 * spectrum `spec`, as the Newton iteration of bdrt_optimize builds it: H_out [D x D] row-major on the host.
 * lin = 0: every <lower=0> parameter on the log scale.  lin = 1 (nonnegative coefficients only): the coefficients on the
 * LINEAR scale z = x with their floor, 1e-14 of the largest one; a coefficient within twice the floor whose gradient points
 * below it is held: held_out [D] (may be NULL) is 1.0 there and 0.0 elsewhere, and H has -1 on its diagonal entry and 0 in
 * the rest of its row and column.  Returns 1 when the model has no closed form here (the iteration then differences
 * gradients), or when lin = 1 is asked of a model whose coefficients are free. */
int bdrt_debug_hessian_lin(bdrt_problem *p, const double *theta, int spec, int lin, double *H_out, double *held_out);
/* the same with lin = 0 */
int bdrt_debug_hessian(bdrt_problem *p, const double *theta, int spec, double *H_out);
/* A series of one column y [M][N] (host) as bdrt_rank_diagnostics forms it, z_out [2M][N / 2] in time order.  what = 0: the
 * rank-normalised split draws z; 1: the z of the folded split draws (both NaN for a column that gives NaN); 2: the split
 * draws themselves as the kernel stages them, i.e. exp(y) when is_pos != 0 (the device's exp, which may differ from the
 * host's in the last bit). */
int bdrt_debug_rank_z(const double *y, int M, int N, int is_pos, int what, double *z_out);
/* The two kernels of bdrt_powerscale on supplied data (no problem handle; the current device).
 * The distance kernel: columns X [C][S] and weight vectors w [4][S], taken as they are -> cjs2 [C][4].
 * The weights kernel: components L [G][2][S] -> the log weights lw and the weights w [G][4][S] (either may be NULL), pareto_k,
 * n_tail [G][4].  2 <= S <= bdrt_powerscale_max_draws() (-2 above), C <= 65535. */
int bdrt_debug_powerscale_cjs(const double *X, const double *w, int C, int S, double *cjs2);
int bdrt_debug_powerscale_weights(const double *L, int G, int S, double alpha_lo, double alpha_hi, double *lw, double *w,
                                  double *pareto_k, int *n_tail);

/* One launch of the Newton iteration's damped solve on supplied data (no problem handle; the current device):
 * newton_build_kernel (M = -H + lam I from H), newton_solve_kernel with `natt` attempts (1 .. 6) side by side,
 * newton_gather_kernel.  H [D x D] symmetric, row-major; g, x [D].  The linear scale of the coefficients (slots o_x ..
 * o_x + Kx - 1) when tz is not NULL: tz [D] = dy/dz per slot, held [D] != 0 for a coefficient held at its floor, floor_x the
 * floor; NULL for the log scale (held, floor_x, o_x, Kx are ignored then).  Outputs, on the host: L_out [Dp x Dp], Dp = D
 * rounded up to 16, the matrix of the committed attempt as the kernel leaves it (the factor in its lower triangle, the
 * identity on the padding; what is above the diagonal is not part of the result); s_out [D]; trial_out [4][D], the points for
 * the steps s, s/2, s/4, s/8.  Returns -2 without launching when D needs more LDS than a workgroup can have. */
typedef struct {
    int ok;                 /* the committed attempt factored and gave a finite step */
    int attempt;            /* index of the committed attempt: the first that succeeded, the last one if none did */
    int rc, done;           /* the fit's state after the gather kernel (rc 2, done 1: damping exhausted) */
    double lam;             /* the damping of the committed attempt (beyond 1e12 when none factored) */
    double pred, gs, ss;    /* predicted increase, g.s and s.s as the state holds them (valid when ok) */
} bdrt_newton_solve_record;
int bdrt_debug_newton_solve(const double *H, const double *g, const double *x, int D, double lam, int natt, const double *tz,
                            const double *held, double floor_x, int o_x, int Kx, double *L_out, double *s_out, double *trial_out,
                            bdrt_newton_solve_record *rec);
/* One launch of newton_accept_kernel on supplied data: the verdict on the four trial points.  st: the fit's state before
 * (lp, lam, pred, gs, ss, grad_inf, tol, iters, max_iter, lin are read; rc, done, need_hess, n_evals are taken as given) and
 * after.  x, g [D]: in and out; trial [4][D], lp_t [4], gt [4][D]: the trial points, their log-posteriors and gradients.
 * tz, held, floor_x, o_x, Kx as above (they matter when st->lin != 0; tz == NULL clears lin). */
typedef struct {
    double lp, lam, pred, gs, ss, grad_inf, tol, lp_trial;
    int iters, max_iter, lin, rc, done, need_hess, n_evals, pad;
} bdrt_newton_state;
int bdrt_debug_newton_accept(bdrt_newton_state *st, double *x, double *g, int D, const double *trial, const double *lp_t,
                             const double *gt, const double *tz, const double *held, double floor_x, int o_x, int Kx);

/* One launch of the box-QP solver's linear algebra on supplied data (no problem handle; the current device), one 512-thread
 * workgroup per problem: the device code of bdrt_qp_box_batch / bdrt_ridge forms M = (P + P^T) / 2 + diag(dg) + reg I as a packed
 * lower triangle and factors it, reg = 0 first and then 1e-14 (1 + |M(0,0)|), x 100 per rung while reg <= 1e6, until a Cholesky
 * factorisation runs to completion; then both substitutions once per right-hand side on that factor.
 * P [nb][n][n] row-major, not necessarily symmetric; dg [nb][n] (the role of z / s); rhs [nb][nrhs][n] (nrhs may be 0).
 * place = 0: the triangle in LDS (returns -2 without launching when it does not fit: n > 185); 1: in a global work buffer.
 * Outputs per problem: rec [nb]; L_out [nb][n][n], the factor as a dense lower triangle with its diagonal (zeros above);
 * piv_out [nb][n], the pivots the factorisation met (L(j,j)^2 up to the rounding of the square root); sol_out [nb][nrhs][n].
 * L_out and piv_out may be NULL.  A problem that no rung factors has ok = 0 and leaves its part of L_out, piv_out and sol_out
 * as the caller passed it; the call then returns -3, as bdrt_qp_box_batch does. */
typedef struct {
    int ok;                 /* a rung factored */
    int rungs;              /* factorisations tried: 1 when reg = 0 sufficed */
    double reg;             /* the reg added last (ok = 0: the first value beyond 1e6, or NaN) */
} bdrt_qp_factor_record;
int bdrt_debug_qp_factor_solve(const double *P, const double *dg, int n, int nb, int place, const double *rhs, int nrhs,
                               bdrt_qp_factor_record *rec, double *L_out, double *piv_out, double *sol_out);

#ifdef __cplusplus
}
#endif
#endif
