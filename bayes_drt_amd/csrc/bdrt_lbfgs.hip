// bdrt_lbfgs.hip -- MAP estimation: replaces StanModel.optimizing (reference bayes_drt/inversion.py:1216).
//
// L-BFGS on the unconstrained scale, log-density without Jacobian (Stan's `optimizing` semantics),
// history 5, strong-Wolfe line search (c1 = 1e-4, c2 = 0.9) with cubic interpolation, first step alpha0 = 1e-3 and
// Stan's five termination tests (tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param).
// Stan's exact iterate path is not reproducible (its source is not in the reference; H1), only its contract.
//
// MI355X design: the L-BFGS phase is a per-fit state machine on the host; every log_prob+gradient it asks for is
// evaluated on the GPU, and all fits (spectra / restarts) advance in lock-step so that one kernel launch serves
// the whole batch (one 16-column MFMA tile per 16 fits).  The second-order polish that follows runs on the device
// (bdrt_newton.hip): Hessian probes, blocked MFMA Cholesky, damped step and acceptance test without leaving HBM.
#include <cstdlib>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <deque>

#include "bdrt_host.h"
#include "bdrt_lbfgs.h"
#include "bdrt_newton.h"

using namespace bdrt;

namespace bdrt {

struct FitDriver {
    LbfgsFit L;
    int stage = 0;     // 0 L-BFGS, 2 done (the Newton polish runs afterwards, on the device: bdrt_newton.hip)
    int nreq() const { return stage == 0 ? 1 : 0; }
    const double *req(int) const { return L.trial(); }
};

}  // namespace bdrt

extern "C" {

void bdrt_opt_defaults(bdrt_opt_options *o)
{
    o->max_iter = 50000; o->history = 5; o->init_alpha = 1e-3; o->tol_obj = 1e-12; o->tol_rel_obj = 1e4;
    o->tol_grad = 1e-8; o->tol_rel_grad = 1e7; o->tol_param = 1e-8;
    o->newton_max_iter = 2000; o->lbfgs_before_newton = 0; o->newton_tol = 1e-8;
    if (const char *e = getenv("BDRT_LBFGS_BEFORE_NEWTON")) o->lbfgs_before_newton = atoi(e);     // (measurements)
}

int bdrt_optimize(bdrt_problem *p, const double *init_theta, const int *spec, int n_fits, const bdrt_opt_options *opts,
                  double *theta_out, bdrt_opt_report *reports)
{
    if (!p || !init_theta || !theta_out || n_fits < 1) { set_error("bdrt_optimize: bad arguments"); return -1; }
    bdrt_opt_options o;
    if (opts) o = *opts; else bdrt_opt_defaults(&o);
    Problem &P = p->impl;
    const int D = P.dev.D;
    for (int i = 0; i < n_fits; ++i)
        if (spec && (spec[i] < 0 || spec[i] >= P.dev.n_spectra)) { set_error("bdrt_optimize: spectrum index out of range"); return -1; }
    bdrt_opt_options ol = o;                          // L-BFGS phase
    if (o.newton_max_iter > 0) ol.max_iter = std::min(o.max_iter, std::max(o.lbfgs_before_newton, 0));
    std::vector<FitDriver> fits((size_t)n_fits);
    for (int i = 0; i < n_fits; ++i) {
        fits[i].L.init(D, init_theta + (size_t)i * D, &ol);
        if (ol.max_iter <= 0) { fits[i].L.phase = LbfgsFit::DONE; }
    }
    auto advance_stage = [&](FitDriver &F) {
        if (F.stage == 0 && F.L.phase == LbfgsFit::DONE) F.stage = 2;
    };
    // The whole L-BFGS phase on the device when the problem takes one of the one-chain evaluators (every model on log-uniform
    // grids): one launch, a workgroup per fit, the decisions of bdrt_lbfgs.h (bdrt_lbfgs_dev.h).  BDRT_HOST_LBFGS=1 keeps the
    // host-driven loop below, which also serves the problems without a Toeplitz structure.
    if (ol.max_iter > 0 && !getenv("BDRT_HOST_LBFGS")) {
        std::vector<double> xo((size_t)n_fits * D), go((size_t)n_fits * D), fv(n_fits);
        std::vector<int> it(n_fits), ne(n_fits), rcv(n_fits);
        const int drc = lbfgs_device(P, init_theta, spec, n_fits, ol, xo.data(), go.data(), it.data(), ne.data(), rcv.data(), fv.data());
        if (drc < 0) return drc;
        if (drc == 0)
            for (int i = 0; i < n_fits; ++i) fits[i].L.load(&xo[(size_t)i * D], &go[(size_t)i * D], fv[i], it[i], ne[i], rcv[i]);
    }
    for (auto &F : fits) advance_stage(F);

    const size_t MAXCOLS = 16384;                      // columns per launch (PCIe staging bounded to ~45 MB each way)
    int rc;
    // staging of the host-driven loop: sized by the requests of a round, on the first round that has any -- the default path (no
    // L-BFGS phase, or the device-resident one) has none, and 2 x 22 MB of zero-filled host vectors + as much device scratch per call
    // were a third of a K = 81 fit (12 of 35 ms)
    std::vector<double> h_theta;
    std::vector<int> h_spec;
    std::vector<double> fit_lp, fit_grad;             // per-fit assembly buffers for multi-request phases
    const long long max_rounds = (long long)o.max_iter * 70 + (long long)o.newton_max_iter * 60 + 1000;
    for (long long round = 0; round < max_rounds; ++round) {
        // gather the requests of this round: list of (fit, request index)
        std::vector<std::pair<int, int>> reqs;
        for (int i = 0; i < n_fits; ++i) {
            const int n = fits[i].nreq();
            for (int k = 0; k < n; ++k) reqs.emplace_back(i, k);
        }
        if (reqs.empty()) break;
        // results per fit (request order)
        std::vector<size_t> off((size_t)n_fits + 1, 0);
        for (int i = 0; i < n_fits; ++i) off[i + 1] = off[i] + (size_t)fits[i].nreq();
        fit_lp.resize(reqs.size());
        fit_grad.resize(reqs.size() * (size_t)D);
        {
            const size_t cols = std::min(MAXCOLS, reqs.size());
            if ((rc = P.ensure_scratch(cols))) return rc;
            if (h_theta.size() < cols * D) { h_theta.resize(cols * D); h_spec.resize(cols); }
        }
        for (size_t base = 0; base < reqs.size(); base += MAXCOLS) {
            const int B = (int)std::min(MAXCOLS, reqs.size() - base);
            for (int k = 0; k < B; ++k) {
                const auto &rq = reqs[base + k];
                memcpy(&h_theta[(size_t)k * D], fits[rq.first].req(rq.second), D * sizeof(double));
                h_spec[k] = spec ? spec[rq.first] : 0;
            }
            BDRT_HIP(hipMemcpyAsync(P.d_theta, h_theta.data(), (size_t)B * D * sizeof(double), hipMemcpyHostToDevice, P.stream));
            BDRT_HIP(hipMemcpyAsync(P.d_spec, h_spec.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, P.stream));
            if ((rc = launch_logp_grad(&P, P.d_theta, P.d_spec, B, /*jacobian=*/0, P.d_lp, P.d_grad, nullptr, nullptr,
                                       nullptr, P.stream)))
                return rc;
            BDRT_HIP(hipMemcpyAsync(&fit_lp[base], P.d_lp, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, P.stream));
            BDRT_HIP(hipMemcpyAsync(&fit_grad[base * D], P.d_grad, (size_t)B * D * sizeof(double), hipMemcpyDeviceToHost, P.stream));
            BDRT_HIP(hipStreamSynchronize(P.stream));
        }
        for (int i = 0; i < n_fits; ++i) {
            FitDriver &F = fits[i];
            if (F.stage == 2) continue;
            const double *lps = &fit_lp[off[i]];
            const double *grs = &fit_grad[off[i] * D];
            F.L.feed_any(lps[0], grs);
            advance_stage(F);
        }
    }
    // ---- second phase: Newton polish of every fit whose L-BFGS phase ended normally, all on the device ----
    std::vector<int> nw_idx;
    for (int i = 0; i < n_fits; ++i)
        if (o.newton_max_iter > 0 && fits[i].L.rc >= 0) nw_idx.push_back(i);
    const int nn = (int)nw_idx.size();
    std::vector<double> nx((size_t)nn * D), nout((size_t)nn * D), nlp(nn), ngi(nn);
    std::vector<int> nit(nn), nrc(nn), nev(nn), nspec(nn);
    if (nn > 0) {
        for (int a = 0; a < nn; ++a) {
            memcpy(&nx[(size_t)a * D], fits[nw_idx[a]].L.x.data(), D * sizeof(double));
            nspec[a] = spec ? spec[nw_idx[a]] : 0;
        }
        if ((rc = newton_polish_device(P, nx.data(), nspec.data(), nn, o.newton_max_iter, o.newton_tol, nout.data(), nlp.data(),
                                       ngi.data(), nit.data(), nrc.data(), nev.data())))
            return rc;
    }
    std::vector<int> slot((size_t)n_fits, -1);
    for (int a = 0; a < nn; ++a) slot[nw_idx[a]] = a;
    for (int i = 0; i < n_fits; ++i) {
        FitDriver &F = fits[i];
        const int a = slot[i];
        const double *x = a >= 0 ? &nout[(size_t)a * D] : F.L.x.data();
        memcpy(theta_out + (size_t)i * D, x, D * sizeof(double));
        if (reports) {
            bdrt_opt_report &R = reports[i];
            R.iterations = F.L.iters;
            R.n_evals = F.L.n_evals + (a >= 0 ? nev[a] : 0);
            R.newton_iterations = a >= 0 ? nit[a] : 0;
            if (a >= 0) {
                R.return_code = nrc[a];
                R.lp = nlp[a];
                R.grad_inf = ngi[a];
                R.grad_norm = ngi[a];                  // the polish tracks the max-norm only
            } else {
                R.return_code = F.L.phase == LbfgsFit::DONE ? F.L.rc : 1;
                R.lp = -F.L.f;
                R.grad_norm = std::sqrt(LbfgsFit::dot(F.L.g, F.L.g));
                double m = 0; for (double v : F.L.g) m = std::max(m, std::fabs(v));
                R.grad_inf = m;
            }
        }
    }
    return 0;
}

// closed-form Hessian of the log-posterior (no Jacobian) at one unconstrained point, as the Newton iteration uses it (tests):
// H_out [D x D] row-major; returns 1 when the model has no closed form here (the iteration then differences gradients)
// lin = 1: with the coefficients of a Series_pos model on the linear scale (the iteration's own rule picks the branch: lam = 0);
// held_out [D] (may be null): 1.0 for the coefficients held at their floor.  1 as well when lin is asked of a model without <lower=0> coefficients
int bdrt_debug_hessian_lin(bdrt_problem *p, const double *theta, int spec, int lin, double *H_out, double *held_out)
{
    if (!p || !theta || !H_out || spec < 0 || spec >= p->impl.dev.n_spectra || lin < 0 || lin > 1) { set_error("bdrt_debug_hessian_lin: bad arguments"); return -1; }
    return hessian_at_point(p->impl, theta, spec, lin, H_out, held_out);
}

int bdrt_debug_hessian(bdrt_problem *p, const double *theta, int spec, double *H_out)
{
    return bdrt_debug_hessian_lin(p, theta, spec, 0, H_out, nullptr);
}

// one launch of the Newton iteration's damped solve / of its verdict on the trial points, on the caller's data (tests)
int bdrt_debug_newton_solve(const double *H, const double *g, const double *x, int D, double lam, int natt, const double *tz,
                            const double *held, double floor_x, int o_x, int Kx, double *L_out, double *s_out, double *trial_out,
                            bdrt_newton_solve_record *rec)
{
    if (!H || !g || !x || !L_out || !s_out || !trial_out || !rec || D < 1 || natt < 1 || natt > 6 || !(lam > 0.0) ||
        (tz && (o_x < 0 || Kx < 0 || o_x + Kx > D))) { set_error("bdrt_debug_newton_solve: bad arguments"); return -1; }
    return newton_solve_at(H, g, x, D, lam, natt, tz, held, floor_x, o_x, Kx, L_out, s_out, trial_out, rec);
}

int bdrt_debug_newton_accept(bdrt_newton_state *st, double *x, double *g, int D, const double *trial, const double *lp_t,
                             const double *gt, const double *tz, const double *held, double floor_x, int o_x, int Kx)
{
    if (!st || !x || !g || !trial || !lp_t || !gt || D < 1 || (tz && (o_x < 0 || Kx < 0 || o_x + Kx > D))) {
        set_error("bdrt_debug_newton_accept: bad arguments"); return -1;
    }
    return newton_accept_at(st, x, g, D, trial, lp_t, gt, tz, held, floor_x, o_x, Kx);
}

}  // extern "C"
