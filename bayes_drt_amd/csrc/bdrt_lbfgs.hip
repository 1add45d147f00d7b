// bdrt_lbfgs.hip -- MAP estimation: replaces StanModel.optimizing (reference bayes_drt/inversion.py:1216).
//
// L-BFGS on the unconstrained scale, log-density without Jacobian (Stan's `optimizing` semantics),
// history 5, strong-Wolfe line search (c1 = 1e-4, c2 = 0.9) with cubic interpolation, first step alpha0 = 1e-3 and
// Stan's five termination tests (tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param).
// Stan's exact iterate path is not reproducible (its source is not in the reference; H1), only its contract.
//
// MI355X design: bdrt_optimize is four steps -- checks; the L-BFGS phase, one launch for the whole batch where the problem takes
// the device-resident kernel (lbfgs_device, bdrt_lbfgs_dev.h), else lbfgs_host: a per-fit state machine on the host (LbfgsFit,
// bdrt_lbfgs.h) whose fits advance in lock-step, every log_prob+gradient they ask for evaluated on the GPU by one launch for the
// batch (one 16-column MFMA tile per 16 fits); the second-order polish, on the device (newton_phase -> bdrt_newton.hip: Hessian,
// blocked MFMA Cholesky, damped step and acceptance test without leaving HBM); the reports (write_results).
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstring>

#include "bdrt_host.h"
#include "bdrt_lbfgs.h"

using namespace bdrt;

namespace bdrt {

// The host-driven L-BFGS phase: every fit that is not done asks for one evaluation per round, at most max_rounds rounds.
static int lbfgs_host(Problem &P, const int *spec, std::vector<LbfgsFit> &fits, long long max_rounds)
{
    const size_t D = P.dev.D, MAXCOLS = 16384;        // columns per launch (PCIe staging bounded to ~45 MB each way)
    // staging: sized by the requests of a round, on the first round that has any -- the default path (no L-BFGS phase, or the
    // device-resident one) has none, and 2 x 22 MB of zero-filled host vectors + as much device scratch per call were a third of a
    // K = 81 fit (12 of 35 ms)
    std::vector<double> h_theta, lp, grad;
    std::vector<int> h_spec, live;                    // live: the fits that ask, in order
    for (long long round = 0; round < max_rounds; ++round) {
        live.clear();
        for (size_t i = 0; i < fits.size(); ++i) if (fits[i].phase != LbfgsFit::DONE) live.push_back((int)i);
        if (live.empty()) break;
        const size_t cols = std::min(MAXCOLS, live.size());
        if (int rc = P.ensure_scratch(cols)) return rc;
        if (h_theta.size() < cols * D) { h_theta.resize(cols * D); h_spec.resize(cols); }
        lp.resize(live.size()); grad.resize(live.size() * D);
        for (size_t base = 0; base < live.size(); base += MAXCOLS) {
            const int B = (int)std::min(MAXCOLS, live.size() - base);
            for (int k = 0; k < B; ++k) {
                memcpy(&h_theta[(size_t)k * D], fits[live[base + k]].trial(), D * sizeof(double));
                h_spec[k] = spec ? spec[live[base + k]] : 0;
            }
            BDRT_HIP(hipMemcpyAsync(P.d_theta, h_theta.data(), (size_t)B * D * sizeof(double), hipMemcpyHostToDevice, P.stream));
            BDRT_HIP(hipMemcpyAsync(P.d_spec, h_spec.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, P.stream));
            if (int rc = launch_logp_grad(&P, P.d_theta, P.d_spec, B, /*jacobian=*/0, P.d_lp, P.d_grad, nullptr, nullptr, nullptr, P.stream))
                return rc;
            BDRT_HIP(hipMemcpyAsync(&lp[base], P.d_lp, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, P.stream));
            BDRT_HIP(hipMemcpyAsync(&grad[base * D], P.d_grad, (size_t)B * D * sizeof(double), hipMemcpyDeviceToHost, P.stream));
            BDRT_HIP(hipStreamSynchronize(P.stream));
        }
        for (size_t k = 0; k < live.size(); ++k) fits[live[k]].feed_any(lp[k], &grad[k * D]);
    }
    return 0;
}

// what the Newton phase leaves: slot[i], the position of fit i in the polished batch (-1: not polished), the rest per position
struct Polished { std::vector<int> slot; std::vector<double> x; std::vector<NewtonReport> rep; };

// Newton polish of every fit whose L-BFGS phase ended normally, all on the device
static int newton_phase(Problem &P, const int *spec, const std::vector<LbfgsFit> &fits, const bdrt_opt_options &o, Polished &nw)
{
    std::vector<double> x0;
    std::vector<int> nspec;
    nw.slot.assign(fits.size(), -1);
    for (size_t i = 0; i < fits.size(); ++i)
        if (o.newton_max_iter > 0 && fits[i].rc >= 0) {
            nw.slot[i] = (int)nspec.size();
            nspec.push_back(spec ? spec[i] : 0);
            x0.insert(x0.end(), fits[i].x.begin(), fits[i].x.end());
        }
    if (nspec.empty()) return 0;
    nw.x.resize(x0.size()); nw.rep.resize(nspec.size());
    return newton_polish_device(P, x0.data(), nspec.data(), (int)nspec.size(), o.newton_max_iter, o.newton_tol, nw.x.data(), nw.rep.data());
}

// theta and the report of every fit: from the polish where it ran, else from the L-BFGS state
static void write_results(const std::vector<LbfgsFit> &fits, const Polished &nw, size_t D, double *theta_out, bdrt_opt_report *reports)
{
    for (size_t i = 0; i < fits.size(); ++i) {
        const LbfgsFit &L = fits[i];
        const int a = nw.slot[i];
        memcpy(theta_out + i * D, a >= 0 ? &nw.x[(size_t)a * D] : L.x.data(), D * sizeof(double));
        if (!reports) continue;
        bdrt_opt_report &R = reports[i];
        R.iterations = L.iters;
        R.n_evals = L.n_evals + (a >= 0 ? nw.rep[a].n_evals : 0);
        R.newton_iterations = a >= 0 ? nw.rep[a].iters : 0;
        if (a >= 0) {
            R.return_code = nw.rep[a].rc;
            R.lp = nw.rep[a].lp;
            R.grad_inf = R.grad_norm = nw.rep[a].grad_inf;      // the polish tracks the max-norm only
        } else {
            R.return_code = L.phase == LbfgsFit::DONE ? L.rc : 1;
            R.lp = -L.f;
            R.grad_norm = std::sqrt(LbfgsFit::dot(L.g, L.g));
            double m = 0; for (double v : L.g) m = std::max(m, std::fabs(v));
            R.grad_inf = m;
        }
    }
}

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
    // 1. checks
    if (!p || !init_theta || !theta_out || n_fits < 1) { set_error("bdrt_optimize: bad arguments"); return -1; }
    bdrt_opt_options o;
    if (opts) o = *opts; else bdrt_opt_defaults(&o);
    Problem &P = p->impl;
    const int D = P.dev.D;
    for (int i = 0; i < n_fits; ++i)
        if (spec && (spec[i] < 0 || spec[i] >= P.dev.n_spectra)) { set_error("bdrt_optimize: spectrum index out of range"); return -1; }
    // 2. the L-BFGS phase: all of it when there is no polish, else the lbfgs_before_newton iterations in front of it (0: none)
    bdrt_opt_options ol = o;
    if (o.newton_max_iter > 0) ol.max_iter = std::min(o.max_iter, std::max(o.lbfgs_before_newton, 0));
    std::vector<LbfgsFit> fits((size_t)n_fits);
    for (int i = 0; i < n_fits; ++i) {
        fits[i].init(D, init_theta + (size_t)i * D, &ol);
        if (ol.max_iter <= 0) fits[i].phase = LbfgsFit::DONE;
    }
    // On the device when the problem takes one of the one-chain evaluators (every model on log-uniform grids): one launch, a
    // workgroup per fit, the decisions of bdrt_lbfgs.h (bdrt_lbfgs_dev.h).  BDRT_HOST_LBFGS=1 keeps the host-driven loop, which
    // also serves the problems without a Toeplitz structure (lbfgs_device returns 1) and finds nothing to do after the kernel.
    int rc;
    if (ol.max_iter > 0 && !getenv("BDRT_HOST_LBFGS")) {
        std::vector<double> xo((size_t)n_fits * D), go((size_t)n_fits * D), fv(n_fits);
        std::vector<int> it(n_fits), ne(n_fits), rcv(n_fits);
        if ((rc = lbfgs_device(P, init_theta, spec, n_fits, ol, xo.data(), go.data(), it.data(), ne.data(), rcv.data(), fv.data())) < 0) return rc;
        if (rc == 0)
            for (int i = 0; i < n_fits; ++i) fits[i].load(&xo[(size_t)i * D], &go[(size_t)i * D], fv[i], it[i], ne[i], rcv[i]);
    }
    if ((rc = lbfgs_host(P, spec, fits, (long long)o.max_iter * 70 + (long long)o.newton_max_iter * 60 + 1000))) return rc;
    // 3. the Newton phase, 4. the reports
    Polished nw;
    if ((rc = newton_phase(P, spec, fits, o, nw))) return rc;
    write_results(fits, nw, (size_t)D, theta_out, reports);
    return 0;
}

}  // extern "C"
