// bdrt_host.h -- host-side objects shared by the translation units of libbdrt.so
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bdrt.h"
#include "bdrt_device.h"
#include "bdrt_tile_s1.h"
#include "bdrt_tile_hw.h"

namespace bdrt {

void set_error(const char *fmt, ...);

#define BDRT_HIP(call)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            bdrt::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return -10;                                                                             \
        }                                                                                           \
    } while (0)

// The HIP current device is per host thread.  bdrt_set_device records the process-wide device; entry points that take no
// handle (bdrt_build_*, bdrt_gram, bdrt_qp_box_batch, bdrt_percentiles) bind the calling thread to it, entry points that
// take a problem / sampler bind to the device the problem was created on.
extern std::atomic<int> g_process_device;
inline void bind_process_device()
{
    const int d = g_process_device.load(std::memory_order_relaxed);
    if (d >= 0) hipSetDevice(d);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: high-water mark per device id, guarded by a mutex.
struct LdsAttrCache {
    std::mutex mu;
    size_t hw[64] = {};
    template <class F>
    hipError_t ensure(size_t bytes, F set_attrs)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> g(mu);
        if (dev >= 0 && dev < 64 && bytes <= hw[dev]) return hipSuccess;
        e = set_attrs();
        if (e == hipSuccess && dev >= 0 && dev < 64) hw[dev] = bytes;
        return e;
    }
    // the common case: every kernel of `fns` gets the limit `bytes`
    hipError_t raise(size_t bytes, std::initializer_list<const void *> fns)
    {
        return ensure(bytes, [&]() {
            hipError_t e = hipSuccess;
            for (const void *f : fns) if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            return e; });
    }
};

// move-only owner of one device allocation of n elements of T: hipFree on destruction, unless released
template <class T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.release()) {}
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t n)      // (a failed allocation leaves the owner empty)
    {
        reset();
        const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void reset() { if (p) hipFree(p); p = nullptr; }
    T *release() { T *q = p; p = nullptr; return q; }
    operator T *() const { return p; }
};

// host staging of the entry points that take host arrays: status 0 or -10, error text set
// d <- a fresh device buffer holding the n elements at h
template <class T>
int upload(DevBuf<T> &d, const T *h, size_t n)
{
    BDRT_HIP(d.alloc(n));
    BDRT_HIP(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// h <- the n elements at d
template <class T>
int download(T *h, const T *d, size_t n)
{
    BDRT_HIP(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// the same two copies enqueued on a stream, between buffers that exist: the caller synchronises
template <class T>
int upload(T *d, const T *h, size_t n, hipStream_t stream)
{
    BDRT_HIP(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, stream));
    return 0;
}
template <class T>
int download(T *h, const T *d, size_t n, hipStream_t stream)
{
    BDRT_HIP(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, stream));
    return 0;
}

// host draws of `rows` rows of C columns, leading dimension ld >= C: everything up to the last row's last column
inline int upload_rows(DevBuf<double> &d, const double *X, size_t rows, long ld, int C)
{
    return upload(d, X, (rows - 1) * (size_t)ld + (size_t)C);
}

// k result planes of n elements each, adjacent on the device, to the host arrays outs[0 .. k); null outputs are skipped
inline int download_planes(const double *d, size_t n, double *const *outs, int k)
{
    for (int i = 0; i < k; ++i)
        if (outs[i]) BDRT_HIP(hipMemcpy(outs[i], d + (size_t)i * n, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// grid.y holds at most 65535 blocks: launch(g0, gn) for the chunks [g0, g0 + gn) of G groups, in order
template <class F>
int for_grid_y_chunks(int G, F launch)
{
    for (int g0 = 0; g0 < G; g0 += 65535) {
        launch(g0, std::min(G - g0, 65535));
        BDRT_HIP(hipGetLastError());
    }
    return 0;
}

// owners of a stream / an event that live as long as the object that holds them (neither copied nor moved)
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e) hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

// Every device allocation of a problem is a member that frees itself.  MEMBER ORDER is the order of release: members are
// destroyed last to first, so the stream and the event stand before every buffer -- the buffers are freed first (hipFree waits
// for the device), then the event, then the stream.
struct Problem {
    Stream stream;
    // problems beyond the LDS budget (bdrt_big.h): the event the last launch on the per-point workspace recorded (see d_bigws)
    Event bigws_done;
    DevProblem dev;                 // device view (pointers are device pointers), host copy
    DevBuf<DevProblem> d_dev;       // the same struct in HBM: kernels take it by pointer (uniform scalar loads)
    int sync_dev();                 // upload `dev` to d_dev
    std::vector<DevBuf<char>> tables;   // the constant tables `dev` points to (matrices in fragment order, generators, ...)
    std::vector<unsigned char> is_pos;
    size_t lds_bytes = 0;
    int device = 0;
    DevBuf<double> d_Z;
    size_t z_capacity = 0;          // doubles
    // host copies of the layout
    int o_x[MAXB], o_ups[MAXB], o_d[MAXB];
    // scratch buffers for host-pointer entry points (grown on demand)
    DevBuf<double> d_theta, d_grad, d_lp;
    DevBuf<int> d_spec;
    size_t scratch_rows = 0;        // (0 after a failed growth)
    int ensure_scratch(size_t rows);
    // launch_logp_grad_few: which one-workgroup-per-point evaluator the problem takes (-1 not looked at yet, 0 none, 1 the
    // headline family's, 2 the general one), decided once -- the call is launch-latency-bound, host microseconds count
    int few_kind = -1, few_ncu = 0;
    // problems beyond the LDS budget (bdrt_big.h): per-point workspace of the evaluator, grown on demand
    // (ONE buffer per problem, indexed by workgroup: launches on different streams take turns -- each waits for the event the
    // one before it recorded --, and the bookkeeping is under a mutex)
    DevBuf<double> d_bigws;
    size_t bigws_doubles = 0;       // (0 after a failed growth)
    std::mutex bigws_mu;
    int ensure_bigws(size_t doubles);
};

// launch the batched evaluator on device buffers (theta/grad [B x D] row-major)
int launch_logp_grad(Problem *p, const double *d_theta, const int *d_spec, int B, int jacobian, double *d_lp,
                     double *d_grad, double *d_params, double *d_Zhat, double *d_sig, hipStream_t stream);

// Few points (B <= #CUs): one WORKGROUP per point with the Toeplitz / banded structure of the problem instead of one
// 16-column MFMA tile with B live columns (bdrt_solo.h / bdrt_solo_wide.h evaluators; defined in bdrt_nuts.hip).  Returns 1
// when the problem / batch does not take that path (nothing launched), 0 when launched, < 0 on error.  Same formulas, other
// summation order: results agree with the tile evaluator to ~1e-13 relative, not bit for bit.
int launch_logp_grad_few(Problem *p, const double *d_theta, const int *d_spec, int B, int jacobian, double *d_lp, double *d_grad,
                         hipStream_t stream, int any_b = 0);

// the Stan-style L-BFGS of n fits as one launch (bdrt_lbfgs_dev.h; defined in bdrt_nuts.hip); 1: not applicable to this problem
int lbfgs_device(Problem &P, const double *x0, const int *spec, int n, const bdrt_opt_options &o, double *x_out, double *g_out,
                 int *iters, int *n_evals, int *rc, double *f);

// percentiles of X Phi^T + bias (Phi == nullptr: of X itself) over the rows of a DEVICE matrix X; Phi, bias, q, out: host
// expcol[K] (host, Phi == nullptr only): columns whose samples are exp(X); mean[ncols] (host): sample means; both optional
int post_percentiles_device(const double *dX, int rows, int K, long ldx, const double *Phi, int M, const double *bias,
                            const double *q, int nq, double *out, const unsigned char *expcol = nullptr,
                            double *mean = nullptr);

// HMC convergence diagnostics (bdrt_diag.hip) of G groups x M chains x N draws x C columns of DEVICE draws: element (g, m, t, c)
// at dX[(g*M + m) * unit_stride + t * row_stride + c]; is_pos[C] (host, optional): exp() columns; outputs [G x C] on the host
int diagnostics_to_host(const double *dX, long unit_stride, long row_stride, const unsigned char *is_pos, int G, int M, int N,
                        int C, double *mean, double *sd, double *n_eff, double *rhat, hipStream_t stream);

// the same with the flags and the four outputs [G x C] on the DEVICE (dExp may be null); returns after the stream has finished
int diagnostics_device(const double *dX, long unit_stride, long row_stride, const unsigned char *dExp, int G, int M, int N, int C,
                       double *dMean, double *dSd, double *dNeff, double *dRhat, hipStream_t stream);

// PSIS-LOO and the LOO predictive check of draws that are on the device (bdrt_sampler_loo, bdrt_sampler_loo_predict; bdrt_loo.hip,
// bdrt_loo_predict.hip).  G groups of S = chains * n_draws consecutive rows (chain-major) of `draws`; per chunk of groups the batch
// evaluator gives Z_hat and sigma_tot of the rows, and the kernels of the host-staged entry points reduce them against the data
// row of the group's spectrum, scalar observations [col0, col0 + ncols) of the 2 Nf.  Outputs on the host, per group.
constexpr size_t LOO_CHUNK_DEFAULT = (size_t)1 << 30;      // device bytes of one chunk's scratch when chunk_bytes == 0
struct LooDraws {
    Problem *prob;
    const double *draws;            // device [G * S][D], unconstrained
    const int *spec;                // host [G]: the spectrum the units of each group were sampled against
    int G, chains, n_draws;
    int pair, col0, ncols;          // pair: real and imaginary part of a frequency are one unit (the full range only)
    int reff_mode;                  // 0: 1; 1: reff_in [G][units]; 2: n_eff / S of exp(ll - max ll) per unit
    const double *reff_in;
    size_t chunk_bytes;             // 0: LOO_CHUNK_DEFAULT
    hipStream_t stream;             // idle when the call starts; every launch goes here
};
size_t loo_draws_group_bytes(const LooDraws &j, bool predict);       // what one group adds to a chunk's scratch
int loo_of_draws(const LooDraws &j, double *lpd, double *elpd_loo, double *pareto_k, double *p_waic, int *n_tail, double *reff_out);
int loo_predict_of_draws(const LooDraws &j, double *mean, double *sd, double *pit, double *mean_post, double *sd_post,
                         double *pit_post, double *pareto_k, int *n_tail, double *reff_out);

// Prediction at held-out frequencies and its equal-weight reduction (bdrt_heldout.hip).  The device-pointer cores enqueue on
// `stream` and return.  dPar [B][D] constrained parameters, dW [H] = 2 pi f, dA per block [2H][K_b] (real rows, then imaginary
// rows), block after block -> dZh, dSg [B][2H]; -2 for an outlier error model (unless allow_outliers: dSg is then the base scale,
// sigma_tot without sigma_out, which bdrt_heldout_mix.hip integrates over its prior) or a grid beyond the LDS of a CU
int heldout_transformed_device(const char *who, Problem &P, const double *dPar, size_t B, const double *dW, const double *dA, int H,
                               double *dZh, double *dSg, hipStream_t stream, bool allow_outliers);
// dTm, dTs [G][N2][S] (transposed Z_hat, sigma_tot), dz [G][N2] -> dOut: 3 planes of G N2 (mean, sd, pit), then lpd [G U]
int heldout_reduce_device(const double *dTm, const double *dTs, const double *dz, int G, int S, int N2, int pair, double *dOut,
                          hipStream_t stream);
// -1 and the error text (in the name of `who`) unless the H held-out frequencies are positive finite numbers
int heldout_check_grid(const char *who, const double *freq, int H);
// both on a sampler's draws in chunks of groups: j as for loo_of_draws with pair, col0, ncols counted in the 2H held-out columns
// (reff_* unused); freq [H], A (as dA) and z_test [G][2H] on the host; outputs on the host, lpd [G][U], the others [G][ncols]
int heldout_of_draws(const LooDraws &j, const double *freq, int H, const double *A, const double *z_test, double *lpd, double *mean,
                     double *sd, double *pit);
// host copies of the held-out grid -> device: w = 2 pi f [H] and the packed prediction rows
int heldout_upload_grid(const Problem &P, const double *freq, int H, const double *A, DevBuf<double> &dW, DevBuf<double> &dA);
// heldout_of_draws with the reduction of a chunk left to the caller: reduce(dTm, dTs [gn][ncols][S], dz [gn][ncols], gn, S, dOut)
// enqueues on j.stream what fills dOut with 3 planes of gn ncols (mean, sd, pit), then lpd [gn U]; who: the name in error texts
using HeldoutReduceFn = std::function<int(const double *, const double *, const double *, int, int, double *)>;
int heldout_of_draws_with(const char *who, const LooDraws &j, const double *freq, int H, const double *A, const double *z_test,
                          bool allow_outliers, const HeldoutReduceFn &reduce, double *lpd, double *mean, double *sd, double *pit);
// the same under an outlier error model (bdrt_heldout_mix.hip): sigma_out integrated over its prior, the table y, w [Q] with
// second moment ey2 on the host; shared: the two scalars of a frequency have one sigma_out
int heldout_mix_of_draws(const LooDraws &j, const double *freq, int H, const double *A, const double *z_test, int shared,
                         const double *y, const double *w, int Q, double ey2, double *lpd, double *mean, double *sd, double *pit);

// Power-scaling sensitivity (bdrt_powerscale.hip) of draws that are on the device, in chunks of groups: j as for loo_of_draws with
// pair = 0 and reff_mode = 0; every row is evaluated against its group's spectrum.  Outputs on the host: cjs2 [G][D][4] (per
// constrained parameter: prior lower, prior upper, likelihood lower, likelihood upper), pareto_k, n_tail [G][4], and the two
// components L_out [G][2][S] (optional); who: the name in error texts
int powerscale_of_draws(const char *who, const LooDraws &j, double alpha_lo, double alpha_hi, double *cjs2, double *pareto_k,
                        int *n_tail, double *L_out);

// rank-normalised diagnostics (bdrt_rank.hip) of the same layout of DEVICE draws, on the split chains; outputs [G x C] on the host
int rank_diagnostics_to_host(const double *dX, long unit_stride, long row_stride, const unsigned char *is_pos, int G, int M,
                             int N, int C, double p_lo, double p_hi, double *rhat, double *ess_bulk, double *ess_tail,
                             double *ess_mean, double *sd, hipStream_t stream);

// Levenberg-Marquardt Newton polish of n_fits points on the device (bdrt_newton.hip); x0 / x_out [n_fits][D], rep [n_fits] on the host
struct NewtonReport { double lp, grad_inf; int iters, rc, n_evals; };
int newton_polish_device(Problem &P, const double *x0, const int *spec, int n_fits, int max_iter, double tol, double *x_out, NewtonReport *rep);

// the dynamic LDS of the kernels around the box-QP solver (bdrt_qp.hip: bdrt_qp_box_batch, bdrt_ridge_ex, bdrt_debug_qp_factor_solve)
// for n unknowns and `extra` doubles of the kernel's own: whether the packed KKT triangle lives in LDS (else in a global work
// buffer), the bytes to ask for, and whether the launch is possible at all
struct QpLds {
    bool in_lds, fits;
    size_t bytes;
};
QpLds qp_lds_plan(int n, size_t extra);

}  // namespace bdrt

struct bdrt_problem {
    bdrt::Problem impl;
};
