// bdrt_newton.hip -- second-order MAP polish on the device (the state machine of bdrt_newton.h, which remains as the
// host form the tests drive with oracle evaluations).
//
// Round 1 kept this iteration on the host: every Levenberg-Marquardt step copied the 2 D probe gradients (1.75 MB at
// D = 331) over PCIe and factored the D x D Hessian with a scalar Cholesky on one host core -- ~6 ms per step, ~3 s per fit,
// no faster than the reference's CPU.  Here nothing but a 64-byte status record leaves the GPU:
//   Hessian     single series distribution (the headline family): CLOSED FORM, bdrt_newton_hess.h -- newton_hess_prep_kernel (one
//               workgroup per fit) + newton_hess_fill_kernel (16 rows per workgroup; the dense A^T C A product, bands, borders); four
//               gradient evaluations per round (the trial points) instead of 2 D + 4.  Once the damping is below 1e-4 the coefficients
//               of a Series_pos fit are iterated on the linear scale with a floor (projected Newton): 105 rounds instead of 250 at K = 161.
//               Every other family: central differences -- probes x +- h_j e_j (newton_probe_kernel), the batched MFMA log-posterior
//               kernel on the 2 D probes (launch_logp_grad), H symmetrised by newton_build_kernel.  BDRT_NEWTON_FD=1 forces this path.
//   step        (-H + lam I) = L L^T by a blocked right-looking Cholesky (16 x 16 diagonal blocks in registers, panel solves one row
//               per thread, trailing update on v_mfma_f64_16x16x4 tiles); s = (L L^T)^-1 g; trial point; predicted increase
//                                                                            newton_solve_kernel   (one workgroup per fit)
//   trial       log-posterior + gradient at x + s, x + s/2, x + s/4, x + s/8   launch_logp_grad
//   decision    accept / reject, lam update, convergence                     newton_accept_kernel
// The host only sequences these launches and reads the status records; fits of a batch advance together.  Its pieces, after the kernels:
// NewtonEnv (the switches, read once per call), NewtonWork (every device buffer, the NewtonBufs the kernels take, the LDS limits, the host
// synchronisation), group_length, enqueue_round (the launches of one round) and newton_polish_device, which puts them in order.  The debug
// entries at the end (bdrt_debug_hessian(_lin), bdrt_debug_newton_solve / _accept) fill a NewtonWork with what their launches touch.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <cstdio>

#include "bdrt_host.h"
#include "bdrt_newton_hess.h"

namespace bdrt {

constexpr int NW_NT = 512;
constexpr int NW_ATT = 6;           // dampings lam, 4 lam, ... 4^5 lam factored side by side when the machine has room (newton_solve_kernel)
constexpr int NW_TRY = 4;           // step lengths tried per factorisation: s, s/2, s/4, s/8 -- one batched evaluation

struct NewtonState {            // one per fit, in device memory
    double lp, lam, pred, lp_trial, grad_inf;
    double gs, ss;              // g.s and s.s of the current step: predicted increase of t s is  t g.s + t^2/2 (lam s.s - g.s)
    int iters, rc, done, need_hess, n_evals, max_iter, hbad, lin;       // hbad: non-finite Hessian entry seen by the build kernel; lin: coefficients on the linear scale (bdrt_newton_hess.h)
    double tol;
};

// what one factorisation attempt of a launch leaves for the gather kernel (up to NW_ATT attempts per fit when the launch speculates, see newton_solve_kernel)
struct NewtonAttempt { double pred, gs, ss, lam; int ok, pad; };

struct NewtonBufs {
    int D, Dp;                  // Dp = D rounded up to 16
    double *x, *g, *gt, *hstep;            // [n_fits][D]
    double *s, *xt;             // [n_fits][NW_ATT][D]: step and trial point of each attempt
    double *H, *M;              // [n_fits][Dp][Dp]
    double *M2;                 // [n_fits][NW_ATT - 1][Dp][Dp]: the speculative attempts' matrices (nullptr: never more than one attempt)
    NewtonAttempt *att;         // [n_fits][NW_ATT]
    double *probes, *pgrad;     // [n_fits][2 D][D]
    double *plp;                // [n_fits][2 D]
    NewtonState *st;            // [n_fits]
    long long *prof;            // BDRT_NEWTON_PROF=1: cycle counters of the solve kernel's phases (nullptr otherwise)
    // closed-form Hessian (bdrt_newton_hess.h; single series distribution): no probes, no probe gradients
    int analytic;
    double *hws;                // [n_fits][HessLayout::total]
    int hl_total, hl_tz, hl_act, hl_floor, o_x, Kx, lin_ok;   // layout offsets the solve / gather kernels need; lin_ok: Series_pos (the linear scale applies)
    const int *fspec;           // [n_fits] spectrum of each fit
    const DevProblem *dP;
};

// phase counters: thread 0 of workgroup 0 adds the core-clock cycles since the previous mark to slot k
struct NewtonProf {
    long long *p, t;
    __device__ NewtonProf(long long *p_) : p(blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 ? p_ : nullptr), t(0) { if (p) t = clock64(); }
    __device__ void mark(int k) { if (p) { const long long n = clock64(); p[k] += n - t; t = n; } }
};
enum { NP_HESS = 0, NP_BUILD, NP_DIAG, NP_PANEL, NP_TRAIL, NP_SOLVE, NP_PRED, NP_WALL, NP_CALLS, NP_ATTEMPTS /* factorisations started */, NP_PREP0 = 16 /* .. 24: stages of hess_prep */, NP_FILL0 = 32 /* .. 34: stages of hess_fill */, NP_COUNT = 40 };

__global__ void newton_probe_kernel(NewtonBufs b, const int *active, int n_active)
{
    const int a = blockIdx.y, row = blockIdx.x;          // row in [0, 2 D)
    if (a >= n_active) return;
    const int f = active[a], D = b.D, j = row >> 1;
    if (b.st[f].done || !b.st[f].need_hess) return;      // (rejected trial: same Hessian; the probe rows keep whatever they hold)
    const double *x = b.x + (size_t)f * D;
    double *p = b.probes + ((size_t)a * 2 * D + row) * D;
    const double h = 1e-5 * fmax(1.0, fabs(x[j]));
    if (threadIdx.x == 0 && (row & 1) == 0) b.hstep[(size_t)f * D + j] = h;
    for (int k = threadIdx.x; k < D; k += blockDim.x) p[k] = x[k] + (k == j ? ((row & 1) ? -h : h) : 0.0);
}

__device__ __forceinline__ double bcast_lane(double v, int l)        // value of lane l (l uniform), as a scalar operand
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// In-place blocked Cholesky of the lower triangle of the Dp x Dp row-major matrix M (Dp a multiple of 16).  The forward
// substitution L y = v of a right-hand side v [Dp] (LDS) rides along: block J of y from the freshly factored diagonal
// block while it is in registers, the rows below from the panel while it is in LDS -- v holds y on return.
// lds: 16*17 (diagonal block) + 16 (reciprocal pivots) + Dp*17 (panel) + 1 (flag) doubles.  Returns false when not positive definite.
__device__ inline bool chol_blocked(double *M, int Dp, double *lds, NewtonProf &pf, double *v)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *Dg = lds, *rinv = Dg + 16 * 17, *Pn = rinv + 16;
    int *bad = reinterpret_cast<int *>(Pn + (size_t)Dp * 17);
    const int nblk = Dp / 16;
    if (tid == 0) *bad = 0;
    // Factor the 16 x 16 diagonal block that sits in Dg (row-major, stride 17) by the 16 rows' lanes of ONE wave, and the block J of the
    // forward substitution with it.  Lane i keeps row i of the block in registers; column j of the factor is read out of the lanes that
    // own it (v_readlane -> SGPR operand of the multiply-add): no LDS round trips, no branches inside the 16 steps; a non-positive pivot
    // poisons the block with NaNs and is reported after the last step.
    auto factor_diag = [&](int j0) {
        const int i = lane & 15;
        double row[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = Dg[i * 17 + k];
        bool okb = true;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const double d = bcast_lane(row[j], j);
            okb = okb && d > 0.0 && isfinite(d);
            double rs = __builtin_amdgcn_rsq(d);                      // 1 / sqrt(d): hardware estimate + two Newton steps
            rs = rs * (1.5 - 0.5 * d * rs * rs);
            rs = rs * (1.5 - 0.5 * d * rs * rs);
            const double lij = i == j ? d * rs : row[j] * rs;
            row[j] = lij;
#pragma unroll
            for (int k = j + 1; k < 16; ++k) {
                const double lkj = bcast_lane(lij, k);                // L[k][j], held by lane k
                row[k] -= (i > j && k <= i) ? lij * lkj : 0.0;
            }
        }
        if (!okb) { if (lane == 0) *bad = 1; }
        else {
            // y_J = L11^-1 v_J: lane i holds row i of L11; y_k is broadcast as soon as it is known
            const double rd = 1.0 / row[i];
            double t = v[j0 + i];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const double c = t * rd;
                const double yk = bcast_lane(c, k);
                if (i > k) t -= row[k] * yk;
                if (i == k) t = yk * row[i];                          // keeps t / L[i][i] = y_i for the store below
            }
            if (lane < 16) {
#pragma unroll
                for (int k = 0; k < 16; ++k) Dg[i * 17 + k] = row[k];
                rinv[i] = rd;
                v[j0 + i] = t * rd;
            }
        }
    };
    // block 0: from global memory; every later diagonal block is produced by the step before it (look-ahead, below)
    if (tid < 256) Dg[(tid >> 4) * 17 + (tid & 15)] = M[(size_t)(tid >> 4) * Dp + (tid & 15)];
    __syncthreads();
    if (wave == 0) factor_diag(0);
    __syncthreads();
    pf.mark(NP_DIAG);
    for (int J = 0; J < nblk; ++J) {
        const int j0 = 16 * J;
        if (*bad) return false;
        if (tid < 256 && (tid & 15) <= (tid >> 4)) M[(size_t)(j0 + (tid >> 4)) * Dp + j0 + (tid & 15)] = Dg[(tid >> 4) * 17 + (tid & 15)];
        // (b) panel below the block: x L11^T = a, one row per thread.  The m x 16 panel moves between global memory and
        // LDS with coalesced accesses (16 lanes per 128-byte row segment); the solve itself works on the LDS copy.
        const int m = Dp - j0 - 16;
        if (m == 0) break;
        {
            const double *src = M + (size_t)(j0 + 16 + (tid >> 4)) * Dp + j0 + (tid & 15);
            double *dst = Pn + (tid >> 4) * 17 + (tid & 15);
            const int nrow = NW_NT / 16;                                  // rows per pass
            int r = tid >> 4;
            for (; r + 3 * nrow < m; r += 4 * nrow) {                    // four row-passes per trip: the loads overlap
                const double v0 = src[0], v1 = src[(size_t)nrow * Dp], v2 = src[(size_t)2 * nrow * Dp], v3 = src[(size_t)3 * nrow * Dp];
                dst[0] = v0; dst[nrow * 17] = v1; dst[2 * nrow * 17] = v2; dst[3 * nrow * 17] = v3;
                src += (size_t)4 * nrow * Dp; dst += 4 * nrow * 17;
            }
            for (; r < m; r += nrow) { dst[0] = src[0]; src += (size_t)nrow * Dp; dst += nrow * 17; }
        }
        __syncthreads();
        for (int r = tid; r < m; r += NW_NT) {
            double *row = Pn + (size_t)r * 17;
            double xk[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) xk[k] = row[k];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                double t = xk[k];
#pragma unroll
                for (int u = 0; u < k; ++u) t -= xk[u] * Dg[k * 17 + u];
                xk[k] = t * rinv[k];
                __builtin_amdgcn_sched_barrier(0);        // one row of L11 at a time: hoisting all 120 LDS operands costs 240 VGPRs
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) row[k] = xk[k];
            double dotv = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) dotv += xk[k] * v[j0 + k];
            v[j0 + 16 + r] -= dotv;
        }
        __syncthreads();
        for (int e = tid; e < m * 16; e += NW_NT) M[(size_t)(j0 + 16 + (e >> 4)) * Dp + j0 + (e & 15)] = Pn[(size_t)(e >> 4) * 17 + (e & 15)];
        pf.mark(NP_PANEL);
        // (c) trailing update C -= P P^T on 16 x 16 tiles of the lower triangle (tiles on the diagonal are computed in full).
        // Look-ahead: tile 0 is the next diagonal block -- wave 0 updates it into Dg (the panel above was the last reader of this
        // step's factor) and factors it at once, while the other seven waves update the rest of the trailing matrix: the 16
        // sequential steps of the diagonal block (8 k cycles, a quarter of the routine at D = 331) run in the shadow of the update.
        const int mb = m / 16, ntile = mb * (mb + 1) / 2;
        const int col = lane & 15, kq = lane >> 4;
        auto tile_of = [&](int t, int &I, int &Jc) {
            I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
            while ((I + 1) * (I + 2) / 2 <= t) ++I;
            while (I * (I + 1) / 2 > t) --I;
            Jc = t - I * (I + 1) / 2;
        };
        constexpr int NWV = NW_NT / 64, TPT = 4;
        if (wave == 0) {
            const double *C = M + (size_t)(j0 + 16 + kq) * Dp + j0 + 16 + col;
            d4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = C[(size_t)(4 * r) * Dp];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = mfma_f64(-Pn[(size_t)col * 17 + 4 * u + kq], Pn[(size_t)col * 17 + 4 * u + kq], acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) Dg[(kq + 4 * r) * 17 + col] = acc[r];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            factor_diag(j0 + 16);
        } else {
            // four tiles per trip and wavefront: the global loads of all four are in flight before the first MFMA issues.
            // (Measured and dropped: six or eight tiles per trip -- 270 -> 290 / 317 us per launch at D = 331 --; two trips in flight,
            // the next one's loads requested before this one's MFMAs -- the registers it takes slow the panel and the substitutions
            // by more than the update gains: 270 -> 326 us.)
            for (int t = wave; t < ntile; t += TPT * (NWV - 1)) {
                double *C[TPT];
                int Ib[TPT], Jb[TPT];
                d4 acc[TPT];
#pragma unroll
                for (int q = 0; q < TPT; ++q) {
                    const int tq = t + q * (NWV - 1);
                    tile_of(tq < ntile ? tq : t, Ib[q], Jb[q]);
                    C[q] = M + (size_t)(j0 + 16 + 16 * Ib[q] + kq) * Dp + j0 + 16 + 16 * Jb[q] + col;
                }
#pragma unroll
                for (int q = 0; q < TPT; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[q][r] = C[q][(size_t)(4 * r) * Dp];
#pragma unroll
                for (int q = 0; q < TPT; ++q)
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        acc[q] = mfma_f64(-Pn[(size_t)(16 * Ib[q] + col) * 17 + 4 * u + kq], Pn[(size_t)(16 * Jb[q] + col) * 17 + 4 * u + kq], acc[q]);
#pragma unroll
                for (int q = 0; q < TPT; ++q)
                    if (q == 0 || t + q * (NWV - 1) < ntile) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) C[q][(size_t)(4 * r) * Dp] = acc[q][r];
                    }
            }
        }
        __syncthreads();
        pf.mark(NP_TRAIL);
    }
    return true;
}

__device__ __forceinline__ double sum16(double t)                  // sum over each aligned group of 16 lanes (valid in the group's lane 0)
{
    t += dpp_perm<0xB1>(t); t += dpp_perm<0x4E>(t); t += dpp_perm<0x141>(t); t += dpp_perm<0x140>(t);
    return t;
}

// v <- L^-T v (the forward substitution was done by chol_blocked), L = lower triangle of the row-major Dp x Dp matrix M
// (Dp a multiple of 16, identity on the padding); v [Dp] in LDS; Dg: 16*17 doubles of LDS scratch.  Blocked substitution:
// the 16 x 16 diagonal block by one wave with the block's columns in registers, the rest of the right-hand side is updated
// by the whole workgroup with coalesced row reads.
__device__ inline void chol_blocked_solve(const double *M, int Dp, double *v, double *Dg)
{
    const int tid = threadIdx.x;
    const int nblk = Dp / 16;
    for (int J = nblk - 1; J >= 0; --J) {                             // backward: L^T x = y
        const int j0 = 16 * J;
        if (tid < 256) Dg[(tid >> 4) * 17 + (tid & 15)] = M[(size_t)(j0 + (tid >> 4)) * Dp + j0 + (tid & 15)];
        __syncthreads();
        if (tid < 64) {
            // lane j holds column j of the block (row j of L^T); x_k broadcast from the last unknown upwards
            const int j = tid & 15;
            double Lc[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) Lc[k] = Dg[k * 17 + j];
            const double rd = 1.0 / Lc[j];
            double t = v[j0 + j];
#pragma unroll
            for (int k = 15; k >= 0; --k) {
                const double c = t * rd;
                const double xk = bcast_lane(c, k);
                if (j < k) t -= Lc[k] * xk;
                if (j == k) t = xk * Lc[j];
            }
            if (tid < 16) v[j0 + j] = t * rd;
        }
        __syncthreads();
        // columns to the left: v_k -= sum_i L[j0 + i][k] x_{j0 + i}  -- one k per thread, coalesced along k
        for (int k = tid; k < j0; k += NW_NT) {
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) t += M[(size_t)(j0 + i) * Dp + k] * v[j0 + i];
            v[k] -= t;
        }
        __syncthreads();
    }
}

// H (symmetrised central differences of the probe gradients, when the fit asked for a fresh Hessian) and the damped
// matrix M = -H + lam I of every active fit: 16 rows of one fit per workgroup, so the 2 D^2 probe gradients are read at
// the whole chip's bandwidth instead of one CU's load latency (the solve kernel spent 0.4 M of its 1.9 M cycles here at D = 331).
__global__ __launch_bounds__(256) void newton_build_kernel(NewtonBufs b, const int *active, int n_active)
{
    const int a = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f = active[a], D = b.D, Dp = b.Dp;
    NewtonState &S = b.st[f];
    if (S.done) return;
    double *H = b.H + (size_t)f * Dp * Dp, *M = b.M + (size_t)f * Dp * Dp;
    const double lam = S.lam;
    const int r0 = 16 * blockIdx.x;
    if (S.need_hess) {
        // (probe slot a = position in the active list)
        const double *pg = b.pgrad + (size_t)a * 2 * D * D, *hs = b.hstep + (size_t)f * D;
        int bad = 0;
        for (int i = r0 + wv; i < r0 + 16; i += 4) {
            if (i >= D) {
                for (int k = lane; k < Dp; k += 64) M[(size_t)i * Dp + k] = i == k ? 1.0 : 0.0;
                continue;
            }
            const double ri = 0.5 / hs[i];
            for (int k = lane; k < Dp; k += 64) {
                double m = 0.0;
                if (k < D) {
                    const double hik = (pg[(size_t)(2 * i) * D + k] - pg[(size_t)(2 * i + 1) * D + k]) * ri;
                    const double hki = (pg[(size_t)(2 * k) * D + i] - pg[(size_t)(2 * k + 1) * D + i]) * (0.5 / hs[k]);
                    const double h = 0.5 * (hik + hki);
                    if (!isfinite(h)) bad = 1;
                    H[(size_t)i * Dp + k] = h;
                    m = -h + (i == k ? lam : 0.0);
                }
                M[(size_t)i * Dp + k] = m;
            }
        }
        if (__syncthreads_or(bad) && tid == 0) atomicOr(&S.hbad, 1);
    } else {
        for (int i = r0 + wv; i < r0 + 16; i += 4)
            for (int k = lane; k < Dp; k += 64) {
                double m = i == k ? 1.0 : 0.0;
                if (i < D && k < D) m = -H[(size_t)i * Dp + k] + (i == k ? lam : 0.0);
                M[(size_t)i * Dp + k] = m;
            }
    }
}

// The closed-form Hessian (bdrt_newton_hess.h) in place of probes + evaluator + newton_build_kernel: forward quantities and border
// vectors per fit, then H and M = -H + lam I in tiles of 16 rows.  A fit that keeps its Hessian (rejected trial) only gets M again.
__global__ __launch_bounds__(HP_NT) void newton_hess_prep_kernel(NewtonBufs b, const int *active, int n_active)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int f = active[blockIdx.x];
    NewtonState &S = b.st[f];
    if (S.done || !S.need_hess) return;
    // the switch to the linear scale of the coefficients: once, when the damping has dropped to 1e-4 (every later kernel of the round
    // reads the flag this kernel leaves)
    const int lin = (b.lin_ok && (S.lin || S.lam <= 1e-4)) ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) S.lin = lin;
    HessArgs ha{b.dP, b.x, b.g, b.fspec, b.hws, b.H, b.M, b.D, b.Dp, lin, b.prof};
    const long long w0 = (b.prof && blockIdx.x == 0 && threadIdx.x == 0) ? wall_clock64() : 0;
    hess_prep(ha, f, sh);
    if (b.prof && blockIdx.x == 0 && threadIdx.x == 0) b.prof[NP_PREP0 + 9] += wall_clock64() - w0;
}
__global__ __launch_bounds__(HP_NT) void newton_hess_fill_kernel(NewtonBufs b, const int *active, int n_active)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int f = active[blockIdx.y], tid = threadIdx.x, D = b.D, Dp = b.Dp;
    NewtonState &S = b.st[f];
    if (S.done) return;
    const int r0 = 16 * blockIdx.x;
    if (S.need_hess) {
        HessArgs ha{b.dP, b.x, b.g, b.fspec, b.hws, b.H, b.M, b.D, b.Dp, S.lin, b.prof};
        const bool bad = hess_fill(ha, f, r0, S.lam, sh);
        if (__syncthreads_or(bad ? 1 : 0) && tid == 0) atomicOr(&S.hbad, 1);
    } else {
        const double *H = b.H + (size_t)f * Dp * Dp;
        double *M = b.M + (size_t)f * Dp * Dp;
        const double lam = S.lam;
        for (int i = r0 + (tid >> 6); i < r0 + 16; i += HP_NT / 64)
            for (int k = tid & 63; k < Dp; k += 64) {
                double m = i == k ? 1.0 : 0.0;
                if (i < D && k < D) m = -H[(size_t)i * Dp + k] + (i == k ? lam : 0.0);
                M[(size_t)i * Dp + k] = m;
            }
    }
}

// One Levenberg-Marquardt step per active fit: the damped solve and the trial point.
// natt > 1 (natt workgroups per fit, blockIdx.y = attempt): four factorisations in ten at K = 161 find -H + lam I indefinite, and the
// next one with 4 lam is another 250 us on the one workgroup -- up to five in a row where the damping has to grow by orders of magnitude
// (the longest launches took 1.4 ms).  When the machine has room (natt workgroups per active fit <= CUs) attempt j factors
// -H + 4^j lam I at the same time on a CU of its own (its matrix built from H; the last attempt goes on to higher dampings by itself if
// it must), each once; the gather kernel takes the first attempt that succeeded: the same sequence of dampings and the same numbers as
// the one-workgroup loop, the failed factorisations off the critical path.  With natt = 1 attempt 0 runs the whole loop.
// The kernel only reads the fit's state; the gather kernel commits the chosen attempt.
__global__ __launch_bounds__(NW_NT) void newton_solve_kernel(NewtonBufs b, const int *active, int n_active, int natt)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int a = blockIdx.x, att = blockIdx.y, tid = threadIdx.x;
    const int f = active[a], D = b.D, Dp = b.Dp;
    const NewtonState &S = b.st[f];
    if (S.done) return;
    NewtonAttempt &A = b.att[NW_ATT * f + att];
    const double *H = b.H + (size_t)f * Dp * Dp;
    double *M = att ? b.M2 + ((size_t)f * (NW_ATT - 1) + (att - 1)) * Dp * Dp : b.M + (size_t)f * Dp * Dp;
    const double *x = b.x + (size_t)f * D, *g = b.g + (size_t)f * D;
    double *s = b.s + ((size_t)f * NW_ATT + att) * D, *xt = b.xt + ((size_t)f * NW_ATT + att) * D;
    const bool lin = b.analytic && S.lin;
    const double *hw = b.analytic ? b.hws + (size_t)f * b.hl_total : nullptr;
    double *v = sh;                               // [Dp] right-hand side / solution
    double *red = v + Dp;                         // 64 doubles
    double *cl = red + 64;                        // Cholesky scratch
    __shared__ int s_fin;
    NewtonProf pf(b.prof);
    const long long wall0 = b.prof ? wall_clock64() : 0;
    // H (when new probe gradients arrived) and M = -H + lam I were written by the build / fill kernel
    if (S.need_hess && S.hbad) { if (tid == 0) { A.ok = 0; A.lam = S.lam; } return; }       // (the gather kernel reports it)
    pf.mark(NP_HESS);
    double lam = S.lam;
    bool ok = false, rebuilt = true;
    if (att) { lam *= ldexp(1.0, 2 * att); rebuilt = false; }
    while (lam <= 1e12) {
        if (!rebuilt) {
            // more damping after a failed factorisation (or the speculative attempt's first matrix): M again from H -- the lower block
            // triangle only (what chol_blocked reads: diagonal tiles in full), four rows of a wave's column slice in flight at a time
            // (one dependent load per row was 160 k cycles per rebuild)
            const int wv = tid >> 6, ln = tid & 63;
            for (int i0 = 4 * wv; i0 < Dp; i0 += 4 * (NW_NT / 64)) {
                const int kend = ((i0 + 3) | 15) + 1;               // columns up to the end of the rows' diagonal tile
                for (int k = ln; k < kend; k += 64) {
                    double h[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const int i = i0 + r; h[r] = (i < D && k < D) ? H[(size_t)i * Dp + k] : 0.0; }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = i0 + r;
                        double m = i == k ? 1.0 : 0.0;             // identity on the padding
                        if (i < D && k < D) m = -h[r] + (i == k ? lam : 0.0);
                        M[(size_t)i * Dp + k] = m;
                    }
                }
            }
            __syncthreads();
        }
        rebuilt = false;
        pf.mark(NP_BUILD);
        // right-hand side: the gradient in the iteration's coordinates (g_z = g_y dy/dz; zero for a coefficient held at its floor)
        for (int i = tid; i < Dp; i += NW_NT) {
            double gi = i < D ? g[i] : 0.0;
            if (lin && i < D) gi = hw[b.hl_act + i] != 0.0 ? 0.0 : gi * hw[b.hl_tz + i];
            v[i] = gi;
        }
        __syncthreads();
        if (pf.p) pf.p[NP_ATTEMPTS] += 1;
        if (chol_blocked(M, Dp, cl, pf, v)) {
            chol_blocked_solve(M, Dp, v, cl);
            pf.mark(NP_SOLVE);
            int fin = 1;
            for (int i = tid; i < D; i += NW_NT) {
                const double t = x[i] + v[i];              // (finite here is finite on either scale)
                if (!isfinite(t)) fin = 0;
            }
            if (tid == 0) s_fin = 1;
            __syncthreads();
            if (!fin) s_fin = 0;
            __syncthreads();
            if (s_fin) { ok = true; break; }
        }
        if (att + 1 < natt) break;                         // (the next damping is another workgroup's)
        lam *= 4.0;
        __syncthreads();
    }
    if (!ok) { if (tid == 0) { A.ok = 0; A.lam = lam; } return; }
    // trial point and the model's predicted increase g.s + 1/2 s^T H s.  With (-H + lam I) s = g this is
    // 1/2 (g.s + lam s.s): no product with H is needed (the difference is the residual of the backward-stable solve).
    double gs = 0.0, ss = 0.0;
    for (int i = tid; i < D; i += NW_NT) {
        const double si = v[i];
        double gi = g[i], xn = x[i] + si;
        if (lin) {
            gi = hw[b.hl_act + i] != 0.0 ? 0.0 : gi * hw[b.hl_tz + i];
            if (i >= b.o_x && i < b.o_x + b.Kx) xn = log(fmax(exp(x[i]) + si, hw[b.hl_floor]));     // projected step on the linear scale
        }
        s[i] = si; xt[i] = xn; gs += gi * si; ss += si * si;
    }
    const int lane = tid & 63, wave = tid >> 6;
    gs = sum32(gs); gs += __shfl_xor(gs, 32);
    ss = sum32(ss); ss += __shfl_xor(ss, 32);
    if (lane == 0) { red[wave] = gs; red[NW_NT / 64 + wave] = ss; }
    __syncthreads();
    if (tid == 0) {
        double p = 0.0, q = 0.0;
        for (int w = 0; w < NW_NT / 64; ++w) { p += red[w]; q += red[NW_NT / 64 + w]; }
        A.pred = 0.5 * (p + lam * q); A.lam = lam;
        A.gs = p; A.ss = q; A.ok = 1;
    }
    pf.mark(NP_PRED);
    if (pf.p) { pf.p[NP_WALL] += wall_clock64() - wall0; pf.p[NP_CALLS] += 1; }
}

// consume the trial evaluations (lp_t, gradients gt; rows NW_TRY a + t): the longest of the step lengths s, s/2, s/4, s/8 that
// passes the sufficient-increase test is accepted (bdrt_newton.h NewtonFit::consume, NEED_TRIAL, is the t = 0 case; the
// shorter steps along the same Levenberg-Marquardt direction cost one batched evaluation instead of a re-factorisation
// with more damping -- 40 % of the solves at K = 161 were such re-factorisations)
template <int NT>
__device__ __forceinline__ void newton_accept_body(const NewtonBufs &b, int f, int a, const double *lp_t, const double *trial)
{
    const int tid = threadIdx.x;
    const int D = b.D;
    NewtonState &S = b.st[f];
    __shared__ double red[NT];
    __shared__ int s_acc, s_t;
    double *x = b.x + (size_t)f * D, *g = b.g + (size_t)f * D;
    if (tid == 0) { s_acc = 0; s_t = 0; S.n_evals += NW_TRY; }
    __syncthreads();
    const bool lin = b.analytic && S.lin;
    const double floor_x = lin ? b.hws[(size_t)f * b.hl_total + b.hl_floor] : 0.0;
    for (int t = 0; t < NW_TRY; ++t) {
        const double *gt = b.gt + ((size_t)a * NW_TRY + t) * D;
        const double *xs_t = trial + ((size_t)a * NW_TRY + t) * D;
        const double lpn = lp_t[a * NW_TRY + t];
        int fin = isfinite(lpn) ? 1 : 0;
        double gi = 0.0;
        for (int j = tid; j < D; j += NT) {
            double v = gt[j];
            if (!isfinite(v)) fin = 0;
            // a coefficient on the linear scale that sits at its floor passes |g_y| = x |g_x| < tol whatever g_x is: there the test is
            // the bound's own condition, g_x <= 0 (a positive g_x, scaled by the largest coefficient, counts as gradient)
            if (lin && j >= b.o_x && j < b.o_x + b.Kx) {
                const double xj = exp(xs_t[j]);
                if (xj <= 4.0 * floor_x && v > 0.0) v = v / xj * (1e14 * floor_x);
            }
            gi = fmax(gi, fabs(v));
        }
        fin = __syncthreads_and(fin);
        red[tid] = gi;
        __syncthreads();
        for (int w = NT / 2; w > 0; w >>= 1) { if (tid < w) red[tid] = fmax(red[tid], red[tid + w]); __syncthreads(); }
        const double ginf = red[0];
        if (tid == 0) {
            const double lp = S.lp, sc = ldexp(1.0, -t);
            // predicted increase of the scaled step: with (-H + lam I) s = g,  t g.s + t^2/2 s^T H s = t g.s + t^2/2 (lam s.s - g.s)
            const double pred = t == 0 ? S.pred : sc * S.gs + 0.5 * sc * sc * (S.lam * S.ss - S.gs);
            int acc = fin && (lpn - lp >= 1e-4 * pred) && (lpn >= lp - 1e-12 * fabs(lp));
            // close to the optimum the predicted increase drops below the resolution of lp itself (a few ulp of |lp|): the
            // sufficient-increase test then compares rounding noise.  There the step is judged by what it is meant to do --
            // reduce the gradient -- as long as lp does not visibly decrease.
            const double noise = 64.0 * 2.220446049250313e-16 * fmax(1.0, fabs(lp));
            if (fin && !acc && pred < noise && lpn >= lp - noise && ginf < S.grad_inf) acc = 1;
            if (t == 0) S.lp_trial = lpn;
            if (acc) {
                const double rho = pred > 0.0 ? (lpn - lp) / pred : 0.0;
                S.lp = lpn;
                if (t == 0) {
                    if (rho > 0.75) S.lam = fmax(S.lam / 5.0, 1e-12);
                    else if (rho < 0.25) S.lam *= 2.0;
                } else {
                    S.lam *= ldexp(1.0, t);                       // the full step was too long: more damping next time
                }
                S.iters += 1;
                S.grad_inf = ginf;
                if (ginf < S.tol) { S.rc = 0; S.done = 1; }
                else if (S.iters >= S.max_iter) { S.rc = 1; S.done = 1; }
                else S.need_hess = 1;
                s_acc = 1; s_t = t;
            }
        }
        __syncthreads();
        if (s_acc) break;
    }
    if (s_acc) {
        const double *xs = trial + ((size_t)a * NW_TRY + s_t) * D, *gt = b.gt + ((size_t)a * NW_TRY + s_t) * D;
        for (int j = tid; j < D; j += NT) { x[j] = xs[j]; g[j] = gt[j]; }
    } else if (tid == 0) {
        S.lam *= 16.0;                                            // none of the lengths: same Hessian, much more damping
    }
}

__global__ __launch_bounds__(256) void newton_accept_kernel(NewtonBufs b, const int *active, int n_active, const double *lp_t,
                                                            const double *trial)
{
    const int f = active[blockIdx.x];
    if (b.st[f].done) return;
    newton_accept_body<256>(b, f, blockIdx.x, lp_t, trial);
}

// closed-form Hessian: the verdict on the trial points and, for a fit that goes on with a new point, the forward quantities of the NEXT
// round's Hessian (newton_hess_prep_kernel) in one launch: as a launch of its own -- one or two workgroups between two short kernels --
// the prep kernel took 48 us of which 25 us are its work (kernel timeline of a K = 161 fit, profiles/r06/newton_timeline.txt).
__global__ __launch_bounds__(HP_NT) void newton_accept_prep_kernel(NewtonBufs b, const int *active, int n_active, const double *lp_t,
                                                                const double *trial)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const long long w0 = (b.prof && blockIdx.x == 0 && threadIdx.x == 0) ? wall_clock64() : 0;
    const int f = active[blockIdx.x];
    NewtonState &S = b.st[f];
    if (S.done) return;
    newton_accept_body<HP_NT>(b, f, blockIdx.x, lp_t, trial);
    __syncthreads();                                       // the verdict (thread 0) and the new point are visible to the workgroup
    if (S.done || !S.need_hess) return;
    const int lin = (b.lin_ok && (S.lin || S.lam <= 1e-4)) ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) S.lin = lin;
    HessArgs ha{b.dP, b.x, b.g, b.fspec, b.hws, b.H, b.M, b.D, b.Dp, lin, b.prof};
    hess_prep(ha, f, sh);
    if (b.prof) __syncthreads();                           // (profiling runs: the wall time of the whole workgroup, not of thread 0's wave)
    if (b.prof && blockIdx.x == 0 && threadIdx.x == 0) b.prof[NP_PREP0 + 9] += wall_clock64() - w0;
}

// dense batch of the active fits' trial points: rows NW_TRY a + t <- x + 2^-t s of fit active[a]
// (and the commit of the launch's solve: attempt 0 when it succeeded, else the speculative attempt 1 -- newton_solve_kernel)
__global__ void newton_gather_kernel(NewtonBufs b, const int *active, int n_active, double *dst, int natt)
{
    const int a = blockIdx.x, t = blockIdx.y;
    const int f = active[a];
    int c = 0;
    while (c + 1 < natt && !b.att[NW_ATT * f + c].ok) ++c;            // the first attempt that succeeded (the last one if none did)
    const double *x = b.x + (size_t)f * b.D, *sv = b.s + ((size_t)f * NW_ATT + c) * b.D, *xt = b.xt + ((size_t)f * NW_ATT + c) * b.D;
    if (t == 0 && threadIdx.x == 0) {
        NewtonState &S = b.st[f];
        if (!S.done) {
            const NewtonAttempt &A = b.att[NW_ATT * f + c];
            if (S.need_hess) {
                if (S.hbad) { S.rc = 2; S.done = 1; }
                else { S.need_hess = 0; S.n_evals += b.analytic ? 0 : 2 * b.D; }
            }
            if (!S.done) {
                if (A.ok) { S.pred = A.pred; S.lam = A.lam; S.gs = A.gs; S.ss = A.ss; }
                else { S.rc = 2; S.done = 1; S.lam = A.lam; }
            }
        }
    }
    const double sc = ldexp(1.0, -t);
    double *d = dst + ((size_t)a * NW_TRY + t) * b.D;
    const bool lin = b.analytic && b.st[f].lin;
    const double floor_x = lin ? b.hws[(size_t)f * b.hl_total + b.hl_floor] : 0.0;
    for (int k = threadIdx.x; k < b.D; k += blockDim.x) {
        double v = t == 0 ? xt[k] : x[k] + sc * sv[k];
        // a coefficient on the linear scale: the shortened step is shortened there, y = log(max(x + 2^-t s, floor))
        if (lin && t > 0 && k >= b.o_x && k < b.o_x + b.Kx) v = log(fmax(exp(x[k]) + sc * sv[k], floor_x));
        d[k] = v;
    }
}

// first evaluation at the start point: lp, g, convergence test
__global__ __launch_bounds__(256) void newton_init_kernel(NewtonBufs b, int n_fits, const double *lp0, const double *g0)
{
    const int f = blockIdx.x, tid = threadIdx.x, D = b.D;
    NewtonState &S = b.st[f];
    __shared__ double red[256];
    double *g = b.g + (size_t)f * D;
    int fin = isfinite(lp0[f]) ? 1 : 0;
    double gi = 0.0;
    for (int j = tid; j < D; j += 256) { const double v = g0[(size_t)f * D + j]; g[j] = v; if (!isfinite(v)) fin = 0; gi = fmax(gi, fabs(v)); }
    fin = __syncthreads_and(fin);
    red[tid] = gi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] = fmax(red[tid], red[tid + w]); __syncthreads(); }
    if (tid == 0) {
        S.lp = lp0[f]; S.n_evals = 1; S.grad_inf = red[0];
        if (!fin) { S.rc = -1; S.done = 1; }
        else if (red[0] < S.tol) { S.rc = 0; S.done = 1; }
        else S.need_hess = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// dynamic LDS of newton_solve_kernel: right-hand side, reduction scratch, chol_blocked's diagonal block, pivots, panel and flag
static size_t newton_solve_lds_bytes(int Dp)
{
    return ((size_t)Dp + 64 + 16 * 17 + 16 + (size_t)Dp * 17 + 2) * sizeof(double);
}

// The switches of the iteration (measurements: DESIGN 7b), read once per newton_polish_device call; the test entries read none.
struct NewtonEnv {
    bool spec = true;           // BDRT_NEWTON_SPEC=0: never more than one factorisation per launch
    bool fd = false;            // BDRT_NEWTON_FD=1: central differences of the gradient (as in rounds 1-5) where the model has a closed form, too
    bool linear = true;         // BDRT_NEWTON_LINEAR=0: the coefficients stay on the log scale for the whole iteration
    bool prof = false;          // BDRT_NEWTON_PROF=1: cycle counters of the kernels' phases and the host's times, on stderr
    bool trial_few = true;      // BDRT_NEWTON_TRIAL_FEW=0: the trial points through the tile evaluator (as before round 6)
    bool trace = false;         // BDRT_NEWTON_TRACE=1: the status records of the first eight fits at every host synchronisation, on stderr
    bool rounds_set = false;    // BDRT_NEWTON_ROUNDS=<n>: n rounds between host synchronisations, and no group twice as long (group_length)
    int rounds = 4;
};

static NewtonEnv read_newton_env()
{
    auto is = [](const char *name, char c) { const char *e = getenv(name); return e && e[0] == c; };
    NewtonEnv e;
    e.spec = !is("BDRT_NEWTON_SPEC", '0'); e.fd = is("BDRT_NEWTON_FD", '1'); e.linear = !is("BDRT_NEWTON_LINEAR", '0');
    e.prof = is("BDRT_NEWTON_PROF", '1'); e.trial_few = !is("BDRT_NEWTON_TRIAL_FEW", '0'); e.trace = is("BDRT_NEWTON_TRACE", '1');
    if (const char *r = getenv("BDRT_NEWTON_ROUNDS")) { e.rounds_set = true; e.rounds = std::max(1, atoi(r)); }
    return e;
}

// Every device buffer of the iteration, the NewtonBufs the kernels take, and the host's copies of the status records and lists.  The iteration
// sizes all of it (alloc); a test entry fills the few owners its launches touch.  bind() is the one place where NewtonBufs gets its pointers: an
// owner that was not allocated reads as nullptr (M2, pgrad, plp, hws, prof where the iteration does without them).
struct NewtonWork {
    NewtonBufs b;
    DevBuf<double> x, g, s, xt, gt, hstep, H, M, M2, probes, pgrad, plp, hws, lpt;
    DevBuf<NewtonAttempt> att;
    DevBuf<NewtonState> state;
    DevBuf<long long> prof;
    DevBuf<int> active, spec1, specp, fspec;
    size_t lds_prep = 0, lds_fill = 0, lds_solve = 0;      // dynamic LDS of hess_prep / accept_prep, hess_fill, solve
    // the host's side of a synchronisation (sync_active)
    std::vector<NewtonState> hst;
    std::vector<int> hspec, hact, hact_prev, hspecp, sp1;
    int n_active = 0;
    double g_far = 0.0;         // largest |g| of the active fits
    explicit NewtonWork(int D) { memset(&b, 0, sizeof(b)); b.D = D; b.Dp = (D + 15) & ~15; lds_solve = newton_solve_lds_bytes(b.Dp); }
    // the problem whose closed-form Hessian the kernels evaluate (analytic = 0: they difference gradients) and its workspace's layout
    void model(const Problem &P, int analytic, int lin_ok)
    {
        const int nf = P.dev.nf, K = P.dev.blk[0].K;
        const HessLayout hlay(nf, K);
        b.dP = (const DevProblem *)P.d_dev; b.analytic = analytic; b.lin_ok = lin_ok;
        b.hl_total = hlay.total; b.hl_tz = hlay.tz; b.hl_act = hlay.act; b.hl_floor = hlay.h0 + 11; b.o_x = P.dev.blk[0].o_x; b.Kx = K;
        lds_prep = analytic ? hess_prep_lds_doubles(nf, K) * sizeof(double) : 0;
        lds_fill = analytic ? hess_fill_lds_doubles(nf, K) * sizeof(double) : 0;
    }
    // The iteration's buffers for n fits, after model().  The sizing rules: M2, the matrices of the speculative factorisations
    // (newton_solve_kernel), only with speculation and while they stay below 2 GB (a 512-spectrum batch with them -- 2.3 GB of hipMalloc --
    // was 0.31 -> 0.38 s); closed form: probes holds only the NW_TRY trial points of a round, and there is the Hessian's workspace hws;
    // differences: probes holds the 2 D probes of a fit, pgrad and plp their gradients and log-posteriors; prof only when profiling.
    int alloc(size_t n, const NewtonEnv &env, hipStream_t stream)
    {
        const size_t D = b.D, nD = n * D, nM = n * b.Dp * b.Dp;
        BDRT_HIP(x.alloc(nD)); BDRT_HIP(g.alloc(nD)); BDRT_HIP(s.alloc(NW_ATT * nD));
        BDRT_HIP(xt.alloc(NW_ATT * nD)); BDRT_HIP(gt.alloc(nD * NW_TRY)); BDRT_HIP(hstep.alloc(nD));
        BDRT_HIP(att.alloc(n * NW_ATT));
        BDRT_HIP(hipMemsetAsync(att, 0, n * NW_ATT * sizeof(NewtonAttempt), stream));
        BDRT_HIP(H.alloc(nM)); BDRT_HIP(M.alloc(nM));
        if (env.spec && (NW_ATT - 1) * nM * sizeof(double) <= ((size_t)2 << 30)) BDRT_HIP(M2.alloc((NW_ATT - 1) * nM));
        BDRT_HIP(probes.alloc(b.analytic ? nD * NW_TRY : 2 * nD * D));
        if (b.analytic) BDRT_HIP(hws.alloc(n * b.hl_total));
        else { BDRT_HIP(pgrad.alloc(2 * nD * D)); BDRT_HIP(plp.alloc(2 * nD)); }
        BDRT_HIP(state.alloc(n));
        if (env.prof) {
            BDRT_HIP(prof.alloc(NP_COUNT));
            BDRT_HIP(hipMemset(prof, 0, NP_COUNT * sizeof(long long)));
            BDRT_HIP(hipStreamSynchronize(nullptr));          // the fill is asynchronous; the kernels run on the problem's own stream
        }
        BDRT_HIP(active.alloc(n)); BDRT_HIP(spec1.alloc(n * NW_TRY)); BDRT_HIP(specp.alloc(n * (b.analytic ? 1 : 2 * D)));
        BDRT_HIP(fspec.alloc(n)); BDRT_HIP(lpt.alloc(n * NW_TRY));
        bind();
        return 0;
    }
    // A test entry's one fit: its point, gradient and state up, the active list {0}, and a stand-in for the closed-form Hessian's
    // workspace: the three fields the solve, gather and accept kernels read -- tz [D], act [D], the floor -- and the layout offsets
    // that point at them (tz == nullptr: the log scale, no workspace)
    int one_fit(const double *x_, const double *g_, const NewtonState &hs, const double *tz, const double *held, double floor_x, int o_x, int Kx)
    {
        const int D = b.D, zero = 0;
        if (upload(x, x_, (size_t)D) || upload(g, g_, (size_t)D) || upload(state, &hs, 1) || upload(active, &zero, 1)) return -10;
        if (!tz) return 0;
        std::vector<double> w((size_t)2 * D + 1);
        for (int i = 0; i < D; ++i) { w[i] = tz[i]; w[(size_t)D + i] = held && held[i] != 0.0 ? 1.0 : 0.0; }
        w[(size_t)2 * D] = floor_x;
        if (upload(hws, w.data(), w.size())) return -10;
        b.analytic = 1; b.lin_ok = 1;
        b.hl_total = 2 * D + 1; b.hl_tz = 0; b.hl_act = D; b.hl_floor = 2 * D; b.o_x = o_x; b.Kx = Kx;
        return 0;
    }
    void bind()
    {
        b.x = x; b.g = g; b.gt = gt; b.hstep = hstep; b.s = s; b.xt = xt; b.H = H; b.M = M; b.M2 = M2; b.att = att; b.probes = probes;
        b.pgrad = pgrad; b.plp = plp; b.st = state; b.prof = prof; b.hws = hws; b.fspec = fspec;
    }
    // the kernels that take more dynamic LDS than a launch gets by default: their limits, raised once per device and size
    int raise_lds_limits() const
    {
        static LdsAttrCache prep, fill, solve;
        BDRT_HIP(prep.raise(lds_prep, {(const void *)newton_hess_prep_kernel, (const void *)newton_accept_prep_kernel}));
        BDRT_HIP(fill.raise(lds_fill, {(const void *)newton_hess_fill_kernel}));
        BDRT_HIP(solve.raise(lds_solve, {(const void *)newton_solve_kernel}));
        return 0;
    }
    // (what the profile times as "frees": the matrices and vectors go here and not at the closing brace)
    void release_arrays() { for (DevBuf<double> *d : {&M2, &H, &M, &s, &xt, &gt, &probes, &pgrad, &hws, &x, &g, &hstep, &plp, &lpt}) d->reset(); }
    // the start of the iteration: the fits' states and points up (x0 [n][D], spec [n] or null on the host)
    int start(const double *x0, const int *spec, int n, int max_iter, double tol, hipStream_t stream)
    {
        hst.resize((size_t)n); hspec.resize((size_t)n); hact.resize((size_t)n);
        for (auto &h : hst) { memset(&h, 0, sizeof(h)); h.lam = 1e-3; h.max_iter = max_iter; h.tol = tol; h.rc = 1; h.done = max_iter > 0 ? 0 : 1; }
        BDRT_HIP(hipMemcpy(b.st, hst.data(), hst.size() * sizeof(NewtonState), hipMemcpyHostToDevice));
        BDRT_HIP(hipMemcpy(b.x, x0, (size_t)n * b.D * sizeof(double), hipMemcpyHostToDevice));
        for (int i = 0; i < n; ++i) hspec[i] = spec ? spec[i] : 0;
        return (upload(spec1.p, hspec.data(), (size_t)n, stream) || upload(fspec.p, hspec.data(), (size_t)n, stream)) ? -10 : 0;
    }
    // One host synchronisation, ~90 us: the status records down, the list of the fits that go on and its spectrum ids (one per trial
    // point; one per probe when gradients are differenced) up -- the lists only when they changed.
    int sync_active(hipStream_t stream)
    {
        if (download(hst.data(), b.st, hst.size(), stream)) return -10;
        BDRT_HIP(hipStreamSynchronize(stream));
        n_active = 0; g_far = 0.0;
        for (int i = 0; i < (int)hst.size(); ++i) if (!hst[i].done) { hact[n_active++] = i; g_far = std::max(g_far, hst[i].grad_inf); }
        if (n_active == 0 || ((int)hact_prev.size() == n_active && std::equal(hact_prev.begin(), hact_prev.end(), hact.begin()))) return 0;
        hact_prev.assign(hact.begin(), hact.begin() + n_active);
        sp1.clear(); hspecp.clear();
        for (int f : hact_prev) { sp1.insert(sp1.end(), NW_TRY, hspec[f]); if (!b.analytic) hspecp.insert(hspecp.end(), (size_t)2 * b.D, hspec[f]); }
        return (upload(active.p, hact.data(), (size_t)n_active, stream) || (!b.analytic && upload(specp.p, hspecp.data(), hspecp.size(), stream)) ||
                upload(spec1.p, sp1.data(), sp1.size(), stream)) ? -10 : 0;
    }
};

// Rounds between two host synchronisations: twice as many while some active fit is far from its stationary point (|g| > 0.01: at least three more
// rounds) -- small batches only: a fit that finishes inside a group keeps its rows in the evaluator's batch until the next synchronisation
static int group_length(const NewtonEnv &env, double g_far, int n_active) { return (env.rounds_set || !(g_far > 1e-2) || n_active > 32) ? env.rounds : 2 * env.rounds; }

// One Levenberg-Marquardt round of the active fits, enqueued on the problem's stream.  The sequence of launches does not depend on
// what the round decides (kernels skip the fits that are done; a fit that keeps its Hessian after a rejected trial skips the probe
// writes and ignores the probe gradients), so several rounds are enqueued back to back.
static int enqueue_round(Problem &P, const NewtonWork &w, bool trial_few, int natt, bool first)
{
    const NewtonBufs &b = w.b;
    const int D = b.D, Dp = b.Dp, n_active = w.n_active;
    const int *d_active = w.active;
    const double *d_lpt = w.lpt;
    hipStream_t st = P.stream;
    int rc;
    // probes of the fits that ask for a fresh Hessian (probe slot a = position in the active list) and their gradients
    if (b.analytic) {
        // (the forward quantities of this round's Hessian: left by the previous round's accept + prep kernel, by a launch of
        //  their own in the first round)
        if (first) hipLaunchKernelGGL(newton_hess_prep_kernel, dim3(n_active), dim3(HP_NT), w.lds_prep, st, b, d_active, n_active);
        hipLaunchKernelGGL(newton_hess_fill_kernel, dim3(Dp / 16, n_active), dim3(HP_NT), w.lds_fill, st, b, d_active, n_active);
    } else {
        hipLaunchKernelGGL(newton_probe_kernel, dim3(2 * D, n_active), dim3(128), 0, st, b, d_active, n_active);
        if ((rc = launch_logp_grad(&P, b.probes, w.specp, n_active * 2 * D, 0, b.plp, b.pgrad, nullptr, nullptr, nullptr, st))) return rc;
        hipLaunchKernelGGL(newton_build_kernel, dim3(Dp / 16, n_active), dim3(256), 0, st, b, d_active, n_active);
    }
    hipLaunchKernelGGL(newton_solve_kernel, dim3(n_active, natt), dim3(NW_NT), w.lds_solve, st, b, d_active, n_active, natt);
    // trial points (NW_TRY step lengths per fit) as a dense batch for the evaluator, then the verdict
    hipLaunchKernelGGL(newton_gather_kernel, dim3(n_active, NW_TRY), dim3(128), 0, st, b, d_active, n_active, b.probes, natt);
    // (the one-workgroup-per-point evaluator where the family has one: 8 us against the tile evaluator's 24 for the eight points of
    //  a two-start fit; the same evaluator for every batch size -- a fit's numbers do not depend on its batch)
    rc = trial_few ? launch_logp_grad_few(&P, b.probes, w.spec1, n_active * NW_TRY, 0, w.lpt, b.gt, st, 1) : 1;
    if (rc < 0) return rc;
    if (rc == 1 && (rc = launch_logp_grad(&P, b.probes, w.spec1, n_active * NW_TRY, 0, w.lpt, b.gt, nullptr, nullptr, nullptr, st))) return rc;
    if (b.analytic)
        hipLaunchKernelGGL(newton_accept_prep_kernel, dim3(n_active), dim3(HP_NT), w.lds_prep, st, b, d_active, n_active, d_lpt, (const double *)b.probes);
    else
        hipLaunchKernelGGL(newton_accept_kernel, dim3(n_active), dim3(256), 0, st, b, d_active, n_active, d_lpt, (const double *)b.probes);
    return 0;
}

static void print_trace(const NewtonWork &w, long long round)
{
    for (int i = 0; i < (int)w.hst.size() && i < 8; ++i)
        fprintf(stderr, "[bdrt newton trace] round %lld fit %d spec %d: lp %.12g lam %.3g |g| %.3g iters %d done %d rc %d lin %d\n", round, i, w.hspec[i],
                w.hst[i].lp, w.hst[i].lam, w.hst[i].grad_inf, w.hst[i].iters, w.hst[i].done, w.hst[i].rc, w.hst[i].lin);
}

static int print_profile(const NewtonBufs &b)
{
    long long hp[NP_COUNT];
    if (download(hp, b.prof, (size_t)NP_COUNT)) return -10;
    const double n = hp[NP_CALLS] ? (double)hp[NP_CALLS] : 1.0;
    fprintf(stderr, "[bdrt newton prof] D %d, %lld solve launches (workgroup 0); core cycles per launch: hessian %.0f, build %.0f, "
            "chol diag %.0f / panel %.0f / trailing %.0f, solve %.0f, pred %.0f; wall %.1f us per launch\n", b.D, hp[NP_CALLS],
            hp[NP_HESS] / n, hp[NP_BUILD] / n, hp[NP_DIAG] / n, hp[NP_PANEL] / n, hp[NP_TRAIL] / n, hp[NP_SOLVE] / n, hp[NP_PRED] / n,
            hp[NP_WALL] / n / 100.0);
    fprintf(stderr, "[bdrt newton prof] factorisations started per launch: %.2f\n", hp[NP_ATTEMPTS] / n);
    fprintf(stderr, "[bdrt newton prof] closed-form Hessian, cycles per launch: prep");
    for (int k = NP_PREP0; k <= NP_PREP0 + 8; ++k) fprintf(stderr, " %.0f", hp[k] / n);
    fprintf(stderr, "; fill (row tile 8): stage %.0f, dense product %.0f, entries + stores %.0f; prep wall %.1f us\n", hp[NP_FILL0] / n, hp[NP_FILL0 + 1] / n, hp[NP_FILL0 + 2] / n, hp[NP_PREP0 + 9] / n / 100.0);
    return 0;
}

// Newton polish of n_fits points (x0 [n_fits][D] on the host); results back to x_out, reports filled.  The host only sequences:
// workspace and start points up, then groups of rounds between synchronisations until no fit goes on.
int newton_polish_device(Problem &P, const double *x0, const int *spec, int n_fits, int max_iter, double tol, double *x_out, NewtonReport *rep)
{
    BDRT_HIP(hipSetDevice(P.device));
    const NewtonEnv env = read_newton_env();
    auto now = [] { return std::chrono::steady_clock::now(); };
    const auto t_host0 = now();
    hipStream_t st = P.stream;
    int rc, n_cu = 0;
    BDRT_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, P.device));
    NewtonWork w(P.dev.D);
    NewtonBufs &b = w.b;
    // closed-form Hessian where the model has one, and for a Series_pos model the linear scale of the coefficients
    const int analytic = (hess_analytic_ok(P.dev) && !env.fd) ? 1 : 0;
    w.model(P, analytic, (analytic && P.dev.blk[0].is_pos && env.linear) ? 1 : 0);
    if ((rc = w.alloc((size_t)n_fits, env, st)) || (rc = w.start(x0, spec, n_fits, max_iter, tol, st))) return rc;
    const auto t_host1 = now();
    // evaluation at the start points
    if ((rc = w.raise_lds_limits())) return rc;
    if ((rc = launch_logp_grad(&P, b.x, w.spec1, n_fits, 0, w.lpt, b.gt, nullptr, nullptr, nullptr, st))) return rc;
    hipLaunchKernelGGL(newton_init_kernel, dim3(n_fits), dim3(256), 0, st, b, n_fits, (const double *)w.lpt.p, (const double *)b.gt);
    // the host reads the status records once per group of rounds
    const long long max_rounds = (long long)max_iter * 40 + 100;
    int group = env.rounds;
    for (long long round = 0; round < max_rounds; round += group) {
        if ((rc = w.sync_active(st))) return rc;
        group = group_length(env, w.g_far, w.n_active);
        if (env.trace) print_trace(w, round);
        if (w.n_active == 0) break;
        const int natt = b.M2 ? std::max(1, std::min(NW_ATT, n_cu / w.n_active)) : 1;
        for (int r = 0; r < group; ++r)
            if ((rc = enqueue_round(P, w, env.trial_few, natt, round == 0 && r == 0))) return rc;
        BDRT_HIP(hipGetLastError());
    }
    if (download(w.hst.data(), b.st, w.hst.size(), st) || download(x_out, b.x, (size_t)n_fits * b.D, st)) return -10;
    BDRT_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n_fits; ++i) {
        const NewtonState &h = w.hst[i];
        rep[i] = NewtonReport{h.lp, h.grad_inf, h.iters, h.done ? h.rc : 1, h.n_evals};
    }
    if (b.prof && (rc = print_profile(b))) return rc;
    const auto t_host2 = now();
    w.release_arrays();
    if (env.prof) {
        auto us = [](auto a, auto b) { return (double)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
        fprintf(stderr, "[bdrt newton prof] host: allocations + uploads %.0f us, iteration %.0f us, frees %.0f us\n", us(t_host0, t_host1), us(t_host1, t_host2),
                us(t_host2, now()));
    }
    return 0;
}

// the state of a fit as the debug entry's caller holds it (bdrt_newton_state) <-> as the kernels do: the members both have
template <class From, class To> static void copy_state(const From &a, To &b)
{
    b.lp = a.lp; b.lam = a.lam; b.pred = a.pred; b.gs = a.gs; b.ss = a.ss; b.grad_inf = a.grad_inf; b.tol = a.tol; b.lp_trial = a.lp_trial;
    b.iters = a.iters; b.max_iter = a.max_iter; b.lin = a.lin; b.rc = a.rc; b.done = a.done; b.need_hess = a.need_hess; b.n_evals = a.n_evals;
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

// closed-form Hessian of the log-posterior (no Jacobian) at ONE unconstrained point, as the Newton iteration uses it (tests):
// H_out [D x D] row-major on the host; returns 1 when the model has no closed form here (the iteration then differences gradients).
// lin = 1: with the coefficients of a Series_pos model on the linear scale, as the iteration takes them once its damping has dropped
// (lam stays 0 here, so the kernels' own rule selects the branch from lin_ok); 1 as well when that is asked of a model without
// <lower=0> coefficients.  held_out [D] (may be null): the workspace's `act` slots, 1.0 for a coefficient held at its floor.
int bdrt_debug_hessian_lin(bdrt_problem *p, const double *theta, int spec, int lin, double *H_out, double *held_out)
{
    if (!p || !theta || !H_out || spec < 0 || spec >= p->impl.dev.n_spectra || lin < 0 || lin > 1) { set_error("bdrt_debug_hessian_lin: bad arguments"); return -1; }
    Problem &P = p->impl;
    if (!hess_analytic_ok(P.dev)) return 1;
    if (lin && !P.dev.blk[0].is_pos) return 1;
    BDRT_HIP(hipSetDevice(P.device));
    NewtonWork w(P.dev.D);
    const NewtonBufs &b = w.b;
    const int D = b.D, Dp = b.Dp;
    w.model(P, 1, lin);
    BDRT_HIP(w.x.alloc((size_t)D)); BDRT_HIP(w.g.alloc((size_t)D)); BDRT_HIP(w.H.alloc((size_t)Dp * Dp)); BDRT_HIP(w.M.alloc((size_t)Dp * Dp));
    BDRT_HIP(w.hws.alloc((size_t)b.hl_total)); BDRT_HIP(w.state.alloc(1)); BDRT_HIP(w.active.alloc(1)); BDRT_HIP(w.fspec.alloc(1)); BDRT_HIP(w.lpt.alloc(1));
    w.bind();
    NewtonState hs{};
    hs.need_hess = 1; hs.lam = 0.0;
    const int zero = 0;
    hipStream_t st = P.stream;
    if (upload(b.st, &hs, 1, st) || upload(b.x, theta, (size_t)D, st) || upload(w.active.p, &zero, 1, st) || upload(w.fspec.p, &spec, 1, st)) return -10;
    if (int rc = launch_logp_grad(&P, b.x, w.fspec, 1, 0, w.lpt, b.g, nullptr, nullptr, nullptr, st)) return rc;
    if (int rc = w.raise_lds_limits()) return rc;
    hipLaunchKernelGGL(newton_hess_prep_kernel, dim3(1), dim3(HP_NT), w.lds_prep, st, b, (const int *)w.active.p, 1);
    hipLaunchKernelGGL(newton_hess_fill_kernel, dim3(Dp / 16, 1), dim3(HP_NT), w.lds_fill, st, b, (const int *)w.active.p, 1);
    BDRT_HIP(hipGetLastError());
    std::vector<double> hh((size_t)Dp * Dp);
    if (download(hh.data(), b.H, hh.size(), st) || (held_out && download(held_out, b.hws + b.hl_act, (size_t)D, st))) return -10;
    BDRT_HIP(hipStreamSynchronize(st));
    // (the kernels write the block lower triangle: mirror it)
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) H_out[(size_t)i * D + j] = H_out[(size_t)j * D + i] = hh[(size_t)i * Dp + j];
    return 0;
}

int bdrt_debug_hessian(bdrt_problem *p, const double *theta, int spec, double *H_out) { return bdrt_debug_hessian_lin(p, theta, spec, 0, H_out, nullptr); }

// One launch of the damped solve on the caller's data (tests): newton_build_kernel's need_hess == 0 branch, newton_solve_kernel with
// natt attempts, newton_gather_kernel -- the launches of a round of newton_polish_device for one fit that keeps its Hessian.
int bdrt_debug_newton_solve(const double *H, const double *g, const double *x, int D, double lam, int natt, const double *tz,
                            const double *held, double floor_x, int o_x, int Kx, double *L_out, double *s_out, double *trial_out,
                            bdrt_newton_solve_record *rec)
{
    if (!H || !g || !x || !L_out || !s_out || !trial_out || !rec || D < 1 || natt < 1 || natt > 6 || !(lam > 0.0) ||
        (tz && (o_x < 0 || Kx < 0 || o_x + Kx > D))) { set_error("bdrt_debug_newton_solve: bad arguments"); return -1; }
    NewtonWork w(D);
    const NewtonBufs &b = w.b;
    const int Dp = b.Dp;
    const size_t nM = (size_t)Dp * Dp;
    if (w.lds_solve + 64 > 160 * 1024) { set_error("bdrt_debug_newton_solve: D = %d needs %zu bytes of LDS", D, w.lds_solve); return -2; }     // (+ the kernel's static LDS)
    bind_process_device();
    std::vector<double> hh(nM, 0.0);
    for (int i = 0; i < D; ++i) memcpy(&hh[(size_t)i * Dp], H + (size_t)i * D, (size_t)D * sizeof(double));
    NewtonState hs{};
    hs.lam = lam; hs.rc = 1; hs.lin = tz ? 1 : 0;
    int rc;
    if ((rc = w.one_fit(x, g, hs, tz, held, floor_x, o_x, Kx)) || (rc = upload(w.H, hh.data(), nM))) return rc;
    BDRT_HIP(w.s.alloc((size_t)NW_ATT * D)); BDRT_HIP(w.xt.alloc((size_t)NW_ATT * D)); BDRT_HIP(w.probes.alloc((size_t)NW_TRY * D)); BDRT_HIP(w.M.alloc(nM));
    BDRT_HIP(w.att.alloc(NW_ATT));
    BDRT_HIP(hipMemset(w.att, 0, NW_ATT * sizeof(NewtonAttempt)));
    if (natt > 1) {
        // (the speculative attempts write the lower block triangle of their matrices only: the rest reads as zero)
        BDRT_HIP(w.M2.alloc((NW_ATT - 1) * nM));
        BDRT_HIP(hipMemset(w.M2, 0, (NW_ATT - 1) * nM * sizeof(double)));
    }
    w.bind();
    if ((rc = w.raise_lds_limits())) return rc;
    hipStream_t st = nullptr;
    hipLaunchKernelGGL(newton_build_kernel, dim3(Dp / 16, 1), dim3(256), 0, st, b, (const int *)w.active.p, 1);
    hipLaunchKernelGGL(newton_solve_kernel, dim3(1, natt), dim3(NW_NT), w.lds_solve, st, b, (const int *)w.active.p, 1, natt);
    hipLaunchKernelGGL(newton_gather_kernel, dim3(1, NW_TRY), dim3(128), 0, st, b, (const int *)w.active.p, 1, b.probes, natt);
    BDRT_HIP(hipGetLastError());
    BDRT_HIP(hipStreamSynchronize(st));
    NewtonAttempt hatt[NW_ATT];
    if (download(hatt, (const NewtonAttempt *)b.att, (size_t)NW_ATT) || download(&hs, (const NewtonState *)b.st, 1)) return -10;
    int c = 0;
    while (c + 1 < natt && !hatt[c].ok) ++c;                           // the gather kernel's choice
    const double *Mc = c ? b.M2 + (size_t)(c - 1) * nM : b.M;
    if (download(L_out, Mc, nM) || download(s_out, (const double *)b.s + (size_t)c * D, (size_t)D) ||
        download(trial_out, (const double *)b.probes, (size_t)NW_TRY * D)) return -10;
    rec->ok = hatt[c].ok; rec->attempt = c; rec->rc = hs.rc; rec->done = hs.done;
    rec->lam = hs.lam; rec->pred = hs.pred; rec->gs = hs.gs; rec->ss = hs.ss;
    return 0;
}

// One launch of newton_accept_kernel on the caller's data (tests): the state, the point and its gradient before and after
int bdrt_debug_newton_accept(bdrt_newton_state *s, double *x, double *g, int D, const double *trial, const double *lp_t,
                             const double *gt, const double *tz, const double *held, double floor_x, int o_x, int Kx)
{
    if (!s || !x || !g || !trial || !lp_t || !gt || D < 1 || (tz && (o_x < 0 || Kx < 0 || o_x + Kx > D))) { set_error("bdrt_debug_newton_accept: bad arguments"); return -1; }
    bind_process_device();
    NewtonWork w(D);
    const NewtonBufs &b = w.b;
    NewtonState hs{};
    copy_state(*s, hs);
    if (!tz) hs.lin = 0;
    int rc;
    if ((rc = w.one_fit(x, g, hs, tz, held, floor_x, o_x, Kx)) || (rc = upload(w.gt, gt, (size_t)NW_TRY * D)) ||
        (rc = upload(w.probes, trial, (size_t)NW_TRY * D)) || (rc = upload(w.lpt, lp_t, (size_t)NW_TRY))) return rc;
    w.bind();
    hipStream_t st = nullptr;
    hipLaunchKernelGGL(newton_accept_kernel, dim3(1), dim3(256), 0, st, b, (const int *)w.active.p, 1, (const double *)w.lpt.p, (const double *)b.probes);
    BDRT_HIP(hipGetLastError());
    BDRT_HIP(hipStreamSynchronize(st));
    if (download(&hs, (const NewtonState *)b.st, 1) || download(x, (const double *)b.x, (size_t)D) || download(g, (const double *)b.g, (size_t)D)) return -10;
    copy_state(hs, *s);
    return 0;
}

}  // extern "C"
