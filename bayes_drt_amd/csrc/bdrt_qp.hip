// bdrt_qp.hip -- batched box-constrained QP on the GPU: the ridge / hyper-lambda ridge solve (include/bdrt.h section (3)).
//
// Replaces cvxopt.solvers.qp inside Inverter._convex_opt (reference bayes_drt/inversion.py:1043-1067), which the
// reference calls once per hyper-lambda iteration and 2 x len(lambdas) x iterations times inside ridge_ReImCV (:902-945):
//     min 1/2 x'Px + q'x   s.t.  x >= lo        (lo[i] = -inf: free variable)
// Same algorithm as the host solver bdrt_qp_box (bdrt_ridge.hip, which documents it): cvxopt's coneqp path-following
// method (Mehrotra predictor-corrector, cvxopt's starting point, residual handling, step rules and default tolerances
// abstol 1e-7 / reltol 1e-6 / feastol 1e-7, 100 iterations) specialised to G = -I.  The ridge problems are nearly flat, so
// where on the central path the iteration stops is part of the reference's answer: the solver reproduces solutions cvxopt
// itself computed (stored in the reference's pickled fits) to 1e-8 (tests/test_ridge_reference.py).
//
// One workgroup (512 threads) per problem; problems of a batch run concurrently (Re-Im cross-validation: 62 fits).  The
// KKT matrix lives in LDS as a column-major packed lower triangle (qp_lds_plan: n <= 185 for the plain QP, n <= 180 under the
// ridge kernel's own vectors; 156.5 KiB and 157.3 KiB there) -- or in a global work buffer for larger n -- and is factored by a
// blocked right-looking Cholesky (chol_packed); the two triangular solves of a Newton direction are blocked the same way
// (chol_solve_blocked).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bdrt_host.h"

namespace bdrt {

constexpr int QP_NT = 512;
// BDRT_QP_PROF=1: core-clock cycles of workgroup 0's phases (form KKT, factor, triangular solves, everything else), printed per call
__device__ long long g_qp_prof[8];
__device__ int g_qp_prof_on;
struct QpProf {
    long long t; bool on;
    __device__ QpProf() : t(0), on(g_qp_prof_on && blockIdx.x == 0 && threadIdx.x == 0) { if (on) t = clock64(); }
    __device__ void mark(int k) { if (on) { const long long n = clock64(); g_qp_prof[k] += n - t; t = n; } }
};
constexpr int QP_NVEC = 14;          // x, s, z, rd, rhs, dx, ds, dz, dsa, dza, Px, lo, bounded, rz

__device__ __forceinline__ void qp_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wave_sum64(double x)
{
    x += __shfl_xor(x, 32); x += __shfl_xor(x, 16); x += __shfl_xor(x, 8);
    x += __shfl_xor(x, 4); x += __shfl_xor(x, 2); x += __shfl_xor(x, 1);
    return x;
}

// sums of up to 3 per-thread values over the workgroup (deterministic order); result to all threads
__device__ inline void block_sum3(double &a, double &b, double &c, double *red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    a = wave_sum64(a); b = wave_sum64(b); c = wave_sum64(c);
    __syncthreads();                       // red may still be read from the previous call
    if (lane == 0) { red[wave] = a; red[8 + wave] = b; red[16 + wave] = c; }
    __syncthreads();
    double sa = 0, sb = 0, sc = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) { sa += red[w]; sb += red[8 + w]; sc += red[16 + w]; }
    a = sa; b = sb; c = sc;
}

__device__ inline double block_min(double v, double *red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double m = red[0];
#pragma unroll
    for (int w = 1; w < 8; ++w) m = fmin(m, red[w]);
    return m;
}

// column-major packed lower triangle: element (i, j), i >= j
__device__ __forceinline__ int cidx(int i, int j, int n) { return j * n - ((j * (j - 1)) >> 1) + (i - j); }      // (n < 46 000: 32-bit index arithmetic)

// In-place Cholesky of the packed lower triangle; diag[j] receives L(j,j) (M(j,j) keeps the pivot).  Returns false
// (uniformly) when a pivot is not positive.  All threads of the workgroup must call.  Right-looking in blocks of 16 columns
// (round 4; round 2's form updated the whole trailing triangle after every column -- two workgroup barriers and a pass over up to
// n^2 / 2 LDS cells per column: 570 k cycles at n = 163, 60 % of an interior-point iteration):
//   (a) the 16 x 16 diagonal block by wavefront 0 on a register copy, lane r = row r; the scaled column reaches the other lanes
//       through a 16-double LDS buffer (one round trip per column);
//   (b) the rows below by forward substitution against the block, one row per thread;
//   (c) the trailing triangle on v_mfma_f64_16x16x4 tiles, operands and cells straight from the packed triangle.
// Three barriers per block.  `scr`: 32 doubles of scratch.
// LDSM: M is in LDS -- addressed as such (through a generic pointer every access is a flat load: several times the latency)
template <bool LDSM>
__device__ __noinline__ bool chol_packed(double *M, double *diag, int n, double *scr)
{
    typedef __attribute__((address_space(3))) double *lds_dptr;
    auto LD = [&](int idx) -> double { if constexpr (LDSM) return ((lds_dptr)M)[idx]; else return M[idx]; };
    auto ST = [&](int idx, double val) { if constexpr (LDSM) ((lds_dptr)M)[idx] = val; else M[idx] = val; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_bad;
    __shared__ double s_inv[16];
    __shared__ double s_tile[16 * 17];
    int *bad = &s_bad;
    if (tid == 0) *bad = 0;
    __syncthreads();
    QpProf pq;
    for (int j0 = 0; j0 < n; j0 += 16) {
        const int jb = min(16, n - j0), m = n - j0 - jb;
        pq.mark(7);
        // (a) the block in a 16 x 17 LDS tile, thread (r, k) of the first 256 owns element (r, k), k <= r.  Column c: every thread
        //     reads the pivot and its two column-c entries as they stand, scales them itself (the columns stay unscaled in the
        //     tile until the end: nobody writes what another thread reads in the same step) and updates its own element --
        //     one barrier per column.
        {
            const int r = tid >> 4, k = tid & 15;
            const bool mine = tid < 256 && r < jb && k <= r;
            if (mine) s_tile[r * 17 + k] = LD(cidx(j0 + r, j0 + k, n));
            __syncthreads();
            bool ok = true;
            double mineval = mine ? s_tile[r * 17 + k] : 0.0;
            for (int c = 0; c < jb; ++c) {
                const double d = s_tile[c * 17 + c];
                ok = ok && d > 0.0 && isfinite(d);
                // 1 / sqrt(d): hardware estimate + two Newton steps
                double inv = __builtin_amdgcn_rsq(d);
                inv = inv * (1.5 - 0.5 * d * inv * inv);
                inv = inv * (1.5 - 0.5 * d * inv * inv);
                if (tid == c) {
                    // sqrt(d) = d * inv, then one correction from the residual d - g^2 (an FMA gives it exactly): g^2 matches the
                    // pivot to an ulp or two, where d * inv alone carries the error of inv twice over
                    const double g = d * inv;
                    diag[j0 + c] = fma(0.5 * inv, fma(-g, g, d), g);
                    s_inv[c] = inv;
                }
                if (mine && k > c) {
                    const double lr = s_tile[r * 17 + c] * inv, lk = s_tile[k * 17 + c] * inv;
                    mineval -= lr * lk;
                    s_tile[r * 17 + k] = mineval;
                }
                __syncthreads();
            }
            if (!ok) { if (tid == 0) *bad = 1; }
            else if (mine) ST(cidx(j0 + r, j0 + k, n), k < r ? mineval * s_inv[k] : mineval);     // (the diagonal keeps the pivot)
        }
        __syncthreads();
        pq.mark(5);
        if (*bad) return false;
        if (m > 0) {
            // (b) x_c = (a_c - sum_{k < c} x_k L(c, k)) / L(c, c), one row per thread (jb = 16 here)
            for (int i = j0 + 16 + tid; i < n; i += QP_NT) {
                double x[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) x[c] = LD(cidx(i, j0 + c, n));
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    double t = x[c];
#pragma unroll
                    for (int k = 0; k < c; ++k) t -= x[k] * LD(cidx(j0 + c, j0 + k, n));
                    x[c] = t * s_inv[c];
                    __builtin_amdgcn_sched_barrier(0);      // one row of the block at a time (else all 120 operands are requested up front)
                }
#pragma unroll
                for (int c = 0; c < 16; ++c) ST(cidx(i, j0 + c, n), x[c]);
            }
            __syncthreads();
            pq.mark(6);
            // (c) C(i, k) -= sum_c X(i, c) X(k, c) on the tiles of the lower triangle of the trailing part
            const int r0 = j0 + 16, mb = (m + 15) >> 4, ntile = mb * (mb + 1) / 2;
            const int col = lane & 15, kq = lane >> 4;
            for (int t = wave; t < ntile; t += QP_NT / 64) {
                int I = (int)((__fsqrt_rn((float)(8 * t + 1)) - 1.0f) * 0.5f);
                while ((I + 1) * (I + 2) / 2 <= t) ++I;
                while (I * (I + 1) / 2 > t) --I;
                const int Jc = t - I * (I + 1) / 2;
                const int R0 = r0 + 16 * I, C0 = r0 + 16 * Jc;
                const int ia = R0 + col, ib = C0 + col;                     // operand rows of this lane
                double xa[4], xb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xa[u] = ia < n ? LD(cidx(ia, j0 + 4 * u + kq, n)) : 0.0;
                    xb[u] = ib < n ? LD(cidx(ib, j0 + 4 * u + kq, n)) : 0.0;
                }
                // the block's sixteen products are summed from zero and leave the cell in one subtraction: one rounding on the scale
                // of the cell per block.  (Accumulated onto the cell itself every product rounds on that scale -- sixteen times as
                // many; where the diagonal dominates, as under a barrier term z / s, the factor's residual was 4 .. 7 times LAPACK's.)
                d4 acc = {0.0, 0.0, 0.0, 0.0};
                bool own[4];
                double cell[4];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int ri = R0 + kq + 4 * rr, ci = C0 + col;
                    own[rr] = ri < n && ci <= ri;
                    cell[rr] = own[rr] ? LD(cidx(ri, ci, n)) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = mfma_f64(xa[u], xb[u], acc);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    if (own[rr]) ST(cidx(R0 + kq + 4 * rr, C0 + col, n), cell[rr] - acc[rr]);
            }
            __syncthreads();
        }
    }
    return true;
}

// v <- (L L^T)^-1 v (L strictly-lower part in M, diagonal in diag); ends with a workgroup barrier.  Blocked by 16 unknowns:
// the 16 x 16 triangle of a block by 16 lanes of wavefront 0 with the block's right-hand side in registers (the unknown just found
// goes to the other lanes through v_readlane), the rest of the right-hand side by the whole workgroup -- forward one row per
// thread, backward 32 threads per column.  (Round 2's form did both substitutions with one wavefront, two wave-level exchanges and a
// division per unknown: about 40 % of an interior-point iteration at n = 163.)  rd: 1 / diag, scratch of n doubles; tb: 16 doubles.
template <bool LDSM>
__device__ __noinline__ void chol_solve_blocked(const double *M, const double *diag, int n, double *v, double *rd, double *tb)
{
    typedef const __attribute__((address_space(3))) double *lds_cdptr;
    auto LD = [&](int idx) -> double { if constexpr (LDSM) return ((lds_cdptr)M)[idx]; else return M[idx]; };
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < n; i += QP_NT) rd[i] = 1.0 / diag[i];
    __syncthreads();
    const int nb = (n + 15) / 16;
    auto bcast = [](double y, int c) { return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(y), c), __builtin_amdgcn_readlane(__double2loint(y), c)); };
    for (int J = 0; J < nb; ++J) {                                      // forward: L y = v
        const int j0 = 16 * J, jb = min(16, n - j0);
        if (tid < 64) {
            // lane r: row j0 + r of the block's triangle in registers (zeros outside it), its own reciprocal pivot
            const int r = lane & 15, i = j0 + r;
            const bool in = r < jb;
            double Lr[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) Lr[c] = (in && c < r) ? LD(cidx(i, j0 + c, n)) : 0.0;
            const double rdo = in ? rd[i] : 1.0;
            double t = in ? v[i] : 0.0;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const double yc = bcast(t * rdo, c);
                t = r == c ? yc : t - Lr[c] * yc;
            }
            if (lane < jb) v[i] = t;
        }
        __syncthreads();
        for (int i = j0 + jb + tid; i < n; i += QP_NT) {
            // (jb = 16 here: only the last block is shorter, and nothing lies below it; all sixteen requests go out together)
            double Lrow[16], yv[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) { Lrow[c] = LD(cidx(i, j0 + c, n)); yv[c] = v[j0 + c]; }
            double t = 0.0;
#pragma unroll
            for (int c = 0; c < 16; ++c) t += Lrow[c] * yv[c];
            v[i] -= t;
        }
        __syncthreads();
    }
    for (int J = nb - 1; J >= 0; --J) {                                 // backward: L^T x = y
        const int j0 = 16 * J, jb = min(16, n - j0);
        {
            const int c = tid >> 5, l32 = tid & 31;                     // 32 threads per column of the block
            double t = 0.0;
            if (c < jb) {
                const int cj = cidx(j0 + c, j0 + c, n);                 // LD(cj + i - j) = L(i, j)
                for (int i = j0 + jb + l32; i < n; i += 32) t += LD(cj + i - (j0 + c)) * v[i];
            }
            t += __shfl_xor(t, 16); t += __shfl_xor(t, 8); t += __shfl_xor(t, 4); t += __shfl_xor(t, 2); t += __shfl_xor(t, 1);
            if (l32 == 0 && c < 16) tb[c] = t;
        }
        __syncthreads();
        if (tid < 64) {
            // lane r: column j0 + r of the block's triangle (row r of its transpose)
            const int r = lane & 15, j = j0 + r;
            const bool in = r < jb;
            double Lc[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) Lc[c] = (in && c > r && c < jb) ? LD(cidx(j0 + c, j, n)) : 0.0;
            const double rdo = in ? rd[j] : 1.0;
            double u = in ? v[j] - tb[r] : 0.0;
#pragma unroll
            for (int c = 15; c >= 0; --c) {
                const double xc = bcast(u * rdo, c);
                u = r == c ? xc : u - Lc[c] * xc;
            }
            if (lane < jb) v[j] = u;
        }
        __syncthreads();
    }
}

// M <- the packed lower triangle of sym(P) + diag(dgv(i)) + reg I, factored in place by chol_packed: reg = 0 first, then the
// ladder 1e-14 (1 + |M(0,0)|), x 100 per rung while reg <= 1e6, until a factorisation runs to completion.  P [n x n] row-major in
// global memory (not necessarily symmetric); red: 32 doubles of scratch.  Returns (uniformly) whether a rung factored; *reg_out,
// *rungs_out (null: not wanted): the reg last added and the number of factorisations tried.  All threads must call.
template <bool LDSM, class DG>
__device__ inline bool qp_factor(const double *__restrict__ P, int n, double *M, double *diag, double *red, DG dgv, QpProf &pf,
                                 double *reg_out, int *rungs_out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double reg = 0.0;
    bool ok = false;
    int rungs = 0;
    while (true) {
        __syncthreads();
        pf.mark(3);
        for (int j = wave; j < n; j += QP_NT / 64) {              // one wavefront per column of the lower triangle
            double *colj = M + cidx(j, j, n);
            for (int i = j + lane; i < n; i += 64) {
                double v = 0.5 * (P[(size_t)i * n + j] + P[(size_t)j * n + i]);
                if (i == j) v += dgv(i) + reg;
                colj[i - j] = v;
            }
        }
        __syncthreads();
        pf.mark(0);
        const double m00 = M[0] - reg;
        ok = chol_packed<LDSM>(M, diag, n, red);
        ++rungs;
        pf.mark(1);
        if (ok) break;
        reg = reg == 0.0 ? 1e-14 * (1.0 + fabs(m00)) : reg * 100.0;
        if (!(reg <= 1e6)) break;                                  // (also leaves on NaN: non-finite input must not spin here)
    }
    if (reg_out) *reg_out = reg;
    if (rungs_out) *rungs_out = rungs;
    return ok;
}

// One box-constrained QP by the calling workgroup: P [n x n] and q [n] in global memory, the solution is left in sh[0..n)
// (LDS) and, when xout != nullptr, copied there.  sh: (QP_NVEC + 1) * np + 32 doubles of LDS followed (LDSM) by the packed
// KKT triangle; Mwork: the triangle when it lives in a global work buffer.  Returns the iteration count, -3 (KKT matrix not
// positive definite) or -4 (iteration limit: the last iterate is left in place, as cvxopt does with status 'unknown');
// *pobj_out receives the primal objective.  All threads must call.
// Algorithm: cvxopt's coneqp path-following method for G = -I, h = -lo, restated in unscaled variables -- the same
// statement as the host solver bdrt_qp_box (bdrt_ridge.hip), which documents it.
template <bool LDSM>
__device__ inline int qp_box_solve(const double *__restrict__ P, const double *__restrict__ q, const double *__restrict__ lo,
                                   int n, double *sh, double *Mwork, double *xout, double *pobj_out)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = (n + 1) & ~1;
    double *x = sh, *s = x + np, *z = s + np, *rd = z + np, *rhs = rd + np, *dx = rhs + np, *ds = dx + np, *dz = ds + np,
           *dsa = dz + np, *dza = dsa + np, *Px = dza + np, *lv = Px + np, *bd = lv + np, *rz = bd + np, *diag = rz + np,
           *red = diag + np;
    double *M = LDSM ? red + 32 : Mwork;
    const double abstol = 1e-7, reltol = 1e-6, feastol = 1e-7;      // cvxopt.solvers.options defaults
    const int max_it = 100;                                          // cvxopt 'maxiters'

    double nbv = 0.0, qq = 0.0, hh = 0.0;
    for (int i = tid; i < n; i += QP_NT) {
        const double li = lo ? lo[i] : -INFINITY;
        const bool bnd = isfinite(li);
        bd[i] = bnd ? 1.0 : 0.0;
        lv[i] = bnd ? li : 0.0;
        s[i] = 0.0; z[i] = 0.0; rz[i] = 0.0; ds[i] = 0.0; dz[i] = 0.0; dsa[i] = 0.0; dza[i] = 0.0;
        nbv += bnd ? 1.0 : 0.0;
        qq += q[i] * q[i];
        hh += bnd ? li * li : 0.0;
    }
    block_sum3(nbv, qq, hh, red);
    const double resx0 = fmax(1.0, sqrt(qq)), resz0 = fmax(1.0, sqrt(hh));
    const int nb = (int)nbv;

    auto matvec = [&]() {                                             // Px = P x : one wavefront per row
        __syncthreads();
        for (int i = wave; i < n; i += QP_NT / 64) {
            const double *row = P + (size_t)i * n;
            double t = 0.0;
            for (int j = lane; j < n; j += 64) t += row[j] * x[j];
            t = wave_sum64(t);
            if (lane == 0) Px[i] = t;
        }
        __syncthreads();
    };
    // factor sym(P) + diag(dgv[i]) (+ reg I when only semi-definite); dgv: unit = 1 on bounded variables, else z/s
    QpProf pf;
    auto factor = [&](bool unit) -> bool {
        return qp_factor<LDSM>(P, n, M, diag, red, [&](int i) { return bd[i] != 0.0 ? (unit ? 1.0 : z[i] / s[i]) : 0.0; }, pf, nullptr, nullptr);
    };

    // ---- starting point: (P + diag(b)) x = -q + b lo; s = x - lo, z = -s, both shifted into the interior ----
    if (!factor(true)) { *pobj_out = 0.0; return -3; }
    for (int i = tid; i < n; i += QP_NT) x[i] = -q[i] + (bd[i] != 0.0 ? lv[i] : 0.0);
    __syncthreads();
    pf.mark(3);
    chol_solve_blocked<LDSM>(M, diag, n, x, rhs, red);
    pf.mark(2);
    {
        double nrm2 = 0.0, mn = INFINITY, mx = INFINITY, dummy = 0.0, dummy2 = 0.0;
        for (int i = tid; i < n; i += QP_NT)
            if (bd[i] != 0.0) {
                const double si = x[i] - lv[i];
                s[i] = si; z[i] = -si;
                nrm2 += si * si;
                mn = fmin(mn, si);                                    // ts = max(-s) = -min(s)
                mx = fmin(mx, -si);                                   // tz = max(-z) = -min(z) = -min(-s)
            }
        block_sum3(nrm2, dummy, dummy2, red);
        const double ts = -block_min(mn, red), tz = -block_min(mx, red);
        const double nrm = fmax(sqrt(nrm2), 1.0);
        for (int i = tid; i < n; i += QP_NT)
            if (bd[i] != 0.0) {
                if (nb && ts >= -1e-8 * nrm) s[i] += 1.0 + ts;
                if (nb && tz >= -1e-8 * nrm) z[i] += 1.0 + tz;
            }
        __syncthreads();
    }

    int it = 0, status = 0;
    for (;; ++it) {
        matvec();
        double f0 = 0.0, gap = 0.0, resx = 0.0, resz = 0.0, zrz = 0.0, dummy = 0.0;
        for (int i = tid; i < n; i += QP_NT) {
            const double r0 = Px[i] + q[i];
            f0 += x[i] * r0 + x[i] * q[i];
            const double r = r0 - (bd[i] != 0.0 ? z[i] : 0.0);
            rd[i] = r;
            resx += r * r;
            if (bd[i] != 0.0) {
                const double rzi = s[i] - (x[i] - lv[i]);
                rz[i] = rzi;
                resz += rzi * rzi;
                zrz += z[i] * rzi;
                gap += s[i] * z[i];
            }
        }
        block_sum3(f0, gap, resx, red);
        block_sum3(resz, zrz, dummy, red);
        resx = sqrt(resx); resz = sqrt(resz);
        const double pcost = 0.5 * f0, dcost = pcost + zrz - gap;
        double relgap = INFINITY;
        if (pcost < 0) relgap = gap / -pcost; else if (dcost > 0) relgap = gap / dcost;
        if (resz / resz0 <= feastol && resx / resx0 <= feastol && (gap <= abstol || relgap <= reltol)) break;
        if (it == max_it) { status = -4; break; }
        const double mu = nb ? gap / nb : 0.0;
        if (!factor(false)) { status = -3; break; }

        auto solve_dir = [&](double sigma_mu, bool corrector) {
            for (int i = tid; i < n; i += QP_NT) {
                double t = 0.0;
                if (bd[i] != 0.0) {
                    double rc = sigma_mu - s[i] * z[i];
                    if (corrector) rc -= dsa[i] * dza[i];
                    t = (rc + z[i] * rz[i]) / s[i];
                }
                rhs[i] = -rd[i] + t;
                dx[i] = rhs[i];
            }
            __syncthreads();
            pf.mark(3);
            chol_solve_blocked<LDSM>(M, diag, n, dx, Px, red);
            pf.mark(2);
            for (int i = tid; i < n; i += QP_NT) {
                if (bd[i] != 0.0) {
                    double rc = sigma_mu - s[i] * z[i];
                    if (corrector) rc -= dsa[i] * dza[i];
                    ds[i] = dx[i] - rz[i];
                    dz[i] = (rc - z[i] * ds[i]) / s[i];
                } else { ds[i] = 0.0; dz[i] = 0.0; }
            }
            __syncthreads();
        };
        auto boundary = [&]() {                                       // t = max(0, max -ds/s, max -dz/z)
            double t = 0.0;
            for (int i = tid; i < n; i += QP_NT) {
                if (bd[i] == 0.0) continue;
                t = fmax(t, -ds[i] / s[i]);
                t = fmax(t, -dz[i] / z[i]);
            }
            return -block_min(-t, red);
        };
        solve_dir(0.0, false);                                        // predictor (affine scaling)
        double dsdz = 0.0, d1 = 0.0, d2 = 0.0;
        for (int i = tid; i < n; i += QP_NT)
            if (bd[i] != 0.0) dsdz += ds[i] * dz[i];
        block_sum3(dsdz, d1, d2, red);
        double t = boundary();
        double step = t == 0.0 ? 1.0 : fmin(1.0, 1.0 / t);
        double sigma = gap > 0 ? 1.0 - step + dsdz / gap * step * step : 0.0;
        sigma = fmin(1.0, fmax(0.0, sigma));
        sigma = sigma * sigma * sigma;
        for (int i = tid; i < n; i += QP_NT) { dsa[i] = ds[i]; dza[i] = dz[i]; }
        __syncthreads();
        solve_dir(sigma * mu, true);                                  // corrector
        t = boundary();
        step = t == 0.0 ? 1.0 : fmin(1.0, 0.99 / t);
        for (int i = tid; i < n; i += QP_NT) {
            x[i] += step * dx[i];
            if (bd[i] != 0.0) { s[i] += step * ds[i]; z[i] += step * dz[i]; }
        }
        __syncthreads();
    }
    matvec();
    double pobj = 0.0, d1 = 0.0, d2 = 0.0;
    for (int i = tid; i < n; i += QP_NT) {
        pobj += x[i] * (0.5 * Px[i] + q[i]);
        if (xout) xout[i] = x[i];
    }
    block_sum3(pobj, d1, d2, red);
    pf.mark(3);
    if (pf.on) g_qp_prof[4] += it;
    *pobj_out = pobj;
    __syncthreads();
    return status < 0 ? status : it;
}

template <bool LDSM>
__global__ __launch_bounds__(QP_NT) void qp_box_kernel(const double *__restrict__ Pall, const double *__restrict__ qall,
                                                       const double *__restrict__ lo, int n, double *__restrict__ Xall,
                                                       double *__restrict__ objall, int *__restrict__ itall,
                                                       double *__restrict__ work)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int b = blockIdx.x;
    const size_t msize = (size_t)n * (n + 1) / 2;
    double pobj;
    const int its = qp_box_solve<LDSM>(Pall + (size_t)b * n * n, qall + (size_t)b * n, lo, n, sh, LDSM ? nullptr : work + (size_t)b * msize,
                                       Xall + (size_t)b * n, &pobj);
    if (threadIdx.x == 0) { objall[b] = pobj; itall[b] = its; }
}

// ---- hyper-lambda ridge: the whole outer loop of Inverter.ridge_fit on the device ---------------------------------------------
// (reference bayes_drt/inversion.py:518-740; lambda updates :947-983; see include/bdrt.h bdrt_ridge for the arithmetic)
struct RidgeArgs {
    int n, K, off, penalty, max_iter, hyper_lambda;
    double xtol;
    double reg_ord[3];
    const double *G, *qbase;     // [ng][n][n], [ng][n]
    const int *gsel;             // [nb]
    const unsigned char *zero_delta1_g;   // [ng]  data part g leaves entry 1 out of the convergence test
    const double *hl_fbeta_b;    // [nb]       <= 0: analytic discrete update
    const double *base;          // [3][n][n]
    const double *Ls;            // [3][K][n] (discrete penalty)
    const double *lo;            // [n]
    const double *lambda0;       // [nb]       start value of every lambda vector
    const double *lam0s, *betas; // [nb][3]    prior rate / shape terms of the lambda update (see bdrt.h)
    const double *x0;            // [nb][n] or nullptr
    double *Pwork;               // [nb][n][n]
    double *Mwork;               // [nb][n(n+1)/2] when the KKT triangle does not fit in LDS
    double *coef, *lam, *cost, *fun;
    int *iters, *flags;
    double *hist_coef, *hist_lam, *hist_fun, *hist_cost;
};

template <bool LDSM>
__global__ __launch_bounds__(QP_NT) void ridge_kernel(RidgeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, K = a.K, off = a.off;
    const int np = (n + 1) & ~1;
    // LDS: [QP vectors + reduction scratch (+ KKT triangle) | coef | prev | lam[3] | tmp | red]
    const size_t qp_doubles = (size_t)(QP_NVEC + 1) * np + 32 + (LDSM ? (size_t)n * (n + 1) / 2 : 0);
    double *coef = sh + ((qp_doubles + 1) & ~(size_t)1), *prev = coef + np, *lam = prev + np, *tmp = lam + 3 * np, *red = tmp + np;
    const double *G = a.G + (size_t)a.gsel[b] * n * n, *q = a.qbase + (size_t)a.gsel[b] * n;
    double *P = a.Pwork + (size_t)b * n * n;
    double *Mw = LDSM ? nullptr : a.Mwork + (size_t)b * ((size_t)n * (n + 1) / 2);
    const double l0 = a.lambda0[b], hl_fbeta = a.hl_fbeta_b[b];
    const bool zero_delta1 = a.zero_delta1_g[a.gsel[b]] != 0;
    for (int i = tid; i < n; i += QP_NT) {
        coef[i] = a.x0 ? a.x0[(size_t)b * n + i] : 1e-6;
        lam[i] = l0; lam[np + i] = l0; lam[2 * np + i] = l0;
    }
    __syncthreads();
    int it = 0, flag = 0, qp_its = 0;
    double cost = 0.0, fun = 0.0;
    const int iters_max = a.hyper_lambda ? a.max_iter : 1;
    while (it < iters_max) {
        for (int i = tid; i < n; i += QP_NT) prev[i] = coef[i];
        __syncthreads();
        if (a.hyper_lambda) {
            for (int o = 0; o < 3; ++o) {
                if (!(a.reg_ord[o] > 0.0)) continue;
                const double *Mb = a.base + (size_t)o * n * n;
                double *lv = lam + o * np;
                const double beta = a.betas[b * 3 + o], lam0 = a.lam0s[b * 3 + o];
                if (a.penalty == 0) {
                    // discrete: (L x)^2 per row of L_o, then the closed-form lambda (inversion.py:947-964)
                    const double *L = a.Ls + (size_t)o * K * n;
                    for (int r = wave; r < K; r += QP_NT / 64) {
                        const double *row = L + (size_t)r * n;
                        double t = 0.0;
                        for (int c = lane; c < n; c += 64) t += row[c] * prev[c];
                        t = wave_sum64(t);
                        if (lane == 0) tmp[r] = t * t;
                    }
                    __syncthreads();
                    if (hl_fbeta > 0.0) {
                        double mx = 0.0;
                        for (int r = tid; r < K; r += QP_NT) mx = fmax(mx, tmp[r]);
                        mx = -block_min(-mx, red);
                        for (int r = tid; r < K; r += QP_NT) lv[off + r] = l0 / (tmp[r] / (mx * hl_fbeta) + 1.0);
                    } else {
                        for (int r = tid; r < K; r += QP_NT) lv[off + r] = 1.0 / (tmp[r] / (beta - 1.0) + 1.0 / lam0);
                    }
                    for (int i = tid; i < off; i += QP_NT) lv[i] = 1.0;
                    __syncthreads();
                } else {
                    // integral: C_j = sum_{r != j} (c_r sqrt(lam_r)) M_rj c_j with c = factor * x, then the positive root
                    // (inversion.py:973-983)
                    const double factor = o == 0 ? 100.0 : (o == 1 ? 10.0 : 1.0);
                    for (int j = wave; j < n; j += QP_NT / 64) {
                        const double cj = factor * prev[j];
                        double t = 0.0;
                        for (int r = lane; r < n; r += 64)
                            if (r != j) t += ((factor * prev[r]) * sqrt(lv[r])) * Mb[(size_t)r * n + j] * cj;
                        t = wave_sum64(t);
                        if (lane == 0) tmp[j] = t;
                    }
                    __syncthreads();
                    for (int j = tid; j < n; j += QP_NT) {
                        const double c = factor * prev[j], Cv = tmp[j];
                        const double aa = beta / 2.0, bb = 0.5 * (2.0 * aa - 2.0) / lam0;
                        const double d = c * c * Mb[(size_t)j * n + j] + 2.0 * bb;
                        const double sg = Cv > 0.0 ? 1.0 : (Cv < 0.0 ? -1.0 : 0.0);
                        double l = (Cv * Cv - sg * Cv * sqrt(4.0 * d * (2.0 * aa - 2.0) + Cv * Cv) + 2.0 * d * (2.0 * aa - 2.0)) / (2.0 * d * d);
                        if (l <= 0.0) l = 1e-15;
                        lv[j] = l;
                    }
                    __syncthreads();
                }
            }
        }
        // P = G + sum_o frac_o * (sqrt(lam_o) M_o sqrt(lam_o))
        for (size_t e = tid; e < (size_t)n * n; e += QP_NT) {
            const int r = (int)(e / n), c = (int)(e - (size_t)r * n);
            double l2 = 0.0;
            for (int o = 0; o < 3; ++o)
                if (a.reg_ord[o] > 0.0) l2 += a.reg_ord[o] * ((sqrt(lam[o * np + r]) * a.base[(size_t)o * n * n + e]) * sqrt(lam[o * np + c]));
            P[e] = G[e] + l2;
        }
        __syncthreads();
        qp_its = qp_box_solve<LDSM>(P, q, a.lo, n, sh, Mw, nullptr, &fun);
        if (qp_its == -3) { flag = -3; break; }
        for (int i = tid; i < n; i += QP_NT) coef[i] = sh[i];
        __syncthreads();
        // cost = 1/2 x.P x + q.x and the relative change of the coefficients
        for (int i = wave; i < n; i += QP_NT / 64) {
            const double *row = P + (size_t)i * n;
            double t = 0.0;
            for (int j = lane; j < n; j += 64) t += row[j] * coef[j];
            t = wave_sum64(t);
            if (lane == 0) tmp[i] = t;
        }
        __syncthreads();
        double c1 = 0.0, dsum = 0.0, dnan = 0.0;
        for (int i = tid; i < n; i += QP_NT) {
            c1 += coef[i] * (0.5 * tmp[i] + q[i]);
            double dl = (coef[i] - prev[i]) / prev[i];
            if (i == 1 && zero_delta1) dl = 0.0;     // (a property of the fit's data part)
            dl = fabs(dl);
            if (dl != dl) dnan += 1.0; else dsum += dl;
        }
        block_sum3(c1, dsum, dnan, red);
        cost = c1;
        if (a.hist_coef) {
            for (int i = tid; i < n; i += QP_NT) {
                a.hist_coef[((size_t)b * a.max_iter + it) * n + i] = coef[i];
                for (int o = 0; o < 3; ++o) a.hist_lam[(((size_t)b * a.max_iter + it) * 3 + o) * n + i] = lam[o * np + i];
            }
            if (tid == 0) { a.hist_fun[(size_t)b * a.max_iter + it] = fun; a.hist_cost[(size_t)b * a.max_iter + it] = cost; }
        }
        if (qp_its == -4) flag |= 4;                    // a QP hit its iteration limit: last iterate used (cvxopt: status "unknown")
        ++it;
        if (!a.hyper_lambda) break;
        // np.mean(np.abs(delta)) < xtol: a NaN (0/0) makes the comparison false, an inf makes the mean inf
        if (dnan == 0.0 && dsum / (double)n < a.xtol) { flag |= 1; break; }
    }
    for (int i = tid; i < n; i += QP_NT) {
        a.coef[(size_t)b * n + i] = coef[i];
        for (int o = 0; o < 3; ++o) a.lam[((size_t)b * 3 + o) * n + i] = lam[o * np + i];
    }
    if (tid == 0) { a.cost[b] = cost; a.fun[b] = fun; a.iters[b] = it; a.flags[b] = flag; }
}

// ---- debug (tests): the production form-KKT loop, ladder, factorisation and substitutions on supplied data ---------------------
// One workgroup per problem b: M = sym(P[b]) + diag(dg[b]) through qp_factor, then chol_solve_blocked once per right-hand side
// on that factor.  LDS as qp_box_solve lays it out (v in the slot of x, 1 / diag in the slot of rhs, diag, red, triangle).
// ok, rungs, reg [nb]; a problem that does not factor writes nothing else.  L [nb][n][n]: the factor as a dense lower triangle,
// diag[] on its diagonal, zeros above; piv [nb][n]: what M(j, j) keeps; sol [nb][nrhs][n].
template <bool LDSM>
__global__ __launch_bounds__(QP_NT) void qp_factor_solve_kernel(const double *__restrict__ Pall, const double *__restrict__ dgall, int n,
                                                                const double *__restrict__ rhsall, int nrhs, double *__restrict__ work,
                                                                int *__restrict__ okall, int *__restrict__ rungsall, double *__restrict__ regall,
                                                                double *__restrict__ Lall, double *__restrict__ pivall, double *__restrict__ solall)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int np = (n + 1) & ~1;
    const size_t msize = (size_t)n * (n + 1) / 2;
    double *v = sh, *rd = sh + 4 * np, *diag = sh + QP_NVEC * np, *red = diag + np;
    double *M = LDSM ? red + 32 : work + (size_t)b * msize;
    const double *P = Pall + (size_t)b * n * n, *dg = dgall + (size_t)b * n;
    QpProf pf;
    double reg;
    int rungs;
    const bool ok = qp_factor<LDSM>(P, n, M, diag, red, [&](int i) { return dg[i]; }, pf, &reg, &rungs);
    if (tid == 0) { okall[b] = ok ? 1 : 0; rungsall[b] = rungs; regall[b] = reg; }
    if (!ok) return;
    double *L = Lall + (size_t)b * n * n;
    for (size_t e = tid; e < (size_t)n * n; e += QP_NT) {
        const int i = (int)(e / n), j = (int)(e - (size_t)i * n);
        L[e] = j < i ? M[cidx(i, j, n)] : (j == i ? diag[i] : 0.0);
    }
    for (int i = tid; i < n; i += QP_NT) pivall[(size_t)b * n + i] = M[cidx(i, i, n)];
    for (int r = 0; r < nrhs; ++r) {
        const size_t o = ((size_t)b * nrhs + r) * n;
        for (int i = tid; i < n; i += QP_NT) v[i] = rhsall[o + i];
        __syncthreads();
        chol_solve_blocked<LDSM>(M, diag, n, v, rd, red);
        for (int i = tid; i < n; i += QP_NT) solall[o + i] = v[i];
        __syncthreads();
    }
}

// The dynamic LDS of a kernel around qp_box_solve and whether the packed KKT triangle lives there: the QP's vectors, diag and
// reduction scratch, `extra` doubles of the caller's own, and the triangle when all of it stays within the 160 KiB of a workgroup
// less QP_STATIC_LDS (chol_packed's static tile, rounded up).  fits: the launch is possible at all.
constexpr size_t QP_STATIC_LDS = 2560, QP_LDS_TOTAL = 160 * 1024;
QpLds qp_lds_plan(int n, size_t extra)
{
    const int np = (n + 1) & ~1;
    const size_t msize = (size_t)n * (n + 1) / 2;
    const size_t vec = (size_t)(QP_NVEC + 1) * np + 32 + extra;
    QpLds r;
    r.in_lds = (vec + msize) * sizeof(double) <= QP_LDS_TOTAL - QP_STATIC_LDS;
    r.bytes = (vec + (r.in_lds ? msize : 0)) * sizeof(double);
    r.fits = r.bytes + QP_STATIC_LDS <= QP_LDS_TOTAL;
    return r;
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_qp_box_batch(const double *P, const double *q, const double *lo, int n, int nb, double *x,
                      double *primal_objective, int *iterations)
{
    if (!P || !q || !x || n < 1 || nb < 1) { set_error("bdrt_qp_box_batch: bad arguments"); return -1; }
    bind_process_device();
    const size_t msize = (size_t)n * (n + 1) / 2;
    const QpLds plan = qp_lds_plan(n, 0);
    const bool in_lds = plan.in_lds;
    const size_t lds = plan.bytes;
    if (!plan.fits) { set_error("bdrt_qp_box_batch: n = %d too large", n); return -2; }
    DevBuf<double> dP, dq, dlo, dx, dobj, dwork;
    DevBuf<int> dit;
    if (upload(dP, P, (size_t)nb * n * n) || upload(dq, q, (size_t)nb * n) || (lo && upload(dlo, lo, (size_t)n))) return -10;
    BDRT_HIP(dx.alloc((size_t)nb * n));
    BDRT_HIP(dobj.alloc((size_t)nb));
    BDRT_HIP(dit.alloc((size_t)nb));
    if (!in_lds) BDRT_HIP(dwork.alloc((size_t)nb * msize));
    static LdsAttrCache attr_cache;
    BDRT_HIP(attr_cache.ensure(lds, [&]() {
        hipError_t e = hipFuncSetAttribute((const void *)qp_box_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *)qp_box_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        return e;
    }));
    if (in_lds)
        hipLaunchKernelGGL(qp_box_kernel<true>, dim3(nb), dim3(QP_NT), lds, 0, dP.p, dq.p, dlo.p, n, dx.p, dobj.p, dit.p, dwork.p);
    else
        hipLaunchKernelGGL(qp_box_kernel<false>, dim3(nb), dim3(QP_NT), lds, 0, dP.p, dq.p, dlo.p, n, dx.p, dobj.p, dit.p, dwork.p);
    BDRT_HIP(hipGetLastError());
    BDRT_HIP(hipDeviceSynchronize());
    std::vector<int> its(nb);
    if (download(x, dx.p, (size_t)nb * n) || download(its.data(), dit.p, (size_t)nb) ||
        (primal_objective && download(primal_objective, dobj.p, (size_t)nb)))
        return -10;
    int worst = 0;
    for (int b = 0; b < nb; ++b) {
        if (iterations) iterations[b] = its[b];
        if (its[b] == -3) worst = -3;                              // a non-PD problem outranks an iteration limit elsewhere
        else if (its[b] < 0 && worst == 0) worst = its[b];
    }
    if (worst == -3) { set_error("bdrt_qp_box_batch: KKT matrix not positive definite"); return -3; }
    if (worst == -4) { set_error("bdrt_qp_box_batch: iteration limit"); return -4; }
    return 0;
}


int bdrt_ridge_ex(const bdrt_ridge_options *opt, const unsigned char *zero_delta1_g, const double *hl_fbeta_b, int nb, int ng,
                  const double *G, const double *qbase, const int *gsel, const double *base, const double *Ls, const double *lo,
                  const double *lambda0, const double *lam0s, const double *betas, const double *x0, double *coef, double *lam,
                  double *cost, double *fun, int *iters, int *flags, double *hist_coef, double *hist_lam, double *hist_fun,
                  double *hist_cost)
{
    if (!opt || !zero_delta1_g || !hl_fbeta_b || nb < 1 || ng < 1 || !G || !qbase || !gsel || !base || !lambda0 || !lam0s || !betas || !coef || opt->n < 1 ||
        opt->max_iter < 1 || (opt->penalty == 0 && opt->hyper_lambda && (!Ls || opt->K < 1)) || opt->off < 0 || opt->off > opt->n) {
        set_error("bdrt_ridge: bad arguments");
        return -1;
    }
    for (int b = 0; b < nb; ++b) if (gsel[b] < 0 || gsel[b] >= ng) { set_error("bdrt_ridge: gsel out of range"); return -1; }
    if (opt->penalty == 0 && opt->hyper_lambda && opt->off + opt->K != opt->n) { set_error("bdrt_ridge: off + K must equal n"); return -1; }
    bind_process_device();
    const int n = opt->n, K = opt->K, np = (n + 1) & ~1, mi = opt->max_iter;
    const size_t msize = (size_t)n * (n + 1) / 2;
    const QpLds plan = qp_lds_plan(n, (size_t)6 * np + 32 + 2);       // ridge_kernel's coef, prev, lam[3], tmp, red (+ alignment)
    const bool in_lds = plan.in_lds;
    const size_t lds = plan.bytes;
    if (!plan.fits) { set_error("bdrt_ridge: n = %d too large", n); return -2; }
    // inputs: a fresh buffer each, filled from the host; outputs and work space: allocated only
    DevBuf<double> dG, dqbase, dfb, dbase, dLs, dlo, dlam0, dlam0s, dbetas, dx0, dPwork, dMwork, dcoef, dlam, dcost, dfun, dhc, dhl, dhf, dhk;
    DevBuf<int> dgsel, diters, dflags;
    DevBuf<unsigned char> dzd;
    // (every size is positive by the checks above -- n, nb, ng, max_iter >= 1 -- except that of Ls, which a caller may pass with
    //  K == 0 where the kernel does not read it: one element then, the kernel's pointer stays non-null)
    if (Ls && K == 0) BDRT_HIP(dLs.alloc(1));
    if (upload(dG, G, (size_t)ng * n * n) || upload(dqbase, qbase, (size_t)ng * n) || upload(dgsel, gsel, (size_t)nb) ||
        upload(dzd, zero_delta1_g, (size_t)ng) || upload(dfb, hl_fbeta_b, (size_t)nb) || upload(dbase, base, (size_t)3 * n * n) ||
        (Ls && K != 0 && upload(dLs, Ls, (size_t)3 * K * n)) || (lo && upload(dlo, lo, (size_t)n)) ||
        upload(dlam0, lambda0, (size_t)nb) || upload(dlam0s, lam0s, (size_t)nb * 3) || upload(dbetas, betas, (size_t)nb * 3) ||
        (x0 && upload(dx0, x0, (size_t)nb * n)))
        return -10;
    const bool hist = hist_coef && hist_lam && hist_fun && hist_cost;
    BDRT_HIP(dPwork.alloc((size_t)nb * n * n));
    if (!in_lds) BDRT_HIP(dMwork.alloc((size_t)nb * msize));
    BDRT_HIP(dcoef.alloc((size_t)nb * n));
    BDRT_HIP(dlam.alloc((size_t)nb * 3 * n));
    BDRT_HIP(dcost.alloc((size_t)nb));
    BDRT_HIP(dfun.alloc((size_t)nb));
    BDRT_HIP(diters.alloc((size_t)nb));
    BDRT_HIP(dflags.alloc((size_t)nb));
    if (hist) {
        BDRT_HIP(dhc.alloc((size_t)nb * mi * n));
        BDRT_HIP(dhl.alloc((size_t)nb * mi * 3 * n));
        BDRT_HIP(dhf.alloc((size_t)nb * mi));
        BDRT_HIP(dhk.alloc((size_t)nb * mi));
        BDRT_HIP(hipMemset(dhf, 0, (size_t)nb * mi * sizeof(double)));
        BDRT_HIP(hipMemset(dhk, 0, (size_t)nb * mi * sizeof(double)));
    }
    RidgeArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.K = K; a.off = opt->off; a.penalty = opt->penalty; a.max_iter = mi; a.hyper_lambda = opt->hyper_lambda;
    a.xtol = opt->xtol;
    for (int o = 0; o < 3; ++o) a.reg_ord[o] = opt->reg_ord[o];
    a.G = dG; a.qbase = dqbase; a.gsel = dgsel; a.zero_delta1_g = dzd; a.hl_fbeta_b = dfb; a.base = dbase; a.Ls = dLs; a.lo = dlo;
    a.lambda0 = dlam0; a.lam0s = dlam0s; a.betas = dbetas; a.x0 = dx0; a.Pwork = dPwork; a.Mwork = dMwork; a.coef = dcoef; a.lam = dlam;
    a.cost = dcost; a.fun = dfun; a.iters = diters; a.flags = dflags; a.hist_coef = dhc; a.hist_lam = dhl; a.hist_fun = dhf; a.hist_cost = dhk;
    static LdsAttrCache attr_cache;
    BDRT_HIP(attr_cache.ensure(lds, [&]() {
        hipError_t e = hipFuncSetAttribute((const void *)ridge_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *)ridge_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        return e;
    }));
    { const int on = getenv("BDRT_QP_PROF") ? 1 : 0; static int was = 0; if (on != was) { BDRT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_qp_prof_on), &on, sizeof(on))); was = on; } }
    if (in_lds) hipLaunchKernelGGL(ridge_kernel<true>, dim3(nb), dim3(QP_NT), lds, 0, a);
    else hipLaunchKernelGGL(ridge_kernel<false>, dim3(nb), dim3(QP_NT), lds, 0, a);
    BDRT_HIP(hipGetLastError());
    BDRT_HIP(hipDeviceSynchronize());
    if (getenv("BDRT_QP_PROF")) {
        long long h[8] = {0}, z[8] = {0};
        BDRT_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_qp_prof), sizeof(h)));
        BDRT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_qp_prof), z, sizeof(z)));
        fprintf(stderr, "[bdrt qp prof] n %d, fit 0: %lld interior-point iterations; core cycles: form KKT %lld, factor %lld (diagonal blocks %lld, panels %lld, trailing %lld), triangular solves %lld, other %lld\n",
                n, h[4], h[0], h[1], h[5], h[6], h[7], h[2], h[3]);
    }
    std::vector<int> hfl(nb);
    if (download(coef, dcoef.p, (size_t)nb * n) || (lam && download(lam, dlam.p, (size_t)nb * 3 * n)) || (cost && download(cost, dcost.p, (size_t)nb)) ||
        (fun && download(fun, dfun.p, (size_t)nb)) || download(hfl.data(), dflags.p, (size_t)nb) || (iters && download(iters, diters.p, (size_t)nb)))
        return -10;
    if (flags) memcpy(flags, hfl.data(), (size_t)nb * sizeof(int));
    if (hist && (download(hist_coef, dhc.p, (size_t)nb * mi * n) || download(hist_lam, dhl.p, (size_t)nb * mi * 3 * n) ||
                 download(hist_fun, dhf.p, (size_t)nb * mi) || download(hist_cost, dhk.p, (size_t)nb * mi)))
        return -10;
    for (int b = 0; b < nb; ++b)
        if (hfl[b] == -3) { set_error("bdrt_ridge: KKT matrix of fit %d not positive definite", b); return -3; }
    return 0;
}

// the entry with one flag word and one hl_fbeta per launch: bit g of opt->zero_delta1 for the data parts g < 31 (further
// parts: not set), opt->hl_fbeta for every fit
int bdrt_ridge(const bdrt_ridge_options *opt, int nb, int ng, const double *G, const double *qbase, const int *gsel,
               const double *base, const double *Ls, const double *lo, const double *lambda0, const double *lam0s,
               const double *betas, const double *x0, double *coef, double *lam, double *cost, double *fun, int *iters,
               int *flags, double *hist_coef, double *hist_lam, double *hist_fun, double *hist_cost)
{
    if (!opt || nb < 1 || ng < 1) { set_error("bdrt_ridge: bad arguments"); return -1; }
    std::vector<unsigned char> zd((size_t)ng, 0);
    for (int g = 0; g < ng && g < 31; ++g) zd[g] = (unsigned char)((opt->zero_delta1 >> g) & 1);
    std::vector<double> fb((size_t)nb, opt->hl_fbeta);
    return bdrt_ridge_ex(opt, zd.data(), fb.data(), nb, ng, G, qbase, gsel, base, Ls, lo, lambda0, lam0s, betas, x0, coef, lam, cost,
                         fun, iters, flags, hist_coef, hist_lam, hist_fun, hist_cost);
}

int bdrt_debug_qp_factor_solve(const double *P, const double *dg, int n, int nb, int place, const double *rhs, int nrhs,
                               bdrt_qp_factor_record *rec, double *L_out, double *piv_out, double *sol_out)
{
    if (!P || !dg || n < 1 || nb < 1 || (place != 0 && place != 1) || nrhs < 0 || (nrhs > 0 && (!rhs || !sol_out)) || !rec) {
        set_error("bdrt_debug_qp_factor_solve: bad arguments");
        return -1;
    }
    bind_process_device();
    const size_t msize = (size_t)n * (n + 1) / 2, nn = (size_t)n * n;
    const QpLds plan = qp_lds_plan(n, 0);
    if (!plan.fits || (place == 0 && !plan.in_lds)) {
        set_error("bdrt_debug_qp_factor_solve: the triangle of n = %d does not fit in LDS", n);
        return -2;
    }
    const bool in_lds = place == 0;
    const size_t lds = in_lds ? plan.bytes : plan.bytes - (plan.in_lds ? msize * sizeof(double) : 0);
    DevBuf<double> dP, ddg, drhs, dwork, dreg, dL, dpiv, dsol;
    DevBuf<int> dok, drungs;
    if (upload(dP, P, (size_t)nb * nn) || upload(ddg, dg, (size_t)nb * n) || (nrhs > 0 && upload(drhs, rhs, (size_t)nb * nrhs * n))) return -10;
    if (!in_lds) BDRT_HIP(dwork.alloc((size_t)nb * msize));
    BDRT_HIP(dok.alloc((size_t)nb));
    BDRT_HIP(drungs.alloc((size_t)nb));
    BDRT_HIP(dreg.alloc((size_t)nb));
    BDRT_HIP(dL.alloc((size_t)nb * nn));
    BDRT_HIP(dpiv.alloc((size_t)nb * n));
    if (nrhs > 0) BDRT_HIP(dsol.alloc((size_t)nb * nrhs * n));
    static LdsAttrCache attr_cache;
    BDRT_HIP(attr_cache.ensure(lds, [&]() {
        hipError_t e = hipFuncSetAttribute((const void *)qp_factor_solve_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *)qp_factor_solve_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        return e;
    }));
    if (in_lds)
        hipLaunchKernelGGL(qp_factor_solve_kernel<true>, dim3(nb), dim3(QP_NT), lds, 0, dP.p, ddg.p, n, drhs.p, nrhs, dwork.p, dok.p, drungs.p,
                           dreg.p, dL.p, dpiv.p, dsol.p);
    else
        hipLaunchKernelGGL(qp_factor_solve_kernel<false>, dim3(nb), dim3(QP_NT), lds, 0, dP.p, ddg.p, n, drhs.p, nrhs, dwork.p, dok.p, drungs.p,
                           dreg.p, dL.p, dpiv.p, dsol.p);
    BDRT_HIP(hipGetLastError());
    BDRT_HIP(hipDeviceSynchronize());
    std::vector<int> ok(nb), rungs(nb);
    std::vector<double> reg(nb);
    if (download(ok.data(), dok.p, (size_t)nb) || download(rungs.data(), drungs.p, (size_t)nb) || download(reg.data(), dreg.p, (size_t)nb)) return -10;
    int bad = -1;
    for (int b = 0; b < nb; ++b) {
        rec[b].ok = ok[b]; rec[b].rungs = rungs[b]; rec[b].reg = reg[b];
        if (!ok[b]) { if (bad < 0) bad = b; continue; }             // (the caller's arrays of this problem stay as they are)
        if ((L_out && download(L_out + (size_t)b * nn, dL.p + (size_t)b * nn, nn)) ||
            (piv_out && download(piv_out + (size_t)b * n, dpiv.p + (size_t)b * n, (size_t)n)) ||
            (nrhs > 0 && download(sol_out + (size_t)b * nrhs * n, dsol.p + (size_t)b * nrhs * n, (size_t)nrhs * n)))
            return -10;
    }
    if (bad >= 0) { set_error("bdrt_debug_qp_factor_solve: KKT matrix of problem %d not positive definite", bad); return -3; }
    return 0;
}

}  // extern "C"
