// bdrt_powerscale.hip -- power-scaling prior and likelihood sensitivity of HMC draws on the device (include/bdrt.h section (4d)).
//
// Kallioinen, Paananen, Buerkner, Vehtari (2023): raise the prior, then the likelihood, to a power alpha near 1, re-weight the
// draws by Pareto-smoothed importance sampling and measure how far every marginal posterior moves by the cumulative
// Jensen-Shannon distance between its ECDF and the re-weighted one.  Definitions: tests/powerscale_numpy.py (the yardstick).
// No refit: the batch evaluator gives the Jacobian-free log density, the constrained parameters, Z_hat and sigma_tot of every
// draw (the launch of LooStage::eval, here with the spectrum of every row), loglik_kernel the pointwise log-likelihoods.
//
//   ps_sums_kernel     one wave per draw row: L_lik = the row of ll [rows][U] summed (lanes stride the row, then a butterfly),
//                      L_pri = lp0 - L_lik                                                          -> L [G][2][S]
//   ps_weights_kernel  one workgroup (8 waves) per (fit, component, alpha): tests/psis_numpy.psislw of (alpha - 1) L
//     1  the log ratios go to LDS; max, min; x = ratio - max
//     2  the (M+1)-th largest x by radix select; cutoff = max(that, log DBL_MIN)                    (bdrt_psis.h)
//     3  the draws above the cutoff leave their INDEX in the tail buffer; their values are gathered and sorted by (value,
//        draw index): the stable order of the numpy statement, and a total order, so the compaction order (the one thing
//        atomics decide) is erased
//     4  Zhang-Stephens fit, smoothed tail values scattered back to their draws                     (bdrt_psis.h)
//     5  log-sum-exp over all S in a fixed order; log weights and weights                           -> w [G][4][S], k, n_tail
//   ps_cjs_kernel      one workgroup (8 waves) per (fit, column):
//     1  the column goes to LDS; a 16-bit index is sorted by (value, index) (bitonic_any)
//     2  the gaps d_j = x_(j+1) - x_(j) replace the column, through registers: the one gathered LDS pass; everything after it
//        reads LDS with unit stride
//     3  for each of the four weight vectors: every wave owns one contiguous segment of the sorted positions; it gathers w
//        through the index (from HBM / L2: at 8192 draws the LDS has no room for a weight vector), scans 64 positions at a
//        time (Hillis-Steele over the lanes) with a running carry, and leaves the segment's running sums in the work series;
//        the eight segment totals are added from wave 0 upward; a second sweep forms the eight sums of the distance on the
//        distribution functions P, Q and on the survival functions 1 - P, 1 - Q
//     -> cjs2 [G][C][4]
// LDS per draw of ps_cjs_kernel: 8 B column + 8 B work series + 2 B index, as in bdrt_rank.hip: PS_MAX_DRAWS = 8192 take 144 KiB,
// plus 0.6 KiB of scratch.  No atomics in it; in ps_weights_kernel atomics only count (histogram, compaction).  Every sum has a
// fixed order that depends on S alone, so a column and a fit give the same bits alone or in any batch.  Every product and sum
// is rounded separately, as in the numpy statement.
#include <cfloat>
#include <cmath>

#include "bdrt_host.h"
#include "bdrt_psis.h"

namespace bdrt {

constexpr int PS_NT = LO_NT;                     // 8 waves: the pieces of bdrt_psis.h are written for LO_NT threads
constexpr int PS_NW = LO_NW;
constexpr int PS_MAX_DRAWS = 8192;
constexpr int PS_PER = PS_MAX_DRAWS / PS_NT;     // sorted positions per thread
constexpr int PS_NSUM = 8;

// ll [rows][U], lp [rows] -> L [G][2][S]: plane 0 the prior component, plane 1 the likelihood component
__global__ __launch_bounds__(256) void ps_sums_kernel(const double *__restrict__ ll, const double *__restrict__ lp, size_t rows, int S,
                                                      int U, double *__restrict__ L)
{
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                            // (whole waves leave)
    const double *src = ll + r * (size_t)U;
    double s = 0.0;
    for (int j = lane; j < U; j += 64) s += src[j];
    s = wave_sum(s);
    if (lane == 0) {
        const size_t g = r / S, t = r - g * S;
        L[(2 * g) * S + t] = lp[r] - s;
        L[(2 * g + 1) * S + t] = s;
    }
}

struct PsWeightArgs {
    const double *L;                             // [G][2][S] device
    int S, cap, M;                               // cap = ceil(S / 5); M: tail length at reff = 1
    double am1[2];                               // alpha - 1, lower and upper
    double log_dbl_min;
    double *lw, *w;                              // [G][4][S] device, either may be null
    double *khat;                                // [G][4]
    int *ntail;
};

__global__ __launch_bounds__(PS_NT) void ps_weights_kernel(PsWeightArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int S = a.S;
    const size_t b = blockIdx.x, g = b >> 2;
    const int comp = (int)(b >> 1) & 1;
    double *col = lds;                                                // [S]      log ratios, then x, tail entries smoothed
    double *tail = col + S;                                           // [cap] each
    double *y = tail + a.cap;
    double *sm = y + a.cap;
    double *red = sm + a.cap;                                         // [PS_NW]
    double *bj = red + PS_NW;                                         // [LO_MAX_M] each
    double *kj = bj + LO_MAX_M;
    double *Lj = kj + LO_MAX_M;
    double *wj = Lj + LO_MAX_M;
    double *sc = wj + LO_MAX_M;                                       // [4]
    int *hist = (int *)(sc + 4);                                      // [256]
    int *si = hist + 256;                                             // [4]
    int *idx = si + 4;                                                // [cap]    draw indices of the tail
    const double *src = a.L + (2 * g + comp) * (size_t)S;
    const double scale = a.am1[b & 1];
    double *lw = a.lw ? a.lw + b * (size_t)S : nullptr, *w = a.w ? a.w + b * (size_t)S : nullptr;

    // ---- 1: log ratios to LDS; extremes
    int bad = 0;
    double mx = -INFINITY, mn = INFINITY;
    for (int s = tid; s < S; s += PS_NT) {
        const double l = src[s], v = scale * l;
        bad |= !isfinite(l);
        col[s] = v;
        mx = fmax(mx, v);
        mn = fmin(mn, v);
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int s = tid; s < S; s += PS_NT) {
            if (lw) lw[s] = NAN;
            if (w) w[s] = NAN;
        }
        if (tid == 0) { a.khat[b] = NAN; a.ntail[b] = 0; }
        return;
    }
    mx = block_max<PS_NW>(mx, red);
    mn = -block_max<PS_NW>(-mn, red);
    const bool flat = mx == mn;                                       // all draws equal: the weights stay raw and equal
    __syncthreads();
    for (int s = tid; s < S; s += PS_NT) col[s] = col[s] - mx;
    int n = 0;
    double khat = INFINITY;
    int nan = 0;
    if (!flat) {
        // ---- 2: cutoff
        const double cutoff = fmax(lo_radix_select(col, S, a.M + 1, hist, si), a.log_dbl_min);
        const double ecut = exp(cutoff);
        // ---- 3: tail indices; values gathered and sorted by (value, draw index)
        __syncthreads();
        if (tid == 0) si[2] = 0;
        __syncthreads();
        for (int base = 0; base < S; base += PS_NT) {
            const int s = base + tid;
            const bool up = s < S && col[s] > cutoff;
            const unsigned long long um = __ballot(up);
            if (um) {
                const int first = __ffsll((long long)um) - 1;
                int pos = 0;
                if (lane == first) pos = atomicAdd(&si[2], __popcll(um));
                pos = __shfl(pos, first, 64) + __popcll(um & ((1ull << lane) - 1ull));
                if (up && pos < a.cap) idx[pos] = s;
            }
        }
        __syncthreads();
        n = min(si[2], a.cap);
        for (int r = tid; r < n; r += PS_NT) tail[r] = col[idx[r]];
        bitonic_any<PS_NT>(n, [&](int i, int q) {
            const double u = tail[i], v = tail[q];
            const int iu = idx[i], iv = idx[q];
            if (u > v || (u == v && iu > iv)) { tail[i] = v; tail[q] = u; idx[i] = iv; idx[q] = iu; }
        });
        // ---- 4: generalised-Pareto fit; smoothed values back to their draws
        double sigma = NAN;
        if (n > 4) lo_pareto_fit(tail, y, n, ecut, bj, kj, Lj, wj, sc, red, khat, sigma);
        if (n > 4 && isfinite(khat)) {
            for (int r = tid; r < n; r += PS_NT) {
                const double v = lo_smoothed(r, n, khat, sigma, ecut);
                nan |= (v != v);
                col[idx[r]] = v;
            }
        }
    }
    // ---- 5: normalise (a smoothed value that is NaN makes the maximum NaN, as numpy's max does, and with it every weight)
    nan = __syncthreads_or(nan);
    double m = -INFINITY;
    for (int s = tid; s < S; s += PS_NT) m = fmax(m, col[s]);
    m = block_max<PS_NW>(m, red);
    if (nan) m = NAN;
    double se = 0.0;
    for (int s = tid; s < S; s += PS_NT) se += exp(col[s] - m);
    se = block_sum<PS_NW>(se, red);
    const double lse = m + log(se);
    for (int s = tid; s < S; s += PS_NT) {
        const double v = col[s] - lse;
        if (lw) lw[s] = v;
        if (w) w[s] = exp(v);
    }
    if (tid == 0) { a.khat[b] = khat; a.ntail[b] = n; }
}

struct PsCjsArgs {
    const double *X;                             // element (g, s, c) at X[g * group_stride + s * row_stride + c * col_stride]
    size_t group_stride, row_stride, col_stride;
    const double *W;                             // [G][4][S] device (w_shared: [4][S], the same for every group)
    int w_shared;
    int S, C;
    double c_ln2;                                // 1 / (2 ln 2)
    double *out;                                 // [G][C][4]
};

// x (log2 x - lm), 0 at x = 0
__device__ inline double ps_xlog(double x, double lm) { return x > 0.0 ? x * (log2(x) - lm) : 0.0; }

// h(P, Q) from (I_P, I_Q, sum d P (log2 P - log2 M), sum d Q (log2 Q - log2 M))
__device__ inline double ps_h(double ip, double iq, double sp, double sq, double c)
{
    const double pq = sp + c * (iq - ip), qp = sq + c * (ip - iq), den = ip + iq;
    if (!(den > 0.0)) return 0.0;
    return fmax(0.0, (pq + qp) / den);
}

__global__ __launch_bounds__(PS_NT) void ps_cjs_kernel(PsCjsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int S = a.S;
    const size_t g = blockIdx.y, c = blockIdx.x;
    double *val = lds;                                                // [S]   the column, then the gaps of the sorted column
    double *wrk = val + S;                                            // [S]   running sums of the gathered weights
    double *tot = wrk + S;                                            // [PS_NW]  segment totals
    double *red = tot + PS_NW;                                        // [PS_NSUM][PS_NW]
    unsigned short *idx = (unsigned short *)(red + PS_NSUM * PS_NW);  // [S]
    const double *Xc = a.X + g * a.group_stride + c * a.col_stride;
    double *out = a.out + (g * a.C + c) * 4;

    // ---- 1: the column to LDS; sort the index by (value, index)
    int nonfinite = 0;
    for (int i = tid; i < S; i += PS_NT) {
        const double v = Xc[(size_t)i * a.row_stride];
        nonfinite |= !isfinite(v);
        val[i] = v;
        idx[i] = (unsigned short)i;
    }
    nonfinite = __syncthreads_or(nonfinite);
    if (nonfinite) {
        if (tid < 4) out[tid] = NAN;
        return;
    }
    bitonic_any<PS_NT>(S, [&](int i, int q) {
        const unsigned short ia = idx[i], ib = idx[q];
        const double u = val[ia], v = val[ib];
        if (u > v || (u == v && ia > ib)) { idx[i] = ib; idx[q] = ia; }
    });
    // ---- 2: gaps of the sorted column, through registers (val[S - 1] = 0 is never read)
    {
        double dr[PS_PER];
#pragma unroll
        for (int k = 0; k < PS_PER; ++k) {
            const int p = tid + k * PS_NT;
            dr[k] = p + 1 < S ? val[idx[p + 1]] - val[idx[p]] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PS_PER; ++k) {
            const int p = tid + k * PS_NT;
            if (p < S) val[p] = dr[k];
        }
        __syncthreads();
    }
    // ---- 3: the four weight vectors in turn
    const int seg = ((S + PS_NT - 1) / PS_NT) * 64;                  // positions per wave: a multiple of 64
    const int p0 = min(S, wv * seg), p1 = min(S, p0 + seg);
    const double dS = (double)S;
    for (int k = 0; k < 4; ++k) {
        const double *Wk = a.W + ((a.w_shared ? 0 : g * 4) + k) * (size_t)S;
        int wbad = 0;
        double carry = 0.0;
        for (int base = p0; base < p1; base += 64) {
            const int p = base + lane;
            double v = p < p1 ? Wk[idx[p]] : 0.0;
            wbad |= !isfinite(v);
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double t = __shfl_up(v, o, 64);
                if (lane >= o) v += t;
            }
            v = carry + v;
            if (p < p1) wrk[p] = v;
            carry = __shfl(v, 63, 64);
        }
        if (lane == 0) tot[wv] = carry;
        wbad = __syncthreads_or(wbad);                                // (publishes tot)
        double pre = 0.0;
        for (int i = 0; i < wv; ++i) pre += tot[i];
        double s[PS_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int pe = min(p1, S - 1);
        for (int base = p0; base < pe; base += 64) {
            const int p = base + lane;
            if (p < pe) {
                const double d = val[p];
                const double P = (double)(p + 1) / dS, Q = fmin(1.0, pre + wrk[p]);
                const double lm = log2(0.5 * (P + Q));
                s[0] += d * P;
                s[1] += d * Q;
                s[2] += d * ps_xlog(P, lm);
                s[3] += d * ps_xlog(Q, lm);
                const double Pc = 1.0 - P, Qc = 1.0 - Q;
                const double lc = log2(0.5 * (Pc + Qc));
                s[4] += d * Pc;
                s[5] += d * Qc;
                s[6] += d * ps_xlog(Pc, lc);
                s[7] += d * ps_xlog(Qc, lc);
            }
        }
        block_sums<PS_NSUM>(s, red);
        if (tid == 0) {
            const double h1 = ps_h(s[0], s[1], s[2], s[3], a.c_ln2), h2 = ps_h(s[4], s[5], s[6], s[7], a.c_ln2);
            out[k] = wbad ? NAN : fmax(h1, h2);
        }
    }
}

static size_t ps_weights_lds_bytes(int S, int cap)
{
    return ((size_t)S + 3 * (size_t)cap + PS_NW + 4 * LO_MAX_M + 4) * sizeof(double) + (256 + 4 + (size_t)cap) * sizeof(int);
}

static size_t ps_cjs_lds_bytes(int S)
{
    return ((size_t)2 * S + PS_NW + PS_NSUM * PS_NW) * sizeof(double) + (((size_t)S + 7) & ~(size_t)7) * sizeof(unsigned short);
}
static_assert(((size_t)2 * PS_MAX_DRAWS + PS_NW + PS_NSUM * PS_NW) * 8 + (size_t)PS_MAX_DRAWS * 2 <= 160 * 1024,
              "ps_cjs_kernel: the column, the work series and the index of PS_MAX_DRAWS draws must fit the LDS of a CU");
static_assert(((size_t)PS_MAX_DRAWS + 3 * ((PS_MAX_DRAWS + 4) / 5) + PS_NW + 4 * LO_MAX_M + 4) * 8 + (256 + 4 + (PS_MAX_DRAWS + 4) / 5) * 4 <=
                  160 * 1024,
              "ps_weights_kernel: the log ratios and the tail of PS_MAX_DRAWS draws must fit the LDS of a CU");
static_assert(PS_MAX_DRAWS <= 65536, "ps_cjs_kernel sorts a 16-bit index");

static int ps_check_draws(const char *who, long S)
{
    if (S < 2) { set_error("%s: at least 2 draws are needed", who); return -1; }
    if (S > PS_MAX_DRAWS) { set_error("%s: %ld draws per column, the kernel holds at most %d", who, S, PS_MAX_DRAWS); return -2; }
    return 0;
}

static int ps_check_alphas(const char *who, double alpha_lo, double alpha_hi)
{
    if (!(alpha_lo > 0.0) || !(alpha_lo < 1.0) || !(alpha_hi > 1.0) || !std::isfinite(alpha_hi)) {
        set_error("%s: the powers need 0 < alpha_lo < 1 < alpha_hi", who);
        return -1;
    }
    return 0;
}

// ---- device-pointer cores: each enqueues on `stream` and returns; the caller synchronises
static int ps_sums_device(const double *dLl, const double *dLp, size_t rows, int S, int U, double *dL, hipStream_t stream)
{
    const size_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffffull) { set_error("bdrt_powerscale: too many rows"); return -2; }
    hipLaunchKernelGGL(ps_sums_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dLl, dLp, rows, S, U, dL);
    BDRT_HIP(hipGetLastError());
    return 0;
}

// dL [G][2][S] -> dLw, dW [G][4][S] (either may be null), dK [G][4], dNtail [G][4]
static int ps_weights_device(const char *who, const double *dL, int G, int S, double alpha_lo, double alpha_hi, double *dLw, double *dW,
                             double *dK, int *dNtail, hipStream_t stream)
{
    std::vector<int> M;
    if (loo_tail_lengths(who, S, 1, nullptr, M)) return -1;
    const int cap = (S + 4) / 5;
    const size_t lds = ps_weights_lds_bytes(S, cap);
    static LdsAttrCache cache;
    BDRT_HIP(cache.ensure(lds, [&]() {
        return hipFuncSetAttribute((const void *)ps_weights_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }));
    PsWeightArgs a;
    a.L = dL; a.S = S; a.cap = cap; a.M = M[0];
    a.am1[0] = alpha_lo - 1.0; a.am1[1] = alpha_hi - 1.0;
    a.log_dbl_min = std::log(DBL_MIN);
    a.lw = dLw; a.w = dW; a.khat = dK; a.ntail = dNtail;
    if ((size_t)G * 4 > 0x7fffffffull) { set_error("%s: too many fits", who); return -2; }
    hipLaunchKernelGGL(ps_weights_kernel, dim3((unsigned)G * 4), dim3(PS_NT), lds, stream, a);
    BDRT_HIP(hipGetLastError());
    return 0;
}

// columns (g, s, c) of dX by strides, dW [G][4][S] (w_shared: [4][S]) -> dOut [G][C][4]
static int ps_cjs_device(const double *dX, size_t group_stride, size_t row_stride, size_t col_stride, const double *dW, int w_shared,
                         int G, int S, int C, double *dOut, hipStream_t stream)
{
    const size_t lds = ps_cjs_lds_bytes(S);
    static LdsAttrCache cache;
    BDRT_HIP(cache.ensure(lds, [&]() {
        return hipFuncSetAttribute((const void *)ps_cjs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }));
    PsCjsArgs a;
    a.group_stride = group_stride; a.row_stride = row_stride; a.col_stride = col_stride;
    a.w_shared = w_shared; a.S = S; a.C = C; a.c_ln2 = 1.0 / (2.0 * std::log(2.0));
    return for_grid_y_chunks(G, [&](int g0, int gn) {
        a.X = dX + (size_t)g0 * group_stride;
        a.W = w_shared ? dW : dW + (size_t)g0 * 4 * S;
        a.out = dOut + (size_t)g0 * C * 4;
        hipLaunchKernelGGL(ps_cjs_kernel, dim3(C, gn), dim3(PS_NT), lds, stream, a);
    });
}

// The check on draws that are on the device (bdrt_powerscale, bdrt_sampler_powerscale): chunks of groups as loo_of_draws runs
// them (LooStage's buffers; pair and reff_mode of the job are 0).  Outputs on the host: cjs2 [G][D][4], pareto_k, n_tail [G][4];
// L_out [G][2][S] (optional): the two components.
int powerscale_of_draws(const char *who, const LooDraws &j, double alpha_lo, double alpha_hi, double *cjs2, double *pareto_k,
                        int *n_tail, double *L_out)
{
    Problem &P = *j.prob;
    const int S = j.chains * j.n_draws, D = P.dev.D, U = j.ncols;
    const size_t N2 = 2 * (size_t)P.dev.nf;
    LooStage st;
    if (const int rc = st.alloc(j, false, 4 * (size_t)D + 4)) return rc;
    DevBuf<double> dL, dW;
    DevBuf<int> dSpec, dNt;
    BDRT_HIP(dL.alloc((size_t)st.gmax * 2 * S));
    BDRT_HIP(dW.alloc((size_t)st.gmax * 4 * S));
    BDRT_HIP(dNt.alloc((size_t)st.gmax * 4));
    BDRT_HIP(dSpec.alloc((size_t)st.gmax * S));
    std::vector<int> hspec((size_t)st.gmax * S);
    for (int g0 = 0; g0 < j.G; g0 += st.gmax) {
        const int gn = std::min(st.gmax, j.G - g0);
        const size_t rows = (size_t)gn * S;
        for (int g = 0; g < gn; ++g) std::fill(hspec.begin() + (size_t)g * S, hspec.begin() + (size_t)(g + 1) * S, j.spec[g0 + g]);
        if (upload(dSpec.p, hspec.data(), rows, j.stream)) return -10;
        int rc;
        if ((rc = launch_logp_grad(&P, j.draws + (size_t)g0 * S * D, dSpec, (int)rows, 0, st.lp, nullptr, st.par, st.zh, st.sg, j.stream)))
            return rc;
        for (int g = 0; g < gn; ++g)
            BDRT_HIP(hipMemcpyAsync(st.z.p + (size_t)g * U, P.d_Z.p + (size_t)j.spec[g0 + g] * N2 + j.col0, (size_t)U * sizeof(double),
                                    hipMemcpyDeviceToDevice, j.stream));
        double *dCjs = st.out, *dK = st.out.p + (size_t)gn * D * 4;
        if ((rc = loo_loglik_device(st.zh.p + j.col0, st.sg.p + j.col0, st.z, rows, S, U, N2, 0, st.ll, j.stream)) ||
            (rc = ps_sums_device(st.ll, st.lp, rows, S, U, dL, j.stream)) ||
            (rc = ps_weights_device(who, dL, gn, S, alpha_lo, alpha_hi, nullptr, dW, dK, dNt, j.stream)) ||
            (rc = ps_cjs_device(st.par, (size_t)S * D, (size_t)D, 1, dW, 0, gn, S, D, dCjs, j.stream)))
            return rc;
        BDRT_HIP(hipStreamSynchronize(j.stream));                     // (hspec is rewritten by the next chunk)
        if (download(cjs2 + (size_t)g0 * D * 4, dCjs, (size_t)gn * D * 4) || download(pareto_k + (size_t)g0 * 4, dK, (size_t)gn * 4) ||
            download(n_tail + (size_t)g0 * 4, dNt.p, (size_t)gn * 4))
            return -10;
        if (L_out && download(L_out + (size_t)g0 * 2 * S, dL.p, (size_t)gn * 2 * S)) return -10;
    }
    return 0;
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_powerscale_max_draws(void) { return PS_MAX_DRAWS; }

int bdrt_powerscale(bdrt_problem *p, const double *theta, const int *spec, int G, int chains, int n_draws, int col0, int ncols,
                    double alpha_lo, double alpha_hi, size_t chunk_bytes, double *cjs2, double *pareto_k, int *n_tail, double *L_out)
{
    const char *who = "bdrt_powerscale";
    if (!p || !theta || !cjs2 || !pareto_k || !n_tail || G < 1 || chains < 1 || n_draws < 1) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    Problem &P = p->impl;
    const int N2 = 2 * P.dev.nf;
    if (col0 < 0 || ncols < 1 || col0 + ncols > N2) { set_error("%s: bad column range", who); return -1; }
    if (ps_check_alphas(who, alpha_lo, alpha_hi)) return -1;
    const long S = (long)chains * n_draws;
    if (const int rc = ps_check_draws(who, S)) return rc;
    std::vector<int> sp((size_t)G, 0);
    for (int g = 0; g < G; ++g) {
        if (spec) sp[g] = spec[g];
        if (sp[g] < 0 || sp[g] >= P.dev.n_spectra) {
            set_error("%s: spectrum index %d out of range [0,%d) at group %d", who, sp[g], P.dev.n_spectra, g);
            return -1;
        }
    }
    BDRT_HIP(hipSetDevice(P.device));
    BDRT_HIP(hipStreamSynchronize(P.stream));
    DevBuf<double> dTheta;
    if (upload(dTheta, theta, (size_t)G * S * P.dev.D)) return -10;
    LooDraws j = {};
    j.prob = &P; j.draws = dTheta; j.spec = sp.data();
    j.G = G; j.chains = chains; j.n_draws = n_draws;
    j.pair = 0; j.col0 = col0; j.ncols = ncols;
    j.reff_mode = 0; j.reff_in = nullptr; j.chunk_bytes = chunk_bytes; j.stream = P.stream;
    return powerscale_of_draws(who, j, alpha_lo, alpha_hi, cjs2, pareto_k, n_tail, L_out);
}

int bdrt_debug_powerscale_cjs(const double *X, const double *w, int C, int S, double *cjs2)
{
    const char *who = "bdrt_debug_powerscale_cjs";
    if (!X || !w || !cjs2 || C < 1 || C > 65535) { set_error("%s: bad arguments", who); return -1; }
    if (const int rc = ps_check_draws(who, S)) return rc;
    bind_process_device();
    DevBuf<double> dX, dW, dOut;
    if (upload(dX, X, (size_t)C * S) || upload(dW, w, (size_t)4 * S)) return -10;
    BDRT_HIP(dOut.alloc((size_t)C * 4));
    if (const int rc = ps_cjs_device(dX, 0, 1, (size_t)S, dW, 1, 1, S, C, dOut, nullptr)) return rc;
    BDRT_HIP(hipDeviceSynchronize());
    return download(cjs2, dOut.p, (size_t)C * 4);
}

int bdrt_debug_powerscale_weights(const double *L, int G, int S, double alpha_lo, double alpha_hi, double *lw, double *w,
                                  double *pareto_k, int *n_tail)
{
    const char *who = "bdrt_debug_powerscale_weights";
    if (!L || !pareto_k || !n_tail || G < 1) { set_error("%s: bad arguments", who); return -1; }
    if (ps_check_alphas(who, alpha_lo, alpha_hi)) return -1;
    if (const int rc = ps_check_draws(who, S)) return rc;
    bind_process_device();
    const size_t nw = (size_t)G * 4 * S;
    DevBuf<double> dL, dLw, dW, dK;
    DevBuf<int> dNt;
    if (upload(dL, L, (size_t)G * 2 * S)) return -10;
    if (lw) BDRT_HIP(dLw.alloc(nw));
    if (w) BDRT_HIP(dW.alloc(nw));
    BDRT_HIP(dK.alloc((size_t)G * 4));
    BDRT_HIP(dNt.alloc((size_t)G * 4));
    if (const int rc = ps_weights_device(who, dL, G, S, alpha_lo, alpha_hi, dLw, dW, dK, dNt, nullptr)) return rc;
    BDRT_HIP(hipDeviceSynchronize());
    if ((lw && download(lw, dLw.p, nw)) || (w && download(w, dW.p, nw)) || download(pareto_k, dK.p, (size_t)G * 4) ||
        download(n_tail, dNt.p, (size_t)G * 4))
        return -10;
    return 0;
}

}  // extern "C"
