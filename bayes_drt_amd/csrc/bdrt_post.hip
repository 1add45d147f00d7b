// bdrt_post.hip -- posterior post-processing on the device (include/bdrt.h section (4)).
//
// Replaces the numpy reductions the reference applies to the HMC draws right after `sampling`
// (reference bayes_drt/inversion.py): np.percentile(samples, q, axis=0) in coef_percentile (:2560), predict_Z (:2702,
// :2734-2735), predict_Rp (:3068, :3085), predict_sigma (:3096-3113), and the draws-times-basis products in front of
// them (predict_Z: Z_pred_matrix = x_samples A^T + offsets; predict_distribution: F = coef Phi^T).
//
//   project_kernel     Y[rows x M] = X[rows x K] Phi[M x K]^T + bias[M]      one wave per 16x16 tile, v_mfma_f64_16x16x4_f64
//   percentile_kernel  one workgroup per column: the column goes to LDS, bitonic sort, numpy's default ('linear')
//                      percentile rule with numpy's own lerp formula (bit-identical to np.percentile for finite data;
//                      a column with a NaN gives NaN, as numpy does)
//
// The draws never have to leave the GPU: bdrt_sampler_percentiles works on the sampler's device buffer.
#include <cmath>

#include "bdrt_host.h"
#include "bdrt_stats.h"

namespace bdrt {

constexpr int PCT_MAX_ROWS = 16384;   // a column of up to 16384 samples (128 KiB) is sorted in LDS, a longer one in HBM

__global__ __launch_bounds__(64) void project_kernel(const double *__restrict__ X, int rows, int K, long ldx,
                                                     const double *__restrict__ Phi, int M,
                                                     const double *__restrict__ bias, double *__restrict__ Y)
{
    const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
    const int r0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    const int ra = r0 + col, mb = m0 + col;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + kq;
        const double a = (ra < rows && k < K) ? X[(size_t)ra * ldx + k] : 0.0;      // A[i][k] = X[r0 + i][k]
        const double b = (mb < M && k < K) ? Phi[(size_t)mb * K + k] : 0.0;         // B[k][j] = Phi[m0 + j][k]
        acc = mfma_f64(a, b, acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = r0 + kq + 4 * q, m = m0 + col;
        if (r < rows && m < M) Y[(size_t)r * M + m] = acc[q] + (bias ? bias[m] : 0.0);
    }
}

// One workgroup per column.  IN_LDS: the column (padded to n2, a power of two) is sorted in LDS; otherwise (more than
// PCT_MAX_ROWS samples) in the column's slice of the global scratch `work` -- same network, same result.
// expcol[col] != 0: the samples are exp(Y) (constrained scale of a Stan <lower=0> parameter; exp is monotone, so the
// order statistics are those of Y and only the interpolation differs).  mean_out: sample mean of every column.
template <bool IN_LDS>
__global__ __launch_bounds__(512) void percentile_kernel(const double *__restrict__ Y, int rows, long ld_row, long ld_col,
                                                         int ncols, int n2, const double *__restrict__ q, int nq,
                                                         double *__restrict__ out, double *__restrict__ work,
                                                         const unsigned char *__restrict__ expcol,
                                                         double *__restrict__ mean_out)
{
    extern __shared__ __attribute__((aligned(16))) double sh_[];
    const int col = blockIdx.x, tid = threadIdx.x;
    double *red = sh_;                                              // 512 doubles: reduction scratch of the mean
    double *sh = IN_LDS ? sh_ + 512 : work + (size_t)col * n2;
    const bool ex = expcol && expcol[col];
    int flag = 0;
    double part = 0.0;
    for (int i = tid; i < n2; i += 512) {
        double v = INFINITY;
        if (i < rows) {
            v = Y[(size_t)i * ld_row + (size_t)col * ld_col];
            if (ex) v = exp(v);
            part += v;
        }
        if (v != v) { flag = 1; v = INFINITY; }
        sh[i] = v;
    }
    red[tid] = part;
    const int has_nan = __syncthreads_or(flag);
    if (mean_out) {
        for (int w = 256; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) mean_out[col] = has_nan ? NAN : red[0] / (double)rows;
    }
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += 512) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool asc = (i & k) == 0;
                    const double a = sh[i], b = sh[ixj];
                    if ((a > b) == asc) { sh[i] = b; sh[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < nq; t += 512) {
        // q[t] is already q / 100, divided on the host (IEEE division, as numpy's np.true_divide)
        const double r = numpy_quantile([&](int i) -> double { return sh[i]; }, rows, q[t]);
        out[(size_t)t * ncols + col] = has_nan ? NAN : r;
    }
}

static int launch_percentiles(const double *dY, int rows, long ld_row, int ncols, const double *dq, int nq, double *dOut,
                              const unsigned char *dExp, double *dMean, hipStream_t stream)
{
    int n2 = 1;
    while (n2 < rows) n2 <<= 1;
    if (rows <= PCT_MAX_ROWS) {
        const size_t lds = (size_t)(n2 + 512) * sizeof(double);
        static LdsAttrCache attr_cache;
        BDRT_HIP(attr_cache.ensure(lds, [&]() {
            return hipFuncSetAttribute((const void *)percentile_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        }));
        hipLaunchKernelGGL(percentile_kernel<true>, dim3(ncols), dim3(512), lds, stream, dY, rows, ld_row, 1L, ncols, n2, dq, nq,
                           dOut, (double *)nullptr, dExp, dMean);
        BDRT_HIP(hipGetLastError());
        BDRT_HIP(hipStreamSynchronize(stream));
        return 0;
    }
    // long columns (np.percentile has no row limit): sort in a global scratch slice per column
    DevBuf<double> work;
    BDRT_HIP(work.alloc((size_t)ncols * n2));
    hipLaunchKernelGGL(percentile_kernel<false>, dim3(ncols), dim3(512), 512 * sizeof(double), stream, dY, rows, ld_row, 1L, ncols,
                       n2, dq, nq, dOut, (double *)work, dExp, dMean);
    BDRT_HIP(hipGetLastError());
    BDRT_HIP(hipStreamSynchronize(stream));
    return 0;
}

// device core: percentiles of (X Phi^T + bias) or of X itself (Phi == nullptr); all pointers are device pointers
static int percentiles_dev(const double *dX, int rows, int K, long ldx, const double *dPhi, int M, const double *dBias,
                           const double *dq, int nq, double *dOut, const unsigned char *dExp, double *dMean, hipStream_t stream)
{
    if (rows < 1) { set_error("bdrt percentiles: no sample rows"); return -3; }
    if (dPhi) {
        DevBuf<double> dY;
        BDRT_HIP(dY.alloc((size_t)rows * M));
        hipLaunchKernelGGL(project_kernel, dim3((rows + 15) / 16, (M + 15) / 16), dim3(64), 0, stream, dX, rows, K, ldx, dPhi,
                           M, dBias, (double *)dY);
        BDRT_HIP(hipGetLastError());
        return launch_percentiles(dY, rows, (long)M, M, dq, nq, dOut, nullptr, dMean, stream);
    }
    return launch_percentiles(dX, rows, ldx, K, dq, nq, dOut, dExp, dMean, stream);
}

int post_percentiles_device(const double *dX, int rows, int K, long ldx, const double *Phi, int M, const double *bias,
                            const double *q, int nq, double *out, const unsigned char *expcol, double *mean)
{
    const int ncols = Phi ? M : K;
    DevBuf<double> dPhi, dBias, dq, dOut, dMean;
    DevBuf<unsigned char> dExp;
    if (Phi && upload(dPhi, Phi, (size_t)M * K)) return -10;
    if (Phi && bias && upload(dBias, bias, (size_t)M)) return -10;
    std::vector<double> quant(nq);
    for (int t = 0; t < nq; ++t) quant[t] = q[t] / 100.0;           // np.true_divide(q, 100)
    if (upload(dq, quant.data(), (size_t)nq)) return -10;
    BDRT_HIP(dOut.alloc((size_t)nq * ncols));
    if (expcol && !Phi && upload(dExp, expcol, (size_t)K)) return -10;
    if (mean) BDRT_HIP(dMean.alloc((size_t)ncols));
    const int rc = percentiles_dev(dX, rows, K, ldx, dPhi, M, dBias, dq, nq, dOut, dExp, dMean, nullptr);
    if (rc) return rc;
    BDRT_HIP(hipMemcpy(out, dOut, (size_t)nq * ncols * sizeof(double), hipMemcpyDeviceToHost));
    if (mean) BDRT_HIP(hipMemcpy(mean, dMean, (size_t)ncols * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace bdrt

using namespace bdrt;

extern "C" {

int bdrt_percentiles(const double *X, int rows, int K, long ldx, const double *Phi, int M, const double *bias,
                     const double *q, int nq, double *out)
{
    if (!X || rows < 1 || K < 1 || ldx < K || !q || nq < 1 || !out || (Phi && M < 1)) {
        set_error("bdrt_percentiles: bad arguments");
        return -1;
    }
    bind_process_device();
    DevBuf<double> dX;
    if (upload_rows(dX, X, (size_t)rows, ldx, K)) return -10;
    return post_percentiles_device(dX, rows, K, ldx, Phi, M, bias, q, nq, out);
}

int bdrt_summary(const double *X, int rows, int K, long ldx, const unsigned char *is_pos, const double *q, int nq,
                 double *mean, double *pct)
{
    if (!X || rows < 1 || K < 1 || ldx < K || !q || nq < 1 || !pct) { set_error("bdrt_summary: bad arguments"); return -1; }
    bind_process_device();
    DevBuf<double> dX;
    if (upload_rows(dX, X, (size_t)rows, ldx, K)) return -10;
    return post_percentiles_device(dX, rows, K, ldx, nullptr, 0, nullptr, q, nq, pct, is_pos, mean);
}

}  // extern "C"
