// Layout and row passes around the factorisation: transposes, triangle / identity / diagonal fills, row statistics of A^T, row dots.
#include "reduce_device.h"

namespace {

// ---- zero the strict upper triangle -----------------------------------------------------------------
__global__ void zero_upper_kernel(double* A, int n, long lda, long strideA) {
  double* M = A + (long)blockIdx.z * strideA;
  const int r = blockIdx.y;
  for (int c = r + 1 + blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x)
    M[(long)r * lda + c] = 0.0;
}

// ---- transpose with optional triangular mask -------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_kernel(const double* in, int rows, int cols,
                                                        long ldin, double* out, long ldout,
                                                        int mode, long stride_in, long stride_out) {
  __shared__ double tile[32][33];
  const double* I = in + (long)blockIdx.z * stride_in;
  double* O = out + (long)blockIdx.z * stride_out;
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int k = ty; k < 32; k += 8) {
    const int r = by + k, c = bx + tx;
    double v = 0.0;
    if (r < rows && c < cols) {
      const bool keep = (mode == 0) || (mode == 1 && c <= r) || (mode == 2 && c >= r);
      if (keep) v = I[(long)r * ldin + c];
    }
    tile[k][tx] = v;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int r = bx + k, c = by + tx;  // out[r][c] = in[c][r]
    if (r < cols && c < rows) O[(long)r * ldout + c] = tile[tx][k];
  }
}

// out[c][r] = in[r][c] + shift  (used to lay (Y - mean)^T under the covariance matrix)
__global__ __launch_bounds__(256) void transpose_shift_kernel(const double* in, int rows, int cols,
                                                              long ldin, double* out, long ldout,
                                                              double shift) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int r = by + k, c = bx + tx;
    tile[k][tx] = (r < rows && c < cols) ? in[(long)r * ldin + c] + shift : 0.0;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int r = bx + k, c = by + tx;
    if (r < cols && c < rows) out[(long)r * ldout + c] = tile[tx][k];
  }
}

// ---- row statistics of At [rows, m]:  sumsq[b], mv[b,p] = sum_k At[b,k] V[k,p],
//      wsq[p,b] = sum_k (At[b,k] W[k,p])^2.   One wave per row, 4 rows per block. --------------------
template <int PC>
__global__ __launch_bounds__(256) void row_stats_kernel(const double* __restrict__ At, int rows,
                                                        int m, long ldat,
                                                        const double* __restrict__ V,
                                                        const double* __restrict__ W, int P, int p0,
                                                        double alpha, double beta,
                                                        double* __restrict__ sumsq,
                                                        double* __restrict__ mv,
                                                        double* __restrict__ wsq) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  if (row >= rows) return;
  const double* a = At + (long)row * ldat;
  double s = 0.0, dv[PC], dw[PC];
#pragma unroll
  for (int q = 0; q < PC; ++q) { dv[q] = 0.0; dw[q] = 0.0; }
  for (int k = lane; k < m; k += 64) {
    const double x = a[k];
    s = fma(x, x, s);
#pragma unroll
    for (int q = 0; q < PC; ++q) {
      if (p0 + q < P) {
        if (V) dv[q] = fma(x, V[(long)k * P + p0 + q], dv[q]);
        if (W) { const double t = x * W[(long)k * P + p0 + q]; dw[q] = fma(t, t, dw[q]); }
      }
    }
  }
  s = wave_sum(s);
#pragma unroll
  for (int q = 0; q < PC; ++q) { dv[q] = wave_sum(dv[q]); dw[q] = wave_sum(dw[q]); }
  if (lane == 0) {
    if (sumsq && p0 == 0) sumsq[row] = (beta != 0.0 ? beta * sumsq[row] : 0.0) + alpha * s;
#pragma unroll
    for (int q = 0; q < PC; ++q)
      if (p0 + q < P) {
        if (V && mv) mv[(long)row * P + p0 + q] = dv[q];
        if (W && wsq) wsq[(long)(p0 + q) * rows + row] = dw[q];
      }
  }
}

// ---- the same for P separate At_p (SeparateIndependent latents): sumsq[p, b] = sum_k At_p[b,k]^2, mv[b, p] = sum_k At_p[b,k] V[k,p];
// one wave per (row, latent), blockIdx.y = p: ONE launch instead of P (plus P strided-column copies of V on the host side)
__global__ __launch_bounds__(256) void row_stats_sep_kernel(const double* __restrict__ At, long strideAt, int rows, int m, long ldat,
                                                            const double* __restrict__ V, int P, double* __restrict__ sumsq,
                                                            double* __restrict__ mv) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w, p = blockIdx.y;
  if (row >= rows) return;
  const double* a = At + (long)p * strideAt + (long)row * ldat;
  double s = 0.0, dv = 0.0;
  for (int k = lane; k < m; k += 64) {
    const double x = a[k];
    s = fma(x, x, s);
    dv = fma(x, V[(long)k * P + p], dv);
  }
  s = wave_sum(s);
  dv = wave_sum(dv);
  if (lane == 0) {
    sumsq[(long)p * rows + row] = s;
    mv[(long)row * P + p] = dv;
  }
}

// ---- out[i] = beta*out[i] + alpha * sum_j A[i,j] B[i,j]  (one wave per row) --------------------------
__global__ __launch_bounds__(256) void row_dot_kernel(const double* __restrict__ A, long lda,
                                                      const double* __restrict__ B, long ldb, int rows,
                                                      int cols, double alpha, double beta,
                                                      double* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  if (row >= rows) return;
  const double* a = A + (long)row * lda;
  const double* b = B + (long)row * ldb;
  double s = 0.0;
  for (int k = lane; k < cols; k += 64) s = fma(a[k], b[k], s);
  s = wave_sum(s);
  if (lane == 0) out[row] = (beta != 0.0 ? beta * out[row] : 0.0) + alpha * s;
}

__global__ __launch_bounds__(256) void set_identity_kernel(double* __restrict__ A, int n, long lda, long strideA) {
  const int row = blockIdx.y;
  double* a = A + (long)blockIdx.z * strideA;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) a[(long)row * lda + c] = (c == row) ? 1.0 : 0.0;
}

}  // namespace

// A[i,i] += v[i]:  add_noise_cov with a per-row likelihood variance (utilities/model_utils.py:33-38, 46-50)
__global__ __launch_bounds__(256) void diag_add_kernel(double* __restrict__ A, int n, long lda, const double* __restrict__ v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) A[(long)i * lda + i] += v[i];
}
extern "C" int gpk_diag_add(void* stream, double* A, int n, long lda, const double* v) {
  if (!A || !v || n < 0 || lda < n) return GPK_E_ARG;
  if (n == 0) return 0;
  hipLaunchKernelGGL(diag_add_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, A, n, lda, v);
  GPK_LAUNCH_CHECK();
  return 0;
}
int gpk_launch_set_identity(hipStream_t s, double* A, int n, long lda, int batch, long strideA) {
  if (n <= 0) return 0;
  dim3 grid((unsigned)gpk_cdiv(n, 256), (unsigned)n, (unsigned)(batch > 0 ? batch : 1));
  hipLaunchKernelGGL(set_identity_kernel, grid, dim3(256), 0, s, A, n, lda, strideA);
  GPK_LAUNCH_CHECK();
  return 0;
}

int gpk_launch_zero_upper(hipStream_t s, double* A, int n, long lda, int batch, long strideA) {
  if (n <= 1) return 0;
  int gx = gpk_cdiv(n, 256);
  if (gx > 16) gx = 16;
  dim3 grid((unsigned)gx, (unsigned)n, (unsigned)(batch > 0 ? batch : 1));
  hipLaunchKernelGGL(zero_upper_kernel, grid, dim3(256), 0, s, A, n, lda, strideA);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_transpose(void* stream, const double* in, int rows, int cols, long ldin,
                             double* out, long ldout, int mode, int batch, long stride_in,
                             long stride_out) {
  if (rows < 0 || cols < 0) return GPK_E_ARG;
  if (rows == 0 || cols == 0) return 0;
  if (!in || !out) return GPK_E_ARG;
  dim3 grid((unsigned)gpk_cdiv(cols, 32), (unsigned)gpk_cdiv(rows, 32),
            (unsigned)(batch > 0 ? batch : 1));
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, rows, cols, ldin,
                     out, ldout, mode, stride_in, stride_out);
  GPK_LAUNCH_CHECK();
  return 0;
}

// sumsq[b] = beta*sumsq[b] + alpha*sum_k At^2 ; mv = At V ; wsq[p,b] = sum_k (At W[:,p])^2
extern "C" int gpk_row_stats(void* stream, const double* At, int rows, int m, long ldat,
                             const double* V, const double* W, int P, double alpha, double beta,
                             double* sumsq, double* mv, double* wsq) {
  if (rows < 0 || m < 0) return GPK_E_ARG;
  if (rows == 0) return 0;
  if (!At) return GPK_E_ARG;
  const int np = (V || W) ? P : 0;
  const dim3 grid((unsigned)gpk_cdiv(rows, 4));
  int p0 = 0;
  do {
    hipLaunchKernelGGL((row_stats_kernel<4>), grid, dim3(256), 0, (hipStream_t)stream, At, rows, m,
                       ldat, V, W, np, p0, alpha, beta, sumsq, mv, wsq);
    GPK_LAUNCH_CHECK();
    p0 += 4;
  } while (p0 < np);
  return 0;
}

int gpk_launch_row_stats_sep(hipStream_t s, const double* At, long strideAt, int rows, int m, long ldat, const double* V, int P,
                             double* sumsq, double* mv) {
  if (!At || !V || !sumsq || !mv || rows < 0 || m < 0 || P <= 0) return GPK_E_ARG;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(row_stats_sep_kernel, dim3((unsigned)gpk_cdiv(rows, 4), (unsigned)P), dim3(256), 0, s, At, strideAt, rows, m,
                     ldat, V, P, sumsq, mv);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_row_dot(void* stream, const double* A, long lda, const double* B, long ldb,
                           int rows, int cols, double alpha, double beta, double* out) {
  if (rows < 0 || cols < 0) return GPK_E_ARG;
  if (rows == 0) return 0;
  if (!A || !B || !out) return GPK_E_ARG;
  hipLaunchKernelGGL(row_dot_kernel, dim3((unsigned)gpk_cdiv(rows, 4)), dim3(256), 0,
                     (hipStream_t)stream, A, lda, B, ldb, rows, cols, alpha, beta, out);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_row_sumsq(void* stream, const double* A, int rows, int cols, long lda,
                             double alpha, double beta, double* out) {
  return gpk_row_stats(stream, A, rows, cols, lda, nullptr, nullptr, 0, alpha, beta, out, nullptr,
                       nullptr);
}

int gpk_launch_transpose_shift(hipStream_t s, const double* in, int rows, int cols, long ldin,
                               double* out, long ldout, double shift) {
  if (rows == 0 || cols == 0) return 0;
  dim3 grid((unsigned)gpk_cdiv(cols, 32), (unsigned)gpk_cdiv(rows, 32), 1);
  hipLaunchKernelGGL(transpose_shift_kernel, grid, dim3(256), 0, s, in, rows, cols, ldin, out, ldout,
                     shift);
  GPK_LAUNCH_CHECK();
  return 0;
}
