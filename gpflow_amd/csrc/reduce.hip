// The deterministic two-stage scalar reductions (KL, log-dets, sums of squares, LML tail; the ELBO data term's stage 1 is varexp.hip)
// and the fixed-order sums of split-K partials.  All reductions are order-deterministic: stage 1 writes one partial per block,
// stage 2 (one block) sums them in a fixed order -- no floating-point atomics anywhere on this path.
#include "reduce_device.h"

namespace {

// ---- stage 2: out = sum_t scale[t] * sum(part[t][0..count[t])) + add ------------------------------
struct FinalArgs {
  const double* part[4]; int count[4]; double scale[4]; int nterms; double add; double* out;
};
__global__ __launch_bounds__(RB) void final_sum_kernel(FinalArgs a) {
  __shared__ double sh[4];
  double total = a.add;
  for (int t = 0; t < a.nterms; ++t) {
    double v = 0.0;
    for (int i = threadIdx.x; i < a.count[t]; i += RB) v += a.part[t][i];
    const double r = block_sum(v, sh);
    total += a.scale[t] * r;
  }
  if (threadIdx.x == 0) *a.out = total;
}

// ---- ssq[p,b] = sum_t part[p][t][b] -------------------------------------------------------------------
__global__ void sum_parts_kernel(const double* part, int nt, int rows, long stridePart, double* ssq) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
  if (b >= rows) return;
  const double* q = part + (long)p * stridePart;
  double s = 0.0;
  for (int t = 0; t < nt; ++t) s += q[(long)t * rows + b];
  ssq[(long)p * rows + b] = s;
}

// ---- out = alpha * sum_p part[p]  (optionally lower-triangular: zeros above the diagonal, diagonal scaled) --------
// The partial products of a split-K GEMM summed in a fixed order (p = 0, 1, ...): deterministic, one pass, 16-byte
// accesses; with lower != 0 entries above the diagonal are never read (a lower-only GEMM does not write those tiles).
// NP > 0: the number of parts is a compile-time constant and all NP loads of a thread are issued before the first add
// (with a run-time loop every add waited for its own load: 330 us for 8 parts of 2048^2, 0.4 TB/s); NP = 0: any count.
template <int NP>
__global__ __launch_bounds__(256) void combine_parts_kernel(const double* __restrict__ part, int np, long stridePart, int m,
                                                           int n, long ldp, double alpha, int lower, double diag_scale,
                                                           double* __restrict__ out, long ldo) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * 2;
  if (c >= n) return;
  const bool two = c + 1 < n;
  const bool vec_ok = two && ((ldp & 1) == 0) && ((stridePart & 1) == 0) && ((reinterpret_cast<uintptr_t>(part) & 15) == 0);
  for (int r = blockIdx.y; r < m; r += gridDim.y) {
    const bool k0 = !lower || c <= r, k1 = two && (!lower || c + 1 <= r);
    double s0 = 0.0, s1 = 0.0;
    if (k0 || k1) {
      const double* q = part + (long)r * ldp + c;
      if (vec_ok && k0 && k1) {
        if (NP > 0) {
          d2 v[NP > 0 ? NP : 1];
#pragma unroll
          for (int p = 0; p < NP; ++p) v[p] = *reinterpret_cast<const d2*>(q + (long)p * stridePart);
#pragma unroll
          for (int p = 0; p < NP; ++p) { s0 += v[p].x; s1 += v[p].y; }
        } else {
          for (int p = 0; p < np; ++p, q += stridePart) {
            const d2 v = *reinterpret_cast<const d2*>(q);
            s0 += v.x; s1 += v.y;
          }
        }
      } else {
        for (int p = 0; p < np; ++p, q += stridePart) {
          if (k0) s0 += q[0];
          if (k1) s1 += q[1];
        }
      }
      s0 *= alpha; s1 *= alpha;
      if (lower) {
        if (c == r) s0 *= diag_scale;
        if (c + 1 == r) s1 *= diag_scale;
      }
    }
    double* o = out + (long)r * ldo + c;
    if (two && ((ldo & 1) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0)) {
      *reinterpret_cast<d2*>(o) = (d2){k0 ? s0 : 0.0, k1 ? s1 : 0.0};
    } else {
      o[0] = k0 ? s0 : 0.0;
      if (two) o[1] = k1 ? s1 : 0.0;
    }
  }
}

// ---- whitened KL, stage 1: sum q_mu^2 - sum log diag^2 + sum tril^2 -----------------------------------
__global__ __launch_bounds__(RB) void kl_white_kernel(const double* q_mu, const double* q_sqrt, int m,
                                                      int P, int q_diag, double* part, int* zero_word) {
  __shared__ double sh[4];
  // (the ticket of the shard's varexp_kernel<true>, stream-ordered behind this kernel)
  if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;
  double acc = 0.0;
  const long nmu = (long)m * P;
  const long stride = (long)gridDim.x * RB, start = (long)blockIdx.x * RB + threadIdx.x;
  for (long e = start; e < nmu; e += stride) { const double v = q_mu[e]; acc += v * v; }
  if (q_diag) {
    for (long e = start; e < nmu; e += stride) {
      const double v = q_sqrt[e];
      acc += v * v - log(v * v);
    }
  } else {
    const long tot = (long)P * m * m;
    for (long e = start; e < tot; e += stride) {
      const long w = e % ((long)m * m);
      const int r = (int)(w / m), c = (int)(w - (long)r * m);
      if (c <= r) {
        const double v = q_sqrt[e];
        acc += v * v;
        if (c == r) acc -= log(v * v);
      }
    }
  }
  const double r = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// ---- sum log diag(L) per batch (one block per batch) ---------------------------------------------------
__global__ __launch_bounds__(RB) void sum_log_diag_kernel(const double* L, int n, long ldl,
                                                          long strideL, double* out) {
  __shared__ double sh[4];
  const double* M = L + (long)blockIdx.x * strideL;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += RB) acc += log(M[(long)i * ldl + i]);
  const double r = block_sum(acc, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// out[b] = sum_i log(M_b[i,i]^2): the log-determinant of a covariance from a square root whose diagonal may carry either sign
// (kullback_leiblers.py:124: tf.math.log(tf.square(Lq_diag)))
__global__ __launch_bounds__(RB) void sum_log_diag_sq_kernel(const double* L, int n, long ldl, long strideL, double* out) {
  __shared__ double sh[4];
  const double* M = L + (long)blockIdx.x * strideL;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += RB) { const double v = M[(long)i * ldl + i]; acc += log(v * v); }
  const double r = block_sum(acc, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// ---- sum of squares of a matrix, stage 1 -----------------------------------------------------------------
__global__ __launch_bounds__(RB) void sumsq_kernel(const double* A, int rows, int cols, long lda,
                                                   int upper_only, double* part) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const double* a = A + (long)r * lda;
    for (int c = (upper_only ? r : 0) + threadIdx.x; c < cols; c += RB) acc = fma(a[c], a[c], acc);
  }
  const double r = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

}  // namespace

extern "C" size_t gpk_reduce_workspace_bytes(int n) {
  (void)n;
  return (size_t)4 * GPK_REDUCE_MAXPART * sizeof(double);
}

int gpk_launch_sum_parts(hipStream_t s, const double* part, int nt, int rows, long stridePart, int P,
                         double* ssq) {
  if (rows == 0 || P == 0) return 0;
  dim3 grid((unsigned)gpk_cdiv(rows, 256), (unsigned)P);
  hipLaunchKernelGGL(sum_parts_kernel, grid, dim3(256), 0, s, part, nt, rows, stridePart, ssq);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_combine_parts(void* stream, const double* parts, int nparts, long stride_part, int m, int n, long ldp,
                                 double alpha, int lower, double diag_scale, double* out, long ldo) {
  if (nparts <= 0 || m < 0 || n < 0 || ldp < n || ldo < n) return GPK_E_ARG;
  if (m == 0 || n == 0) return 0;
  if (!parts || !out) return GPK_E_ARG;
  dim3 grid((unsigned)gpk_cdiv(gpk_cdiv(n, 2), 256), (unsigned)(m < 65535 ? m : 65535));
#define GPK_COMBINE(NP)                                                                                               \
  hipLaunchKernelGGL((combine_parts_kernel<NP>), grid, dim3(256), 0, (hipStream_t)stream, parts, nparts, stride_part, m, n, \
                     ldp, alpha, lower, diag_scale, out, ldo)
  switch (nparts) {
    case 1: GPK_COMBINE(1); break;
    case 2: GPK_COMBINE(2); break;
    case 4: GPK_COMBINE(4); break;
    case 8: GPK_COMBINE(8); break;
    case 16: GPK_COMBINE(16); break;
    case 32: GPK_COMBINE(32); break;
    default: GPK_COMBINE(0); break;
  }
#undef GPK_COMBINE
  GPK_LAUNCH_CHECK();
  return 0;
}

// out = sum_t scale[t]*sum(part[t][0..count[t])) + add   (used by the fused drivers)
int gpk_launch_final(hipStream_t s, int nterms, const double* const* part, const int* count,
                     const double* scale, double add, double* out) {
  FinalArgs f{};
  f.nterms = nterms;
  for (int t = 0; t < nterms; ++t) { f.part[t] = part[t]; f.count[t] = count[t]; f.scale[t] = scale[t]; }
  f.add = add; f.out = out;
  hipLaunchKernelGGL(final_sum_kernel, dim3(1), dim3(RB), 0, s, f);
  GPK_LAUNCH_CHECK();
  return 0;
}
// the one-term form:  *out = scale * sum(part[0:count]) + add
int gpk_launch_final_one(hipStream_t s, const double* part, int count, double scale, double add, double* out) {
  return gpk_launch_final(s, 1, &part, &count, &scale, add, out);
}

// stage-1 launchers reused by the fused drivers (partials land in `part`, count returned)
int gpk_launch_sumsq_stage1(hipStream_t s, const double* A, int rows, int cols, long lda,
                            int upper_only, double* part, int* count) {
  int nb = rows < GPK_REDUCE_MAXPART ? rows : GPK_REDUCE_MAXPART;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(RB), 0, s, A, rows, cols, lda, upper_only, part);
  GPK_LAUNCH_CHECK();
  *count = nb;
  return 0;
}
int gpk_launch_kl_white_stage1(hipStream_t s, const double* q_mu, const double* q_sqrt, int m, int P,
                               int q_diag, double* part, int* count, int* zero_word) {
  const long elems = q_diag ? (long)m * P : (long)P * m * m;
  const int nb = nblocks_for(elems);
  hipLaunchKernelGGL(kl_white_kernel, dim3(nb), dim3(RB), 0, s, q_mu, q_sqrt, m, P, q_diag, part, zero_word);
  GPK_LAUNCH_CHECK();
  *count = nb;
  return 0;
}

extern "C" int gpk_gauss_kl_white(void* stream, const double* q_mu, const double* q_sqrt, int m,
                                  int P, int q_diag, double* out, void* ws, size_t ws_bytes) {
  if (!q_mu || !q_sqrt || !out || m <= 0 || P <= 0) return GPK_E_ARG;
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, gpk_reduce_workspace_bytes(m)));
  int nb = 0;
  GPK_TRY(gpk_launch_kl_white_stage1((hipStream_t)stream, q_mu, q_sqrt, m, P, q_diag, (double*)ws, &nb, nullptr));
  return gpk_launch_final_one((hipStream_t)stream, (double*)ws, nb, 0.5, -0.5 * (double)m * (double)P, out);
}

extern "C" int gpk_sumsq(void* stream, const double* A, int rows, int cols, long lda, int upper_only,
                         double* out, void* ws, size_t ws_bytes) {
  if ((!A && rows > 0 && cols > 0) || !out || rows < 0 || cols < 0) return GPK_E_ARG;
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, gpk_reduce_workspace_bytes(rows)));
  int nb = 0;
  GPK_TRY(gpk_launch_sumsq_stage1((hipStream_t)stream, A, rows, cols, lda, upper_only, (double*)ws, &nb));
  return gpk_launch_final_one((hipStream_t)stream, (double*)ws, nb, 1.0, 0.0, out);
}

extern "C" int gpk_sum_log_diag(void* stream, const double* L, int n, long ldl, int batch,
                                long strideL, double* out) {
  if (!L || !out || n <= 0) return GPK_E_ARG;
  hipLaunchKernelGGL(sum_log_diag_kernel, dim3((unsigned)(batch > 0 ? batch : 1)), dim3(RB), 0,
                     (hipStream_t)stream, L, n, ldl, strideL, out);
  GPK_LAUNCH_CHECK();
  return 0;
}

// Un-whitened KL with a diagonal q_sqrt (kullback_leiblers.py:128-165, q_diag and K given): per inducing point i
//   part += (K^-1)_ii * sum_p w_ip^2 - sum_p log(w_ip^2),   (K^-1)_ii = |row i of L^-T|^2  (rows of LinvT, upper triangular)
__global__ __launch_bounds__(RB) void kl_unwhite_diag_kernel(const double* __restrict__ LinvT, long ldl, int m,
                                                            const double* __restrict__ W, int P, double* __restrict__ part) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int i = blockIdx.x; i < m; i += gridDim.x) {
    double ss = 0.0;
    for (int k = i + threadIdx.x; k < m; k += RB) {
      const double v = LinvT[(long)i * ldl + k];
      ss += v * v;
    }
    const double kinv = block_sum(ss, sh);
    __syncthreads();
    if (threadIdx.x == 0) {
      double w2 = 0.0, lg = 0.0;
      for (int p = 0; p < P; ++p) {
        const double w = W[(long)i * P + p];
        w2 += w * w;
        lg += log(w * w);
      }
      acc += kinv * w2 - lg;
    }
  }
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
int gpk_launch_kl_unwhite_diag_stage1(hipStream_t s, const double* LinvT, long ldl, int m, const double* W, int P, double* part,
                                      int* count) {
  const int nb = m < GPK_REDUCE_MAXPART ? m : GPK_REDUCE_MAXPART;
  hipLaunchKernelGGL(kl_unwhite_diag_kernel, dim3(nb), dim3(RB), 0, s, LinvT, ldl, m, W, P, part);
  GPK_LAUNCH_CHECK();
  *count = nb;
  return 0;
}

int gpk_launch_sum_log_diag_sq(hipStream_t s, const double* L, int n, long ldl, int batch, long strideL, double* out) {
  if (!L || !out || n <= 0) return GPK_E_ARG;
  hipLaunchKernelGGL(sum_log_diag_sq_kernel, dim3((unsigned)(batch > 0 ? batch : 1)), dim3(RB), 0, s, L, n, ldl, strideL, out);
  GPK_LAUNCH_CHECK();
  return 0;
}
