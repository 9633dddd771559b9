// The heteroskedastic Normal likelihood with TWO latent GPs per row (likelihoods/multilatent.py HeteroskedasticTFPConditional with
// the Normal conditional): y | f, g ~ N(f, s(g)^2), s = exp or softplus, gfx950.  Contract: include/gpk.h (gpk_hetero_varexp_sum,
// gpk_hetero_predict).  The reference integrates a 20 x 20 Gauss-Hermite grid per row; here the location latent is integrated out in
// closed form, which leaves nothing to integrate under exp and a 20-node rule over the scale latent under softplus (hetero_element.h).
//
// Lanes.  LINK is a template parameter, uniform for the launch.  exp: one lane per row, both latents of the row in that lane's
// registers, the row's two means read as ONE 16-byte load (and its seeds written as 16-byte stores) where the pointers allow it;
// 256 rows per block.  softplus: four adjacent lanes per row, five nodes each, the six running sums met by two xor shuffles; 64
// rows per block; lane k == 0 stores.  At most GPK_REDUCE_MAXPART = 1024 blocks: past 262144 (exp) or 65536 (softplus) rows a
// block walks on with a stride of gridDim.x blocks of rows.  Every trip is taken by all lanes of the block -- a lane without a row
// runs on harmless values and is masked at the stores -- so the shuffles always meet active lanes.
//
// Sum.  One accumulator per lane, block_sum's fixed order, one partial per block in parts[block]; the block that draws the last ticket
// adds the partials in index order (strided over its threads, block_sum again), so the bits do not depend on which block that is.
// The ticket is the word behind the partials, parts[blocks]; a one-thread launch in front of the kernel, in the same call, zeroes it
// (and writes out[0] = 0 for rows = 0).  The only atomic is the integer ticket.
#include "hetero_element.h"

namespace {

struct HeteroArgs {
  LatentMoments m;                         // P = 2, Y one column
  double *rows_out, *dmu_out, *dvar_out;   // [rows], [rows, 2], [rows, 2]; each may be null
  double* parts;                           // [gridDim.x] block sums, then the ticket word
  double* out;
  int vec;                                 // fmean and the [rows, 2] outputs are 16-byte aligned
};

template <int LINK> constexpr int hetero_rows_per_block() { return RB / hetero_lpr<LINK>(); }

__device__ __forceinline__ void store2(double* base, long b, double x0, double x1, int vec) {
  if (!base) return;
  if (vec) *reinterpret_cast<double2*>(base + 2 * b) = make_double2(x0, x1);
  else { base[2 * b] = x0; base[2 * b + 1] = x1; }
}

// the row's operands: means + mean_const, variances knn - s0 + ssq (latent_var), label
__device__ __forceinline__ HeteroRow hetero_load(const LatentMoments& m, long b, int vec) {
  HeteroRow r;
  if (vec) {
    const double2 f = *reinterpret_cast<const double2*>(m.fmean + 2 * b);
    r.m1 = f.x; r.m2 = f.y;
  } else {
    r.m1 = m.fmean[2 * b]; r.m2 = m.fmean[2 * b + 1];
  }
  r.m1 += m.mean_const; r.m2 += m.mean_const;
  r.v1 = latent_var(m, b, 0); r.v2 = latent_var(m, b, 1);
  r.y = m.Y[b * m.ldy];
  return r;
}

__global__ void hetero_reset_kernel(double* parts, int nb, double* out) {
  if (parts) *reinterpret_cast<unsigned int*>(parts + nb) = 0u;
  if (nb == 0) out[0] = 0.0;
}

template <int LINK>
__global__ __launch_bounds__(RB) void hetero_varexp_kernel(HeteroArgs a) {
  constexpr int LPR = hetero_lpr<LINK>(), RPB = hetero_rows_per_block<LINK>();
  __shared__ double sh[4];
  __shared__ int s_last;
  const LatentMoments& m = a.m;
  const int k = threadIdx.x % LPR, jr = threadIdx.x / LPR;
  double acc = 0.0;
  for (long b0 = (long)blockIdx.x * RPB; b0 < m.rows; b0 += (long)gridDim.x * RPB) {   // (uniform over the block)
    const long b = b0 + jr;
    const bool act = b < m.rows;
    HeteroRow r{0.0, 0.0, 1.0, 0.0, 1.0};
    if (act) r = hetero_load(m, b, a.vec);
    double ve, dm1, dv1, dm2, dv2;
    hetero_varexp_element<LINK>(r, k, ve, dm1, dv1, dm2, dv2);
    if (act && k == 0) {
      store2(m.fvar_out, b, r.v1, r.v2, a.vec);
      store2(a.dmu_out, b, dm1, dm2, a.vec);
      store2(a.dvar_out, b, dv1, dv2, a.vec);
      if (a.rows_out) a.rows_out[b] = ve;
      acc += ve;
    }
  }
  const double r0 = block_sum(acc, sh);
  if (threadIdx.x == 0) {
    a.parts[blockIdx.x] = r0;
    __threadfence();   // the partial is visible device-wide before the ticket is
    s_last = atomicAdd(reinterpret_cast<unsigned int*>(a.parts + gridDim.x), 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();     // every other block's partial was released before its ticket
  double v = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += RB) v += __hip_atomic_load(a.parts + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double t = block_sum(v, sh);
  if (threadIdx.x == 0) a.out[0] = t;
}

struct HeteroPredictArgs {
  const double *fmean, *fvar, *Y;   // [rows, 2], [rows, 2] contiguous; Y [rows, 1] with row stride ldy, or null
  long ldy; int rows;
  double *mean_out, *var_out, *ld_out;   // [rows] each; each may be null
  int vec;
};

template <int LINK, bool LD>
__global__ __launch_bounds__(RB) void hetero_predict_kernel(HeteroPredictArgs a) {
  constexpr int LPR = hetero_lpr<LINK>(), RPB = hetero_rows_per_block<LINK>();
  const int k = threadIdx.x % LPR, jr = threadIdx.x / LPR;
  for (long b0 = (long)blockIdx.x * RPB; b0 < a.rows; b0 += (long)gridDim.x * RPB) {
    const long b = b0 + jr;
    const bool act = b < a.rows;
    HeteroRow r{0.0, 0.0, 1.0, 0.0, 1.0};
    if (act) {
      if (a.vec) {
        const double2 f = *reinterpret_cast<const double2*>(a.fmean + 2 * b), v = *reinterpret_cast<const double2*>(a.fvar + 2 * b);
        r.m1 = f.x; r.m2 = f.y; r.v1 = v.x; r.v2 = v.y;
      } else {
        r.m1 = a.fmean[2 * b]; r.m2 = a.fmean[2 * b + 1]; r.v1 = a.fvar[2 * b]; r.v2 = a.fvar[2 * b + 1];
      }
      if constexpr (LD) r.y = a.Y[b * a.ldy];
    }
    double var, ld;
    hetero_predict_element<LINK, LD>(r, k, var, ld);
    if (act && k == 0) {
      if (a.mean_out) a.mean_out[b] = r.m1;
      if (a.var_out) a.var_out[b] = var;
      if constexpr (LD) a.ld_out[b] = ld;
    }
  }
}

int hetero_blocks(int rows, int link) {
  const int rpb = link == GPK_HETERO_LINK_EXP ? hetero_rows_per_block<GPK_HETERO_LINK_EXP>()
                                              : hetero_rows_per_block<GPK_HETERO_LINK_SOFTPLUS>();
  long nb = ((long)rows + rpb - 1) / rpb;
  nb = nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb;
  return (int)nb;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }   // (null counts as aligned)
bool known_link(int link) { return link == GPK_HETERO_LINK_EXP || link == GPK_HETERO_LINK_SOFTPLUS; }

}  // namespace

extern "C" int gpk_hetero_varexp_blocks(int rows, int link) {
  if (rows < 0 || !known_link(link)) return 0;
  return hetero_blocks(rows, link);
}

extern "C" int gpk_hetero_varexp_sum(void* stream, int link, const double* Y, long ldy, const double* fmean, int rows,
                                     const double* s0, int s0_per_latent, const double* ssq, const double* knn_host,
                                     int knn_per_latent, double mean_const, double* fvar_out, double* rows_out, double* dmu_out,
                                     double* dvar_out, double* out, double* parts) {
  if (!known_link(link) || rows < 0 || !knn_host || !out) return GPK_E_ARG;
  if (rows > 0 && (!Y || !fmean || !parts || ldy < 1)) return GPK_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int nb = hetero_blocks(rows, link);
  hipLaunchKernelGGL(hetero_reset_kernel, dim3(1), dim3(1), 0, s, rows > 0 ? parts : nullptr, nb, out);
  GPK_LAUNCH_CHECK();
  if (rows == 0) return 0;
  HeteroArgs a{};
  a.m = gpk_latent_moments(Y, ldy, fmean, rows, 2, s0, s0_per_latent, ssq, knn_host, knn_per_latent, mean_const, fvar_out);
  a.rows_out = rows_out; a.dmu_out = dmu_out; a.dvar_out = dvar_out; a.parts = parts; a.out = out;
  a.vec = aligned16(fmean) && aligned16(fvar_out) && aligned16(dmu_out) && aligned16(dvar_out);
  if (link == GPK_HETERO_LINK_EXP)
    hipLaunchKernelGGL(hetero_varexp_kernel<GPK_HETERO_LINK_EXP>, dim3((unsigned)nb), dim3(RB), 0, s, a);
  else
    hipLaunchKernelGGL(hetero_varexp_kernel<GPK_HETERO_LINK_SOFTPLUS>, dim3((unsigned)nb), dim3(RB), 0, s, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_hetero_predict(void* stream, int link, const double* fmean, const double* fvar, const double* Y, long ldy,
                                  int rows, double* mean_out, double* var_out, double* logdens_out) {
  if (!known_link(link) || rows < 0) return GPK_E_ARG;
  if (rows > 0 && (!fmean || !fvar)) return GPK_E_ARG;
  if (Y && (!logdens_out || ldy < 1)) return GPK_E_ARG;
  if (rows == 0) return 0;
  HeteroPredictArgs a{fmean, fvar, Y, ldy, rows, mean_out, var_out, Y ? logdens_out : nullptr, aligned16(fmean) && aligned16(fvar)};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)hetero_blocks(rows, link)), block(RB);
  if (link == GPK_HETERO_LINK_EXP) {
    if (Y) hipLaunchKernelGGL((hetero_predict_kernel<GPK_HETERO_LINK_EXP, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((hetero_predict_kernel<GPK_HETERO_LINK_EXP, false>), grid, block, 0, s, a);
  } else {
    if (Y) hipLaunchKernelGGL((hetero_predict_kernel<GPK_HETERO_LINK_SOFTPLUS, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((hetero_predict_kernel<GPK_HETERO_LINK_SOFTPLUS, false>), grid, block, 0, s, a);
  }
  GPK_LAUNCH_CHECK();
  return 0;
}
