// The variational-expectation stage of an ELBO shard: Gaussian in closed form (varexp_kernel), scalar likelihoods by Gauss-Hermite
// quadrature (lik_varexp_kernel), MultiClass / RobustMax (lik_multiclass_kernel), Gaussian on linearly mixed latents
// (mixed_varexp_kernel: LinearCoregionalization).  Stage 1 of the two-stage reductions of reduce.hip.
#include "lik_element.h"   // latent_var, the quadrature table, QuadLanes, lik_element<LIK>

namespace {

// ---- Gaussian variational expectations, stage 1 -----------------------------------------------------
struct VarexpArgs {
  LatentMoments m;
  double noise; double* part;
  const double* noise_rows;   // per-row noise variances [rows] (heteroskedastic Gaussian, scalar_continuous.py:92-111) or nullptr
  // TAIL only: ssq arrives as nt slot partials [P][nt][rows] (strideSlot between latents); ticket / out: see varexp_kernel
  const double* slot; int nt; long strideSlot; int* ticket; double* out;
};
// TAIL = false: stage 1 of the two-stage reduction (one partial per block).
// TAIL = true: the whole tail of a shard behind the projection GEMM in one launch -- what sum_parts_kernel, this kernel and
// final_sum_kernel did as three dependent launches of 5 - 10 us each.  The slot partials of an element are summed in slot order
// (sum_parts_kernel's bits), their loads issued sixteen at a time: one element per thread with a load per add was 38 us for
// 8192 x 32 partials on eight blocks.  So the grid is one element per thread here (gpk_launch_varexp_tail), not four.  The block
// that draws the last ticket sums the block partials in index order, as final_sum_kernel does.  The ticket word must be 0 at entry: no memset packet, and not a
// reset by the last block either (the first call on a fresh workspace has to be right) -- kl_white_kernel, which every whitened
// shard runs earlier in the same step on a stream that is joined before this launch, zeroes it (drivers.hip: kl_white_to_out).
template <bool TAIL>
__global__ __launch_bounds__(RB) void varexp_kernel(VarexpArgs a) {
  __shared__ double sh[4];
  __shared__ int s_last;
  const double log2pi = 1.8378770664093453;
  const double c0 = -0.5 * log2pi - 0.5 * log(a.noise);
  double acc = 0.0;
  const LatentMoments& m = a.m;
  const long total = (long)m.rows * m.P;
  for (long e = (long)blockIdx.x * RB + threadIdx.x; e < total; e += (long)gridDim.x * RB) {
    const int b = (int)(e / m.P), p = (int)(e - (long)b * m.P);
    double fv;
    if constexpr (TAIL) {
      const double* q = a.slot + (long)p * a.strideSlot + b;
      double s = 0.0;
      int t = 0;
      for (; t + 16 <= a.nt; t += 16) {
        double v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = q[(long)(t + i) * m.rows];
#pragma unroll
        for (int i = 0; i < 16; ++i) s += v[i];
      }
      for (; t < a.nt; ++t) s += q[(long)t * m.rows];
      fv = latent_var(m, b, p, &s);
    } else fv = latent_var(m, b, p);
    const double mu = m.fmean[e] + m.mean_const;
    const double dy = m.Y[(long)b * m.ldy + p] - mu;
    if (m.fvar_out) m.fvar_out[e] = fv;
    if (a.noise_rows) {   // (workgroup-uniform branch)
      const double nv = a.noise_rows[b];
      acc += (-0.5 * log2pi - 0.5 * log(nv)) - 0.5 * (dy * dy + fv) / nv;
    } else {
      acc += c0 - 0.5 * (dy * dy + fv) / a.noise;
    }
  }
  const double r = block_sum(acc, sh);
  if (threadIdx.x == 0) a.part[blockIdx.x] = r;
  if constexpr (TAIL) {
    if (threadIdx.x == 0) {
      __threadfence();   // the partial is visible device-wide before the ticket is
      s_last = atomicAdd(a.ticket, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();     // every other block's partial was released before its ticket
    double v = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += RB) v += __hip_atomic_load(a.part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double t = block_sum(v, sh);
    if (threadIdx.x == 0) *a.out = 0.0 + 1.0 * t;   // (final_sum_kernel's add + scale * sum)
  }
}

// ---- non-Gaussian variational expectations, stage 1 (likelihoods/base.py: ScalarLikelihood through NDiagGHQuadrature,
// quadrature/gauss_hermite.py; scalar_discrete.py Bernoulli / Poisson / Ordinal; scalar_continuous.py StudentT / Exponential /
// Gamma / Beta; the formulas of every code: include/gpk.h) -----------------------------------------------------------------
//   VE[b,p] = sum_h (w_h / sqrt(pi)) g(mu + sqrt(2 v) x_h),  g = log p(y | f),  with d/dmu and d/dv of that same sum.
// the node table: lik_element.h (gpk_gauss_hermite returns the host copy)
const double gh_x_host[GH_N] = {GPK_GH20_X};
const double gh_w_host[GH_N] = {GPK_GH20_W};

struct LikVarexpArgs {
  LatentMoments m;
  double par0, par1, c0;   // Poisson: binsize, -, log(binsize);  StudentT: scale, df, the f-independent part of log p;
                           // MultiClass: log(1 - eps), log(eps / (C - 1)), their difference
  double *rows_out, *dmu_out, *dvar_out;
  double *part, *part1;    // stage-1 partials of sum VE and (part1 may be null) of sum dVE/dtheta (the code's one trainable parameter)
  // Exponential: nothing;  Gamma: par0 = shape, par1 = psi(shape), c0 = lgamma(shape);  Beta: par0 = scale, par1 = psi(scale),
  // c0 = lgamma(scale);  Ordinal: par0 = sigma and the bin edges, by value:
  int nedge; double edge[GPK_ORDINAL_MAXEDGE];
};

// The lane layout (QuadLanes): lik_element.h; the element body of every code: lik_element_body.inc, included in place.  The P elements of a row sit in adjacent groups of
// one wave, so rows_out is a fixed-order shuffle loop; one partial of sum VE and one of sum dVE/dtheta per block.
template <int LIK>
__global__ __launch_bounds__(RB) void lik_varexp_kernel(LikVarexpArgs a) {
  constexpr int LPE = quad_lpe(LIK);
  __shared__ double sh[4];
  const LatentMoments& m = a.m;
  const QuadLanes<LPE> L(m);
  const int w = threadIdx.x >> 6, k = L.k, p = L.p;
  double acc = 0.0, acc1 = 0.0;
  for (long u = (long)blockIdx.x * (RB / 64) + w; u < L.npass; u += (long)gridDim.x * (RB / 64)) {
    long b; double y, mu, fv;
    const bool act = L.load(m, u, p, b, y, mu, fv);
    double ynan = y - y;
    double ve, dmu, dvar, dsc = 0.0;
#include "lik_element_body.inc"
    double rs = 0.0;   // the row's P elements sit in adjacent groups of this wave: summed in the order p = 0, 1, ...
    for (int q = 0; q < m.P; ++q) rs += __shfl(ve, (L.row_lane0 + q * LPE) & 63);
    if (act && k == 0) {
      const long e = b * m.P + p;
      if (m.fvar_out) m.fvar_out[e] = fv;
      if (a.dmu_out) a.dmu_out[e] = dmu;
      if (a.dvar_out) a.dvar_out[e] = dvar;
      if (a.rows_out && p == 0) a.rows_out[b] = rs;
      acc += ve;
      acc1 += dsc;
    }
  }
  const double r0 = block_sum(acc, sh);
  if (threadIdx.x == 0) a.part[blockIdx.x] = r0;
  if (a.part1) {   // (kernel argument: uniform)
    const double r1 = block_sum(acc1, sh);
    if (threadIdx.x == 0) a.part1[blockIdx.x] = r1;
  }
}

// ---- MultiClass / RobustMax variational expectations, stage 1 (likelihoods/multiclass.py: MultiClass._variational_expectations,
// RobustMax.prob_is_largest) ------------------------------------------------------------------------------------------------
//   y = Y[b, 0] (ONE label column),  s = sqrt(max(2 v_y, 1e-10)),  X_h = mu_y + s x_h,  d_kh = (X_h - mu_k) / sqrt(max(v_k, 1e-10)),
//   c_kh = Phi(d_kh) (1 - 2e-4) + 1e-4,  Pi_h = prod_{k != y} c_kh,  p = sum_h (w_h / sqrt pi) Pi_h,
//   VE_b = p log(1 - eps) + (1 - p) log(eps / (C - 1)),  and the exact derivatives of that sum w.r.t. all C means and variances.
// The lane layout of lik_varexp_kernel carries over -- four adjacent lanes per (row, latent) group, five nodes each, floor(16 / P)
// whole rows per wave pass -- but the P groups of a row are coupled: group k evaluates c_kh and t_kh = (1 - 2e-4) phi(d_kh) /
// (sqrt(v_k) c_kh) at its nodes (group y: c = 1, t = 0), the product over the row's groups is a fixed-order shuffle loop (k = 0, 1,
// ...), and each group then forms its own sums  a1 = sum_h w Pi t,  a2 = sum_h w Pi t d,  a3 = sum_h w Pi t x:
//   dVE/dmu_k = -kappa a1,  dVE/dv_k = -kappa a2 / (2 sqrt v_k)   (k != y);   kappa = log(1 - eps) - log(eps / (C - 1))
//   dVE/dmu_y = kappa sum_k a1_k,  dVE/dv_y = kappa sum_k a3_k / s   (the sums over h and k of the definition, k outermost)
// The clamps are comparisons, so a NaN variance stays NaN; where one is active the derivative w.r.t. that variance is exactly 0
// (tf.clip_by_value under autodiff).  A label that is no integer in [0, P) adds NaN to every output of its row.
// par0 = log(1 - eps), par1 = log(eps / (C - 1)), c0 = kappa.
__global__ __launch_bounds__(RB) void lik_multiclass_kernel(LikVarexpArgs a) {
  constexpr int NPL = GH_N / 4;      // nodes per lane
  __shared__ double sh[4];
  const LatentMoments& m = a.m;
  const QuadLanes<4> L(m);
  const int w = threadIdx.x >> 6, k = L.k, p = L.p, row_lane0 = L.row_lane0;   // (p: the class)
  double acc = 0.0;
  for (long u = (long)blockIdx.x * (RB / 64) + w; u < L.npass; u += (long)gridDim.x * (RB / 64)) {
    long b; double y, mu, fv;
    const bool act = L.load(m, u, 0, b, y, mu, fv);
    const bool lab_ok = y >= 0.0 && y < (double)m.P && y == floor(y);   // (false for NaN and +-Inf)
    const int yi = lab_ok ? (int)y : 0;
    const double ynan = lab_ok ? 0.0 : __builtin_nan("");
    const bool isy = p == yi;
    const int ylane = (row_lane0 + yi * 4) & 63;
    const double mu_y = __shfl(mu, ylane), fv_y = __shfl(fv, ylane);
    const double tv = 2.0 * fv_y;
    const bool clamp_y = tv < 1e-10, clamp_k = fv < 1e-10;
    const double s = sqrt(clamp_y ? 1e-10 : tv);
    const double sdk = sqrt(clamp_k ? 1e-10 : fv);
    double c[NPL], t[NPL], d[NPL], pi[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      d[j] = (fma(s, gh_x_dev[k * NPL + j], mu_y) - mu) / sdk;
      const double cc = 0.5 * erfc(-d[j] * 0.7071067811865476) * (1.0 - 2e-4) + 1e-4;
      const double tt = ((1.0 - 2e-4) * 0.3989422804014327) * exp(-0.5 * d[j] * d[j]) / (sdk * cc);
      c[j] = isy ? 1.0 : cc;
      t[j] = isy ? 0.0 : tt;
      pi[j] = 1.0;
    }
    for (int q = 0; q < m.P; ++q) {   // the row's P groups sit in adjacent groups of this wave: multiplied in the order k = 0, 1, ...
      const int src = (row_lane0 + q * 4 + k) & 63;
#pragma unroll
      for (int j = 0; j < NPL; ++j) pi[j] *= __shfl(c[j], src);
    }
    double sp = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const double wp = gh_w_dev[k * NPL + j] * 0.5641895835477563 * pi[j];   // (w_h / sqrt(pi)) Pi_h
      const double wt = wp * t[j];
      sp += wp;
      a1 += wt;
      a2 += wt * d[j];
      a3 += wt * gh_x_dev[k * NPL + j];
    }
    sp += __shfl_xor(sp, 1); a1 += __shfl_xor(a1, 1); a2 += __shfl_xor(a2, 1); a3 += __shfl_xor(a3, 1);
    sp += __shfl_xor(sp, 2); a1 += __shfl_xor(a1, 2); a2 += __shfl_xor(a2, 2); a3 += __shfl_xor(a3, 2);
    double s1 = 0.0, s3 = 0.0;   // group y collects the others' sums in the order k = 0, 1, ... (its own are zeros)
    for (int q = 0; q < m.P; ++q) {
      const int src = (row_lane0 + q * 4) & 63;
      s1 += __shfl(a1, src);
      s3 += __shfl(a3, src);
    }
    const double ve = sp * a.par0 + (1.0 - sp) * a.par1 + ynan;   // (every lane of the row holds the same bits of sp)
    const double dmu = (isy ? a.c0 * s1 : -a.c0 * a1) + ynan;
    const double dvar = (isy ? (clamp_y ? 0.0 : a.c0 * s3 / s) : (clamp_k ? 0.0 : -a.c0 * a2 / (2.0 * sdk))) + ynan;
    if (act && k == 0) {
      const long e = b * m.P + p;
      if (m.fvar_out) m.fvar_out[e] = fv;
      if (a.dmu_out) a.dmu_out[e] = dmu;
      if (a.dvar_out) a.dvar_out[e] = dvar;
      if (p == 0) {   // one group per row
        if (a.rows_out) a.rows_out[b] = ve;
        acc += ve;
      }
    }
  }
  const double r0 = block_sum(acc, sh);
  if (threadIdx.x == 0) {
    a.part[blockIdx.x] = r0;
    if (a.part1) a.part1[blockIdx.x] = 0.0;
  }
}

// ---- Gaussian variational expectations of linearly mixed latents, stage 1 (kernels/multioutput/kernels.py LinearCoregionalization,
// conditionals/util.py mix_latent_gp, then likelihoods/scalar_continuous.py Gaussian._variational_expectations) -----------------
//   f[b,p] = sum_l W[p,l] gmean[b,l] + mean_const,  fvar[b,p] = sum_l W[p,l]^2 gvar[b,l],  gvar = knn - s0 + ssq (latent_var)
// and the adjoints of sum VE w.r.t. gmean and W (include/gpk.h).  GW = max(L, P) adjacent lanes share a row: lane j of the group
// is latent j (j < L) AND output j (j < P), so the loads of gmean, s0 / ssq and Y of a wave pass are floor(64 / GW) whole rows,
// contiguous.  The P outputs read all L latents of their row and the L latents all P residuals: fixed-order shuffle loops inside
// the wave (l = 0, 1, ... and p = 0, 1, ...), as in lik_multiclass_kernel.  dW: lane (row group, p) keeps L running sums over its
// rows; at the end the row groups of a wave are summed in group order, the waves in wave order (LDS), one [P L] partial per block.
struct MixedVarexpArgs {
  LatentMoments g;    // the L = g.P latents: gmean = g.fmean, Y / ldy the P outputs', g.mean_const added after the mixing
  int P;
  double noise;
  double W[256];      // [P, L] row-major
  double *fmean_out, *fvar_out, *dgmu_out;
  double *part0, *part1, *partW;   // stage-1 partials of sum VE, of sum dVE/ds2 (may be null), of dW [blocks][P L] (may be null)
};
__host__ __device__ constexpr int mixed_rows_per_pass(int L, int P) { return 64 / (L > P ? L : P); }

__global__ __launch_bounds__(RB) void mixed_varexp_kernel(MixedVarexpArgs a) {
  __shared__ double sh[4];
  __shared__ double sW[256];
  __shared__ double sAcc[RB / 64][256];
  const LatentMoments& g = a.g;
  const int L = g.P, P = a.P, GW = L > P ? L : P;
  for (int i = threadIdx.x; i < P * L; i += RB) sW[i] = a.W[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int rpw = mixed_rows_per_pass(L, P), jr = lane / GW, j = lane - jr * GW;
  const int row_lane0 = (jr * GW) & 63;           // lane of the row's first latent / output
  const bool isl = j < L, isp = j < P;
  const int wrow = (isp ? j : 0) * L, wcol = isl ? j : 0;   // this lane's row and column of W
  const long npass = ((long)g.rows + rpw - 1) / rpw;
  const double c0 = -0.5 * 1.8378770664093453 - 0.5 * log(a.noise);
  double acc0 = 0.0, acc1 = 0.0;
  double accW[16];
#pragma unroll
  for (int l = 0; l < 16; ++l) accW[l] = 0.0;
  for (long u = (long)blockIdx.x * (RB / 64) + w; u < npass; u += (long)gridDim.x * (RB / 64)) {
    const long b = u * rpw + jr;
    const bool act = jr < rpw && b < g.rows;   // (an idle lane runs on harmless values and is masked below)
    double gm = 0.0, gv = 0.0, y = 0.0;
    if (act && isl) { gv = latent_var(g, b, j); gm = g.fmean[b * L + j]; }
    if (act && isp) y = g.Y[b * g.ldy + j];
    double f = 0.0, fv = 0.0;
    for (int l = 0; l < L; ++l) {   // the row's L latents sit in adjacent lanes of this wave: summed in the order l = 0, 1, ...
      const double wl = sW[wrow + l];
      f += wl * __shfl(gm, (row_lane0 + l) & 63);
      fv += (wl * wl) * __shfl(gv, (row_lane0 + l) & 63);
    }
    f += g.mean_const;
    const double dy = y - f;
    double dg = 0.0;
    for (int p = 0; p < P; ++p) dg += sW[p * L + wcol] * __shfl(dy, (row_lane0 + p) & 63);   // (p = 0, 1, ...)
    dg /= a.noise;
    if (a.partW) {   // (kernel argument: uniform)
#pragma unroll
      for (int l = 0; l < 16; ++l) {
        if (l < L) {
          const double t = dy * __shfl(gm, (row_lane0 + l) & 63) - sW[wrow + l] * __shfl(gv, (row_lane0 + l) & 63);
          if (act && isp) accW[l] += t;
        }
      }
    }
    if (act && isp) {
      const long e = b * P + j;
      const double q = dy * dy + fv;
      acc0 += c0 - 0.5 * q / a.noise;
      acc1 += -0.5 / a.noise + 0.5 * q / (a.noise * a.noise);
      if (a.fmean_out) a.fmean_out[e] = f;
      if (a.fvar_out) a.fvar_out[e] = fv;
    }
    if (act && isl && a.dgmu_out) a.dgmu_out[b * L + j] = dg;
  }
  const double r0 = block_sum(acc0, sh);
  if (threadIdx.x == 0) a.part0[blockIdx.x] = r0;
  if (a.part1) {
    const double r1 = block_sum(acc1, sh);
    if (threadIdx.x == 0) a.part1[blockIdx.x] = r1;
  }
  if (a.partW) {
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      if (l < L) {
        double s = 0.0;
        for (int r = 0; r < rpw; ++r) s += __shfl(accW[l], r * GW + j);   // the wave's row groups, in group order
        if (jr == 0 && isp) sAcc[w][j * L + l] = s;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < P * L; i += RB) {
      double s = 0.0;
      for (int k = 0; k < RB / 64; ++k) s += sAcc[k][i];                  // the waves, in wave order
      a.partW[(long)blockIdx.x * (P * L) + i] = s / a.noise;
    }
  }
}

// stage-1 blocks of the mixed stage: RB / 64 wave passes of mixed_rows_per_pass rows per block and grid-stride round
int mixed_blocks(int rows, int L, int P) {
  const int rpw = mixed_rows_per_pass(L, P);
  long nb = (((long)rows + rpw - 1) / rpw + RB / 64 - 1) / (RB / 64);
  return (int)(nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb));
}

}  // namespace

LatentMoments gpk_latent_moments(const double* Y, long ldy, const double* fmean, int rows, int P, const double* s0, int s0_per_latent,
                                 const double* ssq, const double* knn_host, int knn_per_latent, double mean_const, double* fvar_out) {
  LatentMoments m{Y, ldy, fmean, rows, P, s0, s0_per_latent, ssq, {}, knn_per_latent, mean_const, fvar_out};
  for (int i = 0; i < (knn_per_latent ? P : 1); ++i) m.knn[i] = knn_host[i];
  return m;
}

int gpk_launch_varexp_stage1(hipStream_t s, const LatentMoments& m, double noise, const double* noise_rows, double* part, int* count) {
  VarexpArgs a{};
  a.m = m; a.noise = noise; a.noise_rows = noise_rows; a.part = part;
  const int nb = nblocks_for((long)m.rows * m.P);
  hipLaunchKernelGGL(varexp_kernel<false>, dim3(nb), dim3(RB), 0, s, a);
  GPK_LAUNCH_CHECK();
  *count = nb;
  return 0;
}
int gpk_launch_varexp_tail(hipStream_t s, const LatentMoments& m, const double* slot, int nt, long strideSlot, double noise,
                           const double* noise_rows, double* part, int* ticket, double* out) {
  if (!slot || !part || !ticket || !out || nt < 0) return GPK_E_ARG;
  VarexpArgs a{};
  a.m = m; a.noise = noise; a.noise_rows = noise_rows; a.part = part;
  a.slot = slot; a.nt = nt; a.strideSlot = strideSlot; a.ticket = ticket; a.out = out;
  long nb = ((long)m.rows * m.P + RB - 1) / RB;
  nb = nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb);
  hipLaunchKernelGGL(varexp_kernel<true>, dim3((unsigned)nb), dim3(RB), 0, s, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_gaussian_varexp_sum(void* stream, const double* Y, long ldy, const double* fmean, int rows, int P, const double* s0,
                                       int s0_per_latent, const double* ssq, const double* knn_host, int knn_per_latent,
                                       double noise_variance, const double* noise_rows, double mean_const, double* fvar_out,
                                       double* out, void* ws, size_t ws_bytes) {
  if ((rows > 0 && (!Y || !fmean)) || !knn_host || !out || P <= 0 || P > 16 || rows < 0) return GPK_E_ARG;
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, gpk_reduce_workspace_bytes(rows)));
  const LatentMoments m = gpk_latent_moments(Y, ldy, fmean, rows, P, s0, s0_per_latent, ssq, knn_host, knn_per_latent, mean_const, fvar_out);
  int nb = 0;
  GPK_TRY(gpk_launch_varexp_stage1((hipStream_t)stream, m, noise_variance, noise_rows, (double*)ws, &nb));
  return gpk_launch_final_one((hipStream_t)stream, (double*)ws, nb, 1.0, 0.0, out);
}

int gpk_launch_mixed_varexp_stage1(hipStream_t s, const LatentMoments& g, int P, const double* W_host, double noise, double* fmean_out,
                                   double* fvar_out, double* dgmu_out, double* part0, double* part1, double* partW, int* count) {
  MixedVarexpArgs a{};
  a.g = g; a.P = P; a.noise = noise;
  for (int i = 0; i < P * g.P; ++i) a.W[i] = W_host[i];
  a.fmean_out = fmean_out; a.fvar_out = fvar_out; a.dgmu_out = dgmu_out;
  a.part0 = part0; a.part1 = part1; a.partW = partW;
  const int nb = mixed_blocks(g.rows, g.P, P);
  hipLaunchKernelGGL(mixed_varexp_kernel, dim3(nb), dim3(RB), 0, s, a);
  GPK_LAUNCH_CHECK();
  *count = nb;
  return 0;
}

extern "C" size_t gpk_mixed_varexp_workspace_bytes(int rows, int L, int P) {
  const size_t parts = (size_t)2 * GPK_REDUCE_MAXPART * sizeof(double);
  if (rows < 0 || L < 1 || L > 16 || P < 1 || P > 16) return parts;
  return parts + (size_t)mixed_blocks(rows, L, P) * P * L * sizeof(double);
}

extern "C" int gpk_mixed_gaussian_varexp_sum(void* stream, const double* Y, long ldy, const double* gmean, int rows, int L, int P,
                                             const double* W_host, const double* s0, int s0_per_latent, const double* ssq,
                                             const double* knn_host, int knn_per_latent, double noise_variance, double mean_const,
                                             double* fmean_out, double* fvar_out, double* dgmu_out, double* dW_out, double* out,
                                             void* ws, size_t ws_bytes) {
  if ((rows > 0 && (!Y || !gmean)) || !W_host || !knn_host || !out || L <= 0 || L > 16 || P <= 0 || P > 16 || rows < 0 ||
      !(noise_variance > 0.0))
    return GPK_E_ARG;
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, gpk_mixed_varexp_workspace_bytes(rows, L, P)));
  hipStream_t s = (hipStream_t)stream;
  const LatentMoments g = gpk_latent_moments(Y, ldy, gmean, rows, L, s0, s0_per_latent, ssq, knn_host, knn_per_latent, mean_const, nullptr);
  double* part = (double*)ws;
  double* partW = part + 2 * GPK_REDUCE_MAXPART;
  int nb = 0;
  GPK_TRY(gpk_launch_mixed_varexp_stage1(s, g, P, W_host, noise_variance, fmean_out, fvar_out, dgmu_out, part,
                                         part + GPK_REDUCE_MAXPART, dW_out ? partW : nullptr, &nb));
  GPK_TRY(gpk_launch_final_one(s, part, nb, 1.0, 0.0, out));
  GPK_TRY(gpk_launch_final_one(s, part + GPK_REDUCE_MAXPART, nb, 1.0, 0.0, out + 1));
  if (!dW_out) return 0;
  // dW = the blocks' [P L] partials summed in block order
  return gpk_combine_parts(stream, partW, nb, (long)P * L, 1, P * L, (long)P * L, 1.0, 0, 1.0, dW_out, (long)P * L);
}

extern "C" int gpk_gauss_hermite(int n, double* x_host, double* w_host) {
  if (!x_host || !w_host) return GPK_E_ARG;
  if (n != GH_N) return GPK_E_UNSUPPORTED;
  for (int i = 0; i < GH_N; ++i) { x_host[i] = gh_x_host[i]; w_host[i] = gh_w_host[i]; }
  return 0;
}

// The one host-side description of a likelihood code: which (params, P) it accepts, its kernel, and the three constants the kernel
// reads.  0, GPK_E_UNSUPPORTED (unknown code) or GPK_E_ARG (parameters, classes).
namespace {
struct LikPlan { void (*kernel)(LikVarexpArgs); double par0, par1, c0; int nedge; const double* edge; };
int lik_plan(int lik, const double* q, int P, LikPlan* o) {
  *o = LikPlan{};
  switch (lik) {
    case GPK_LIK_BERNOULLI_PROBIT: o->kernel = lik_varexp_kernel<GPK_LIK_BERNOULLI_PROBIT>; return 0;
    case GPK_LIK_POISSON_EXP:   // params = {binsize}
      if (!(q && q[0] > 0.0)) return GPK_E_ARG;
      o->kernel = lik_varexp_kernel<GPK_LIK_POISSON_EXP>;
      o->par0 = q[0]; o->c0 = log(q[0]);
      return 0;
    case GPK_LIK_STUDENT_T:   // params = {scale, df}
      if (!(q && q[0] > 0.0 && q[1] > 0.0)) return GPK_E_ARG;
      o->kernel = lik_varexp_kernel<GPK_LIK_STUDENT_T>;
      o->par0 = q[0]; o->par1 = q[1];
      o->c0 = lgamma(0.5 * (q[1] + 1.0)) - lgamma(0.5 * q[1]) - 0.5 * (log(q[0] * q[0]) + log(q[1]) + log(3.141592653589793));
      return 0;
    case GPK_LIK_MULTICLASS_ROBUSTMAX:   // params = {epsilon}; P is the number of classes
      if (!(P >= 2 && P <= 16 && q && q[0] > 0.0 && q[0] < 1.0)) return GPK_E_ARG;
      o->kernel = lik_multiclass_kernel;
      o->par0 = log1p(-q[0]); o->par1 = log(q[0] / (double)(P - 1)); o->c0 = o->par0 - o->par1;
      return 0;
    case GPK_LIK_EXPONENTIAL_EXP: o->kernel = lik_varexp_kernel<GPK_LIK_EXPONENTIAL_EXP>; return 0;
    case GPK_LIK_GAMMA_EXP:   // params = {shape}
      if (!(q && q[0] > 0.0)) return GPK_E_ARG;
      o->kernel = lik_varexp_kernel<GPK_LIK_GAMMA_EXP>;
      o->par0 = q[0]; o->par1 = gpk_digamma(q[0]); o->c0 = lgamma(q[0]);
      return 0;
    case GPK_LIK_BETA_PROBIT:   // params = {scale}
      if (!(q && q[0] > 0.0)) return GPK_E_ARG;
      o->kernel = lik_varexp_kernel<GPK_LIK_BETA_PROBIT>;
      o->par0 = q[0]; o->par1 = gpk_digamma(q[0]); o->c0 = lgamma(q[0]);
      return 0;
    case GPK_LIK_ORDINAL: {   // params = {sigma, n, e_0 .. e_{n-1}}: n is read before any edge
      if (!(q && q[0] > 0.0 && q[1] >= 1.0 && q[1] <= (double)GPK_ORDINAL_MAXEDGE && q[1] == floor(q[1]))) return GPK_E_ARG;
      const int n = (int)q[1];
      for (int i = 0; i < n; ++i)
        if (!(isfinite(q[2 + i]) && (i == 0 || q[2 + i] > q[1 + i]))) return GPK_E_ARG;
      o->kernel = lik_varexp_kernel<GPK_LIK_ORDINAL>;
      o->par0 = q[0]; o->nedge = n; o->edge = q + 2;
      return 0;
    }
    default: return GPK_E_UNSUPPORTED;
  }
}
}  // namespace
int gpk_likelihood_check(int lik, const double* params, int P) {
  LikPlan plan;
  return lik_plan(lik, params, P, &plan);
}
int gpk_likelihood_constants(int lik, const double* params, int P, double* par0, double* par1, double* c0) {
  LikPlan plan;
  GPK_TRY(lik_plan(lik, params, P, &plan));
  *par0 = plan.par0; *par1 = plan.par1; *c0 = plan.c0;
  return 0;
}

int gpk_launch_likelihood_varexp_stage1(hipStream_t s, int lik, const double* params, const LatentMoments& m, double* rows_out,
                                        double* dmu_out, double* dvar_out, double* part, double* part1, int* count) {
  LikPlan plan;
  GPK_TRY(lik_plan(lik, params, m.P, &plan));
  LikVarexpArgs a{};
  a.m = m; a.par0 = plan.par0; a.par1 = plan.par1; a.c0 = plan.c0;
  a.nedge = plan.nedge;
  for (int i = 0; i < plan.nedge; ++i) a.edge[i] = plan.edge[i];
  a.rows_out = rows_out; a.dmu_out = dmu_out; a.dvar_out = dvar_out; a.part = part; a.part1 = part1;
  const int per_wave = quad_rows_per_pass(quad_lpe(lik), m.P);   // (MultiClass: per row, not per element)
  long nb = (((long)m.rows + per_wave - 1) / per_wave + RB / 64 - 1) / (RB / 64);
  nb = nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb);
  void* kargs[] = {&a};
  (void)hipLaunchKernel((const void*)plan.kernel, dim3((unsigned)nb), dim3(RB), kargs, 0, s);   // (status: read and cleared below)
  GPK_LAUNCH_CHECK();
  *count = (int)nb;
  return 0;
}

extern "C" int gpk_likelihood_varexp_sum(void* stream, int lik, const double* lik_params_host, const double* Y, long ldy,
                                         const double* fmean, int rows, int P, const double* s0, int s0_per_latent,
                                         const double* ssq, const double* knn_host, int knn_per_latent, double mean_const,
                                         double* fvar_out, double* rows_out, double* dmu_out, double* dvar_out, double* out,
                                         void* ws, size_t ws_bytes) {
  if ((rows > 0 && (!Y || !fmean)) || !knn_host || !out || P <= 0 || P > 16 || rows < 0) return GPK_E_ARG;
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, gpk_reduce_workspace_bytes(rows)));
  const LatentMoments m = gpk_latent_moments(Y, ldy, fmean, rows, P, s0, s0_per_latent, ssq, knn_host, knn_per_latent, mean_const, fvar_out);
  double* part = (double*)ws;
  int nb = 0;
  GPK_TRY(gpk_launch_likelihood_varexp_stage1((hipStream_t)stream, lik, lik_params_host, m, rows_out, dmu_out, dvar_out, part,
                                              part + GPK_REDUCE_MAXPART, &nb));
  // out[0] = sum VE, out[1] = sum dVE/dtheta of the code's one trainable parameter (the partials of a code without one are zeros)
  GPK_TRY(gpk_launch_final_one((hipStream_t)stream, part, nb, 1.0, 0.0, out));
  return gpk_launch_final_one((hipStream_t)stream, part + GPK_REDUCE_MAXPART, nb, 1.0, 0.0, out + 1);
}
