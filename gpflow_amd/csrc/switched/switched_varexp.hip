// The variational-expectation stage of a SWITCHED likelihood (gpflow/likelihoods/misc.py `SwitchedLikelihood`): every row carries a
// task label in one column of Y and is scored by its own task's likelihood -- a Gaussian, or one of the scalar codes of
// gpk_likelihood_varexp_sum -- in ONE launch, gfx950.  Contract: include/gpk.h (gpk_switched_varexp_sum).
//
// Lanes.  The layout of lik_varexp_kernel (lik_element.h: QuadLanes<4>): four adjacent lanes per (row, latent) element, five
// Gauss-Hermite nodes each, floor(16 / P) whole rows per wave pass, a grid-stride loop over the passes under the 1024-block clamp.
// The closed-form members (Gaussian, Poisson, Exponential, Gamma) are evaluated identically by the four lanes of a group; lane
// k == 0 stores.
//
// The choice per row is a WATERFALL, not a lane-divergent switch over seven bodies: per pass the wave loops over the DISTINCT tasks
// among its rows.  The current task is the task of the first lane that is still waiting, read into a scalar register, so the code
// and its three constants are wave-uniform inside an iteration -- scalar reads of the by-value table in the kernel arguments, 32
// bytes per task -- and the `switch` is a uniform branch; the lanes of that task evaluate, the others are masked.  A wave whose rows
// share one task runs one body once (data stacked task by task costs what the single-likelihood kernel costs); a wave with k tasks
// costs k bodies.  The four lanes of an element and the P elements of a row share the row's task, so the xor shuffles inside an
// element body and the row sum always meet active lanes.
//
// Sums.  sum VE: one accumulator per lane, block_sum, one partial per block.  sum dVE/dtheta_t: the waterfall loop itself is
// wave-uniform, so after an iteration's body all 64 lanes are back and the iteration's contributions (0.0 from the lanes of other
// tasks) are summed over the wave in the fixed shuffle order of wave_sum, and lane 0 adds the result to the wave's LDS slot of that
// task; at the end of the block the waves are combined in index order.  parts[(1 + T) block + j].  A one-workgroup tail sums the
// blocks' partials per entry in a fixed order.  No floating-point atomics; each element's outputs depend on its own row alone.
#include "../lik_element.h"
#include "../label.h"   // label_of

namespace {

constexpr int MAXT = 16;

struct SwitchedEntry {   // one task of the table: 32 bytes
  double par0, par1, c0;   // lik_element_body.inc; Gaussian: par0 = the variance s2, c0 = -log(2 pi) / 2 - log(s2) / 2
  int code;                // GPK_LIK_* or 0 (Gaussian)
  int has_grad;            // the code has a trainable parameter: its sum of dVE/dtheta is formed
};

struct SwitchedArgs {
  LatentMoments m;
  int T, ylab;
  SwitchedEntry tab[MAXT];
  double *rows_out, *dmu_out, *dvar_out;
  double* parts;           // [blocks][1 + T]
};

// the Gaussian member: closed form, every lane of the element the same expression; dsc = dVE/ds2.  A non-finite label adds y - y to
// every output, as for the scalar codes (dvar alone would not see it).
__device__ __forceinline__ void gaussian_element(const SwitchedEntry& a, double y, double mu, double fv, double& ve, double& dmu,
                                                 double& dvar, double& dsc) {
  const double ynan = y - y;
  const double dy = y - mu;
  const double q = dy * dy + fv;
  ve = a.c0 - 0.5 * q / a.par0 + ynan;
  dmu = dy / a.par0 + ynan;
  dvar = -0.5 / a.par0 + ynan;
  dsc = -0.5 / a.par0 + 0.5 * q / (a.par0 * a.par0);
}

// HEAVY = true adds the two bodies that call lgamma on the device, Beta and Poisson.  Beta needs 256 VGPRs and AGPRs on its own
// (lik_varexp_kernel<10>) and Poisson's lgamma about 100 more than any other body: with Poisson inside, the light instantiation
// came to 256 VGPRs + 6 AGPRs, one wave per SIMD for a Gaussian + StudentT table too, and bounded to two waves it spilled to
// scratch.  A table with neither code runs the instantiation without them, at the occupancy of its own bodies.
template <bool HEAVY>
__global__ __launch_bounds__(RB) void switched_varexp_kernel(SwitchedArgs a) {
  __shared__ double sh[4];
  __shared__ double s_task[RB / 64][MAXT];   // per wave: the running sum of dVE/dtheta_t of its rows
  const LatentMoments& m = a.m;
  const QuadLanes<4> L(m);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, k = L.k, p = L.p;
  // a wave only ever touches its own slots, so there is no barrier until the end: lanes 0 .. 15 zero them here and lane 0 alone adds to
  // them below, which relies on the LDS operations of ONE wave being carried out in the order they are issued
  if (lane < MAXT) s_task[w][lane] = 0.0;
  double acc = 0.0;
  for (long u = (long)blockIdx.x * (RB / 64) + w; u < L.npass; u += (long)gridDim.x * (RB / 64)) {
    long b; double y, mu, fv;
    const bool act = L.load(m, u, p, b, y, mu, fv);
    // the row's task; -1: an invalid label (the row's outputs are NaN, it belongs to no task) or an idle lane
    const int t = act ? label_of(m.Y[b * m.ldy + a.ylab], a.T) : -1;
    if (act && k == 0 && m.fvar_out) m.fvar_out[b * m.P + p] = fv;   // (before the bodies: fv does not stay live across them)
    double ve = __builtin_nan(""), dmu = ve, dvar = ve;
    unsigned long long waiting = __ballot(t >= 0);
    while (waiting) {   // (wave-uniform: one iteration per distinct task of this pass)
      const int tc = __builtin_amdgcn_readlane(t, __builtin_ctzll(waiting));   // the first waiting lane's task, in a scalar register
      const SwitchedEntry& q = a.tab[tc];
      const bool mine = t == tc;
      double dsc = 0.0;
      if (mine) {
        switch (q.code) {   // (uniform)
          case 0: gaussian_element(q, y, mu, fv, ve, dmu, dvar, dsc); break;
          case GPK_LIK_BERNOULLI_PROBIT: lik_element<GPK_LIK_BERNOULLI_PROBIT>(q, k, y, mu, fv, ve, dmu, dvar, dsc); break;
          case GPK_LIK_POISSON_EXP:
            if constexpr (HEAVY) lik_element<GPK_LIK_POISSON_EXP>(q, k, y, mu, fv, ve, dmu, dvar, dsc);
            break;
          case GPK_LIK_STUDENT_T: lik_element<GPK_LIK_STUDENT_T>(q, k, y, mu, fv, ve, dmu, dvar, dsc); break;
          case GPK_LIK_EXPONENTIAL_EXP: lik_element<GPK_LIK_EXPONENTIAL_EXP>(q, k, y, mu, fv, ve, dmu, dvar, dsc); break;
          case GPK_LIK_GAMMA_EXP: lik_element<GPK_LIK_GAMMA_EXP>(q, k, y, mu, fv, ve, dmu, dvar, dsc); break;
          default:   // (GPK_LIK_BETA_PROBIT: the host admits no other code)
            if constexpr (HEAVY) lik_element<GPK_LIK_BETA_PROBIT>(q, k, y, mu, fv, ve, dmu, dvar, dsc);
            break;
        }
      }
      if (q.has_grad) {   // (uniform) every lane is back: the task's contributions of this pass, in wave_sum's order
        const double s = wave_sum(mine && k == 0 ? dsc : 0.0);
        if (lane == 0) s_task[w][tc] += s;
      }
      waiting &= ~__ballot(mine);
    }
    double rs = 0.0;   // the row's P elements sit in adjacent groups of this wave: summed in the order p = 0, 1, ...
    for (int j = 0; j < m.P; ++j) rs += __shfl(ve, (L.row_lane0 + j * 4) & 63);
    if (act && k == 0) {
      const long e = b * m.P + p;
      if (a.dmu_out) a.dmu_out[e] = dmu;
      if (a.dvar_out) a.dvar_out[e] = dvar;
      if (a.rows_out && p == 0) a.rows_out[b] = rs;
      acc += ve;
    }
  }
  double* part = a.parts + (long)blockIdx.x * (1 + a.T);
  const double r0 = block_sum(acc, sh);   // (its barriers also publish s_task)
  if (threadIdx.x == 0) part[0] = r0;
  if (threadIdx.x < a.T) {
    double s = 0.0;
    for (int i = 0; i < RB / 64; ++i) s += s_task[i][threadIdx.x];   // the waves, in wave order
    part[1 + threadIdx.x] = s;
  }
}

// out[j] = the sum over the blocks of parts[block][j], j < n: one workgroup, entry after entry, block_sum's fixed order
struct SwitchedTailArgs { const double* parts; int nb, n; double* out; };
__global__ __launch_bounds__(RB) void switched_tail_kernel(SwitchedTailArgs a) {
  __shared__ double sh[4];
  for (int j = 0; j < a.n; ++j) {
    double v = 0.0;
    for (int i = threadIdx.x; i < a.nb; i += RB) v += a.parts[(long)i * a.n + j];
    const double r = block_sum(v, sh);
    if (threadIdx.x == 0) a.out[j] = r;
  }
}

int switched_blocks(int rows, int P) {
  const int rpw = quad_rows_per_pass(4, P);
  long nb = (((long)rows + rpw - 1) / rpw + RB / 64 - 1) / (RB / 64);
  nb = nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb);
  return (int)nb;
}

}  // namespace

extern "C" int gpk_switched_varexp_blocks(int rows, int P) {
  if (rows < 0 || P < 1 || P > 16) return 1;
  return switched_blocks(rows, P);
}

extern "C" int gpk_switched_varexp_sum(void* stream, int T, const int* codes_host, const double* params_host, const double* Y, long ldy,
                                       int ylab, const double* fmean, int rows, int P, const double* s0, int s0_per_latent,
                                       const double* ssq, const double* knn_host, int knn_per_latent, double mean_const,
                                       double* fvar_out, double* rows_out, double* dmu_out, double* dvar_out, double* out,
                                       double* parts) {
  if (T < 1 || T > MAXT || P < 1 || P > 16 || rows < 0 || !codes_host || !params_host || !knn_host || !out) return GPK_E_ARG;
  if (rows > 0 && (!Y || !fmean || !parts)) return GPK_E_ARG;
  if (ylab < P || (rows > 0 && ldy <= (long)ylab)) return GPK_E_ARG;   // the value columns are 0 .. P - 1; the label lies in the row
  SwitchedArgs a{};
  bool heavy = false;
  for (int t = 0; t < T; ++t) {
    const int code = codes_host[t];
    const double* q = params_host + 2 * t;
    SwitchedEntry& e = a.tab[t];
    e.code = code;
    if (code == 0) {   // Gaussian: params = {variance}
      if (!(q[0] > 0.0)) return GPK_E_ARG;
      e.par0 = q[0]; e.c0 = -0.5 * 1.8378770664093453 - 0.5 * log(q[0]);
      e.has_grad = 1;
      continue;
    }
    // MultiClass couples the latents of a row; Ordinal needs an edge table per task
    if (code == GPK_LIK_MULTICLASS_ROBUSTMAX || code == GPK_LIK_ORDINAL) return GPK_E_UNSUPPORTED;
    GPK_TRY(gpk_likelihood_constants(code, q, P, &e.par0, &e.par1, &e.c0));   // (an unknown code: GPK_E_UNSUPPORTED)
    e.has_grad = code == GPK_LIK_STUDENT_T || code == GPK_LIK_GAMMA_EXP || code == GPK_LIK_BETA_PROBIT;
    heavy = heavy || code == GPK_LIK_BETA_PROBIT || code == GPK_LIK_POISSON_EXP;
  }
  hipStream_t s = (hipStream_t)stream;
  int nb = 0;
  if (rows > 0) {
    a.m = gpk_latent_moments(Y, ldy, fmean, rows, P, s0, s0_per_latent, ssq, knn_host, knn_per_latent, mean_const, fvar_out);
    a.T = T; a.ylab = ylab;
    a.rows_out = rows_out; a.dmu_out = dmu_out; a.dvar_out = dvar_out; a.parts = parts;
    nb = switched_blocks(rows, P);
    if (heavy) hipLaunchKernelGGL(switched_varexp_kernel<true>, dim3((unsigned)nb), dim3(RB), 0, s, a);
    else hipLaunchKernelGGL(switched_varexp_kernel<false>, dim3((unsigned)nb), dim3(RB), 0, s, a);
    GPK_LAUNCH_CHECK();
  }
  SwitchedTailArgs ta{parts, nb, 1 + T, out};   // (rows = 0: no block, out = 0)
  hipLaunchKernelGGL(switched_tail_kernel, dim3(1), dim3(RB), 0, s, ta);
  GPK_LAUNCH_CHECK();
  return 0;
}
