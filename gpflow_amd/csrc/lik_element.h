// One (row, latent) element of a scalar likelihood's variational expectations, per code, and the lane layout that carries it: shared
// by lik_varexp_kernel / lik_multiclass_kernel (varexp.hip: one code per launch) and switched_varexp_kernel
// (switched/switched_varexp.hip: one code per ROW).  The formulas of every code: include/gpk.h.
#pragma once
#include "reduce_device.h"
#include "digamma.h"

namespace {

// fvar[b,p] = knn - s0 + ssq, in this order and each step a statement of its own: with -ffp-contract=on the bits depend on it.
// slot_sum (varexp_kernel<true>): the last term, already summed from the slot partials in slot order, in place of m.ssq.
__device__ __forceinline__ double latent_var(const LatentMoments& m, long b, int p, const double* slot_sum = nullptr) {
  double fv = m.knn[m.knn_per_latent ? p : 0];
  if (m.s0) fv -= m.s0_per_latent ? m.s0[(long)p * m.rows + b] : m.s0[b];
  if (slot_sum) fv += *slot_sum;
  else if (m.ssq) fv += m.ssq[(long)p * m.rows + b];
  return fv;
}

// numpy.polynomial.hermite.hermgauss(20), the reference's DEFAULT_NUM_GAUSS_HERMITE_POINTS (gpk_gauss_hermite returns this table)
#define GPK_GH20_X                                                                                                          \
  -5.387480890011233, -4.603682449550744, -3.944764040115625, -3.3478545673832163, -2.7888060584281305, -2.2549740020892757, \
      -1.7385377121165861, -1.234076215395323, -0.7374737285453944, -0.24534070830090124, 0.24534070830090124,              \
      0.7374737285453944, 1.234076215395323, 1.7385377121165861, 2.2549740020892757, 2.7888060584281305, 3.3478545673832163, \
      3.944764040115625, 4.603682449550744, 5.387480890011233
#define GPK_GH20_W                                                                                                          \
  2.2293936455341447e-13, 4.3993409922731747e-10, 1.0860693707692782e-07, 7.80255647853206e-06, 0.00022833863601635365,     \
      0.0032437733422378567, 0.024810520887463643, 0.1090172060200233, 0.28667550536283415, 0.4622436696006101,              \
      0.4622436696006101, 0.28667550536283415, 0.1090172060200233, 0.024810520887463643, 0.0032437733422378567,              \
      0.00022833863601635365, 7.80255647853206e-06, 1.0860693707692782e-07, 4.3993409922731747e-10, 2.2293936455341447e-13
constexpr int GH_N = 20;
constexpr int GPK_ORDINAL_MAXEDGE = 15;
__constant__ const double gh_x_dev[GH_N] = {GPK_GH20_X};
__constant__ const double gh_w_dev[GH_N] = {GPK_GH20_W};

// One element (b, p) is shared by LPE = 4 adjacent lanes, five nodes each (8192 x P elements with a serial 20-node loop of fp64
// erfc + log + exp per thread would leave most of the chip idle); the four partial sums meet through two xor shuffles, so all
// four lanes hold the same bits.  The closed-form branches (Poisson, Exponential, Gamma) have no nodes: one lane per element.  A wave pass covers
// floor((64 / LPE) / P) WHOLE rows, so that the row sums of rows_out are a fixed-order shuffle loop inside one wave.
// This layout is written down once, for the kernels and for the launchers' grids:
__host__ __device__ constexpr int quad_lpe(int lik) {   // lanes per element
  return lik == GPK_LIK_POISSON_EXP || lik == GPK_LIK_EXPONENTIAL_EXP || lik == GPK_LIK_GAMMA_EXP ? 1 : 4;
}
__host__ __device__ constexpr int quad_rows_per_pass(int lpe, int P) { return (64 / lpe) / P; }      // (P <= 16 <= 64 / lpe)
template <int LPE>
struct QuadLanes {
  int k, p;        // this lane's node quarter and latent
  int jr, rpw;     // its group's row within a pass, whole rows per pass
  int row_lane0;   // lane of the row's first group
  long npass;
  __device__ explicit QuadLanes(const LatentMoments& m) {
    const int lane = threadIdx.x & 63, g = lane / LPE;
    k = lane % LPE; rpw = quad_rows_per_pass(LPE, m.P);
    jr = g / m.P; p = g - jr * m.P;
    row_lane0 = (jr * m.P * LPE) & 63;
    npass = ((long)m.rows + rpw - 1) / rpw;
  }
  // row b, label (column ycol of Y), mean and variance of this lane's element in pass u; false: an idle lane, which runs on
  // harmless values and is masked by the caller
  __device__ bool load(const LatentMoments& m, long u, int ycol, long& b, double& y, double& mu, double& fv) const {
    b = u * rpw + jr;
    const bool act = jr < rpw && b < m.rows;
    y = 0.0; mu = 0.0; fv = 1.0;
    if (act) {
      fv = latent_var(m, b, p);
      mu = m.fmean[b * m.P + p] + m.mean_const;
      y = m.Y[b * m.ldy + ycol];
    }
    return act;
  }
};

// The element (label y, mean mu, variance fv) under code LIK on the lane that holds node quarter k, for a kernel that picks the
// code per row: lik_element_body.inc (which also says what `a` holds) behind a function.  Closed forms: every lane of the element
// evaluates the same expression.
template <int LIK, class A>
__device__ __forceinline__ void lik_element(const A& a, int k, double y, double mu, double fv, double& ve_out, double& dmu_out,
                                            double& dvar_out, double& dsc_out) {
  double ynan = y - y;
  double ve, dmu, dvar, dsc = 0.0;
#include "lik_element_body.inc"
  ve_out = ve; dmu_out = dmu; dvar_out = dvar; dsc_out = dsc;
}

}  // namespace
