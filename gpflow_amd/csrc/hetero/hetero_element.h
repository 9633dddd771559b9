// One ROW of the heteroskedastic Normal likelihood (likelihoods/multilatent.py HeteroskedasticTFPConditional): y | f, g ~
// N(f, s(g)^2), q(f) = N(m1, v1), q(g) = N(m2, v2), s = exp or softplus.  The bodies are written once here and used by both kernels of
// hetero_varexp.hip (the variational expectations and the predictive quantities).  Formulas and the contract: include/gpk.h.
//
// Lanes.  LINK_EXP has no nodes: one lane holds the row.  LINK_SOFTPLUS spreads the 20 Gauss-Hermite nodes over g on LPR = 4 adjacent
// lanes, five each (lane k: nodes 5 k .. 5 k + 4, as lik_element_body.inc), and the partial sums meet through two xor shuffles, so
// the four lanes end with the same bits.  The predictive log density is a node rule under BOTH links, in the link's own layout.
#pragma once
#include "../lik_element.h"

namespace {

struct HeteroRow { double y, m1, v1, m2, v2; };

template <int LINK> constexpr int hetero_lpr() { return LINK == GPK_HETERO_LINK_EXP ? 1 : 4; }   // lanes per row

constexpr double HETERO_HALF_LOG_2PI = 0.91893853320467274178;
constexpr double HETERO_INV_SQRT_PI = 0.5641895835477563;
// below this g softplus IS exp to fp64: log1p(e^g) = e^g (1 - e^g / 2 + ...), and e^-37 = 8.6e-17 < 2^-53
constexpr double HETERO_SOFTPLUS_EXP_BELOW = -37.0;

template <int LPR>
__device__ __forceinline__ double hetero_group_sum(double v) {
  if constexpr (LPR == 4) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); }
  return v;
}
// a maximum that keeps a NaN (fmax drops it): the log-sum-exp of a row with a NaN term is NaN
__device__ __forceinline__ double hetero_nanmax(double a, double b) { return (a > b || a != a) ? a : b; }

// s = softplus(g) and what the derivatives of log s and s^-2 are made of: logs = log s, sr = sigma(g) / s = (log s)', tau = 1 - sigma(g),
// h2 = s^-2.  g >= 0: s = g + log1p(e^-g) -- no overflow, and g itself from g > 37 on; -37 <= g < 0: s = log1p(e^g);
// g < -37: the exp forms (s = e^g, log s = g, sr = 1, tau = 1, s^-2 = e^-2g), every one within e^-37 relative of the exact value, so
// neither log s nor s^-2 loses the tail where e^g is tiny (or underflows: s^-2 = e^-2g overflows to +Inf by IEEE from g < -354.9).
__device__ __forceinline__ void softplus_parts(double g, double& s, double& logs, double& sr, double& tau, double& h2) {
  if (g < HETERO_SOFTPLUS_EXP_BELOW) {
    s = exp(g); logs = g; sr = 1.0; tau = 1.0; h2 = exp(-2.0 * g);
    return;
  }
  const double e = exp(-fabs(g));
  const double l = log1p(e);
  const double q = 1.0 / (1.0 + e);
  const bool pos = g >= 0.0;
  s = pos ? g + l : l;
  const double sig = pos ? q : e * q;
  tau = pos ? e * q : q;
  const double r = 1.0 / s;
  logs = log(s);
  sr = sig * r;
  h2 = r * r;
}

// The two expectations over g and their derivatives: E1 = E[log s], E2 = E[s^-2]; E1m, E2m = d/dm2; E1v, E2v = d/dv2.
// exp: closed forms.  softplus: ONE pass over the nodes g_h = m2 + sqrt(2 v2) x_h with six running sums; dE[h]/dm = E[h'] and
// dE[h]/dv = E[h''] / 2 (nothing is divided by sqrt(v2): v2 = 0 is the one-point value), with
//   (log s)'' = tau sr - sr^2,   (s^-2)' = -2 sr s^-2,   (s^-2)'' = s^-2 (6 sr^2 - 2 tau sr).
template <int LINK>
__device__ __forceinline__ void hetero_expectations(const HeteroRow& r, int k, double& E1, double& E1m, double& E1v, double& E2,
                                                    double& E2m, double& E2v) {
  if constexpr (LINK == GPK_HETERO_LINK_EXP) {
    E2 = exp(2.0 * r.v2 - 2.0 * r.m2);   // (+Inf by IEEE where it overflows: no clamp)
    E1 = r.m2; E1m = 1.0; E1v = 0.0;
    E2m = -2.0 * E2; E2v = 2.0 * E2;
  } else {
    constexpr int LPR = 4, NPL = GH_N / LPR;
    const double sd = sqrt(2.0 * r.v2);
    double a1 = 0.0, a1m = 0.0, a1v = 0.0, a2 = 0.0, a2m = 0.0, a2v = 0.0;
#pragma unroll 1
    for (int j = 0; j < NPL; ++j) {
      const double wn = gh_w_dev[k * NPL + j] * HETERO_INV_SQRT_PI;
      const double g = fma(sd, gh_x_dev[k * NPL + j], r.m2);
      double s, logs, sr, tau, h2;
      softplus_parts(g, s, logs, sr, tau, h2);
      const double ts = tau * sr, s2 = sr * sr;
      a1 += wn * logs;
      a1m += wn * sr;
      a1v += wn * (ts - s2);
      a2 += wn * h2;
      a2m += wn * (-2.0 * sr * h2);
      a2v += wn * (h2 * (6.0 * s2 - 2.0 * ts));
    }
    E1 = hetero_group_sum<LPR>(a1); E1m = hetero_group_sum<LPR>(a1m); E1v = 0.5 * hetero_group_sum<LPR>(a1v);
    E2 = hetero_group_sum<LPR>(a2); E2m = hetero_group_sum<LPR>(a2m); E2v = 0.5 * hetero_group_sum<LPR>(a2v);
  }
}

// VE = -log(2 pi) / 2 - E1 - a E2 / 2 with a = (y - m1)^2 + v1, and its four seeds.  rn = 0, or NaN where any of the row's five
// operands is not finite (x - x): added to every output, so that such a row is NaN in ALL of them (dv1 = -E2 / 2 alone would not see
// a NaN label) and in the sum, and in nothing else.
template <int LINK>
__device__ __forceinline__ void hetero_varexp_element(const HeteroRow& r, int k, double& ve, double& dm1, double& dv1, double& dm2,
                                                      double& dv2) {
  double E1, E1m, E1v, E2, E2m, E2v;
  hetero_expectations<LINK>(r, k, E1, E1m, E1v, E2, E2m, E2v);
  const double rn = (r.y - r.y) + (r.m1 - r.m1) + (r.v1 - r.v1) + (r.m2 - r.m2) + (r.v2 - r.v2);
  const double dy = r.y - r.m1;
  const double a = dy * dy + r.v1;
  ve = -HETERO_HALF_LOG_2PI - E1 - 0.5 * a * E2 + rn;
  dm1 = dy * E2 + rn;
  dv1 = -0.5 * E2 + rn;
  dm2 = -E1m - 0.5 * a * E2m + rn;
  dv2 = -E1v - 0.5 * a * E2v + rn;
}

// The predictive variance v1 + E[s(g)^2] and, with LD, log sum_h (w_h / sqrt pi) N(y | m1, v1 + s(g_h)^2): a max-shifted log-sum-exp
// over the 20 nodes of g, the terms kept in registers between the two sweeps (20 / LPR per lane).  NaN terms stay NaN (hetero_nanmax);
// a row whose every term is -Inf is -Inf.
template <int LINK, bool LD>
__device__ __forceinline__ void hetero_predict_element(const HeteroRow& r, int k, double& var, double& ld) {
  constexpr int LPR = hetero_lpr<LINK>(), NPL = GH_N / LPR;
  constexpr bool NODES = LD || LINK == GPK_HETERO_LINK_SOFTPLUS;
  double es2 = 0.0;
  ld = 0.0;
  if constexpr (NODES) {
    const double sd = sqrt(2.0 * r.v2);
    const double dy = r.y - r.m1;
    const double dy2 = dy * dy;
    double t[LD ? NPL : 1];
    double mx = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const double wn = gh_w_dev[k * NPL + j] * HETERO_INV_SQRT_PI;
      const double g = fma(sd, gh_x_dev[k * NPL + j], r.m2);
      double s2;
      if constexpr (LINK == GPK_HETERO_LINK_EXP) {
        s2 = exp(2.0 * g);
      } else {
        double s, logs, sr, tau, h2;
        softplus_parts(g, s, logs, sr, tau, h2);
        s2 = s * s;
        es2 += wn * s2;
      }
      if constexpr (LD) {
        const double V = r.v1 + s2;
        t[j] = log(wn) - HETERO_HALF_LOG_2PI - 0.5 * (log(V) + dy2 / V);
        mx = hetero_nanmax(t[j], mx);
      }
    }
    if constexpr (LD) {
      if constexpr (LPR == 4) { mx = hetero_nanmax(__shfl_xor(mx, 1), mx); mx = hetero_nanmax(__shfl_xor(mx, 2), mx); }
      double se = 0.0;
#pragma unroll
      for (int j = 0; j < NPL; ++j) se += exp(t[j] - mx);
      se = hetero_group_sum<LPR>(se);
      ld = mx == -__builtin_inf() ? mx : mx + log(se);
    }
  }
  if constexpr (LINK == GPK_HETERO_LINK_EXP) var = r.v1 + exp(2.0 * r.m2 + 2.0 * r.v2);
  else var = r.v1 + hetero_group_sum<LPR>(es2);
}

}  // namespace
