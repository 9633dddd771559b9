// The body of one (row, latent) element under likelihood code LIK -- a FRAGMENT, included inside a function: textually in
// lik_varexp_kernel<LIK> (varexp.hip), whose instantiations so keep the registers they had when the body was written there, and in
// lik_element<LIK> (lik_element.h) for kernels that choose the code per row.  It reads  LIK (a constant expression), `a` (members
// par0, par1, c0 and, Ordinal, nedge / edge[]), k (the lane's node quarter), y, mu, fv  and `ynan` (= y - y at entry); it assigns
// ve, dmu, dvar and (declared as 0.0) dsc = dVE/dtheta of the code's one trainable parameter.
//   Poisson: par0 = binsize, c0 = log(binsize);  StudentT: par0 = scale, par1 = df, c0 = the f-independent part of log p;
//   Gamma: par0 = shape, par1 = psi(shape), c0 = lgamma(shape);  Beta: par0 = scale, par1 = psi(scale), c0 = lgamma(scale);
//   Ordinal: par0 = sigma and the bin edges (read by comparison: no indexed copy of the table).
// Non-finite inputs: NaN / Inf in mu or fv travel through the arithmetic; a non-finite label adds y - y = NaN to every output
// of its element (the comparison y == 1 of the Bernoulli density would otherwise read a NaN label as class 0).  Ordinal: a label that
// is no integer in [0, nedge] adds NaN instead (the MultiClass rule), to the parameter derivative as well.
// The node loop of the Beta branch is NOT unrolled: each node holds two lgamma and two gpk_digamma, and five inlined copies of
// them buy nothing but registers (DESIGN.md section 6 has the compiler's figures for every instantiation).
// The quadrature codes end in two xor shuffles over the element's four lanes: all four must be active.
{
  constexpr int NPL = GH_N / 4;      // nodes per lane (quadrature branches)
  constexpr int NODE_UNROLL = LIK == GPK_LIK_BETA_PROBIT ? 1 : NPL;
  if (LIK == GPK_LIK_POISSON_EXP) {
    // scalar_discrete.py: Poisson.variational_expectations with the exp link, closed form
    const double e = exp(mu + 0.5 * fv) * a.par0;
    ve = y * mu - e - lgamma(y + 1.0) + y * a.c0;
    dmu = y - e;
    dvar = -0.5 * e;
  } else if (LIK == GPK_LIK_EXPONENTIAL_EXP) {
    // scalar_continuous.py: Exponential.variational_expectations with the exp link, closed form
    const double ye = y * exp(0.5 * fv - mu);
    ve = -mu - ye;
    dmu = ye - 1.0;
    dvar = -0.5 * ye;
  } else if (LIK == GPK_LIK_GAMMA_EXP) {
    // scalar_continuous.py: Gamma.variational_expectations with the exp link, closed form; log y as it comes (no clamp)
    const double ye = y * exp(0.5 * fv - mu);
    const double ly = log(y);
    ve = -a.par0 * mu - a.c0 + (a.par0 - 1.0) * ly - ye;
    dmu = ye - a.par0;
    dvar = -0.5 * ye;
    dsc = ly - mu - a.par1;
  } else {
    const double sd = sqrt(2.0 * fv);
    const double sgn = (y == 1.0) ? 1.0 : -1.0;
    // Beta: the clipped label's two logarithms, once per element (comparisons: a NaN label stays NaN)
    const double yc = y < 1e-6 ? 1e-6 : (y > 1.0 - 1e-6 ? 1.0 - 1e-6 : y);
    const double ly = LIK == GPK_LIK_BETA_PROBIT ? log(yc) : 0.0, l1y = LIK == GPK_LIK_BETA_PROBIT ? log(1.0 - yc) : 0.0;
    // Ordinal: the two edges of the label's bin, picked by comparison (the table is a kernel argument: no indexed copy of it);
    // has_l / has_r: the edge is finite, i.e. not the open end of the first or last bin
    double el = 0.0, er = 0.0;
    bool has_l = false, has_r = false;
    if constexpr (LIK == GPK_LIK_ORDINAL) {   // (constexpr: the one place that reads nedge / edge[], which only Ordinal's caller has)
      const bool lab_ok = y >= 0.0 && y <= (double)a.nedge && y == floor(y);   // (false for NaN and +-Inf)
      const int yi = lab_ok ? (int)y : 0;
      ynan = lab_ok ? 0.0 : __builtin_nan("");
      has_l = yi < a.nedge; has_r = yi > 0;
#pragma unroll
      for (int i = 0; i < GPK_ORDINAL_MAXEDGE; ++i) {
        el = i == yi ? a.edge[i] : el;
        er = i == yi - 1 ? a.edge[i] : er;
      }
    }
    double sv = 0.0, sm = 0.0, sx = 0.0, ss = 0.0;
#pragma unroll NODE_UNROLL
    for (int j = 0; j < NPL; ++j) {
      const double x = gh_x_dev[k * NPL + j];
      const double wn = gh_w_dev[k * NPL + j] * 0.5641895835477563;   // w_h / sqrt(pi)
      const double f = fma(sd, x, mu);
      double gv, gp;
      if (LIK == GPK_LIK_BERNOULLI_PROBIT) {
        // log(y == 1 ? p : 1 - p), p = inv_probit(f) = 0.5 (1 + erf(f / sqrt 2)) (1 - 2e-3) + 1e-3;  1 - p = inv_probit(-f), taken
        // through erfc so that the small side keeps its relative accuracy
        const double q = 0.5 * erfc(-sgn * f * 0.7071067811865476) * (1.0 - 2e-3) + 1e-3;
        gv = log(q);
        gp = sgn * ((1.0 - 2e-3) * 0.3989422804014327) * exp(-0.5 * f * f) / q;
      } else if (LIK == GPK_LIK_BETA_PROBIT) {
        // logdensities.py beta with alpha = m scale, beta = scale - alpha, m = inv_probit(f)
        const double mm = 0.5 * erfc(-f * 0.7071067811865476) * (1.0 - 2e-3) + 1e-3;
        const double al = mm * a.par0, be = a.par0 - al;
        const double pa = gpk_digamma(al), pb = gpk_digamma(be);
        gv = (al - 1.0) * ly + (be - 1.0) * l1y + a.c0 - lgamma(al) - lgamma(be);
        gp = a.par0 * ((1.0 - 2e-3) * 0.3989422804014327) * exp(-0.5 * f * f) * (ly - l1y - pa + pb);
        ss += wn * (mm * ly + (1.0 - mm) * l1y + a.par1 - mm * pa - (1.0 - mm) * pb);
      } else if (LIK == GPK_LIK_ORDINAL) {
        // scalar_discrete.py Ordinal: log(inv_probit(zl) - inv_probit(zr) + 1e-6); the open end of a bin is +-Inf in z (erfc gives
        // exactly 0 or 2 there) and has no density term.  The difference of the two Phi through erfc on the side where both are small.
        const double zl = has_l ? (el - f) / a.par0 : __builtin_inf();
        const double zr = has_r ? (er - f) / a.par0 : -__builtin_inf();
        const bool right = zr >= 0.0;
        const double za = right ? zr : -zl, zb = right ? zl : -zr;
        const double D = (1.0 - 2e-3) * (0.5 * (erfc(za * 0.7071067811865476) - erfc(zb * 0.7071067811865476)));
        const double pl = has_l ? 0.3989422804014327 * exp(-0.5 * zl * zl) : 0.0;
        const double pr = has_r ? 0.3989422804014327 * exp(-0.5 * zr * zr) : 0.0;
        const double den = a.par0 * (D + 1e-6);
        gv = log(D + 1e-6);
        gp = -(1.0 - 2e-3) * (pl - pr) / den;
        ss += wn * (-(1.0 - 2e-3) * ((has_l ? zl * pl : 0.0) - (has_r ? zr * pr : 0.0)) / den);
      } else {
        // logdensities.py student_t:  c0 - (df + 1) / 2 log(1 + ((y - f) / scale)^2 / df)
        const double r = (y - f) / a.par0;
        const double den = a.par1 + r * r;
        gv = a.c0 - 0.5 * (a.par1 + 1.0) * log1p(r * r / a.par1);
        gp = (a.par1 + 1.0) * r / (a.par0 * den);
        ss += wn * (((a.par1 + 1.0) * r * r / den - 1.0) / a.par0);
      }
      sv += wn * gv;
      sm += wn * gp;
      sx += wn * gp * x;
    }
    sv += __shfl_xor(sv, 1); sm += __shfl_xor(sm, 1); sx += __shfl_xor(sx, 1); ss += __shfl_xor(ss, 1);
    sv += __shfl_xor(sv, 2); sm += __shfl_xor(sm, 2); sx += __shfl_xor(sx, 2); ss += __shfl_xor(ss, 2);
    ve = sv;
    dmu = sm;
    dvar = sx / sd;
    dsc = ss;
  }
  ve += ynan; dmu += ynan; dvar += ynan;
  if (LIK == GPK_LIK_ORDINAL) dsc += ynan;
}
