// Host-side orchestration (no device code here) of everything that CALLS the factorisation (potrf.hip, gpk_potrf_core): the
// projection onto q_sqrt and the fused model drivers -- GPR.log_marginal_likelihood, one shard of SVGP.elbo in its three forms
// (whitened; un-whitened with a full or a diagonal q_sqrt), and the shard with separate kernels per latent, whose latents stay
// independent (SeparateIndependent) or are mixed into the outputs (LinearCoregionalization).  The forms are
// built from the same named pieces; WHICH kernel goes on which stream in which order is measured schedule and differs per form.
#include "gpk_internal.h"

// ---- projection:  ssq[p,b] = sum_j ( sum_k At[b,k] Lq_p[k,j] )^2 ---------------------------------------
extern "C" size_t gpk_project_workspace_bytes(int rows, int m, int P) {
  return (size_t)P * 2 * gpk_gemm_tiles_n(m) * rows * sizeof(double);
}

namespace {
// the GEMM alone: partials [P][nt = 2 * tiles_n][rows] in ws, one per 64 output columns.
// V [m, P] (may be null) asks for the row statistics of At as well: s0[b] = sum_k At[b,k]^2, fmean[b,p] = sum_k At[b,k] V[k,p].
// They come out of the GEMM itself where it runs on the 128 x 128 fast tile and P <= 4 (the headline: no pass over At of their
// own); everywhere else -- more latents, the small-tile and generic kernels, one At per latent -- from gpk_row_stats, in front of
// the GEMM as before.  This is the only place that decides.
int project_parts(hipStream_t s, const double* At, int rows, int m, long ldat, long strideAt, const double* LqT, long ldl, int P, void* ws,
                  size_t ws_bytes, const double* V = nullptr, double* s0 = nullptr, double* fmean = nullptr) {
  if ((!At && rows > 0) || !LqT || rows < 0 || m <= 0 || P <= 0 || strideAt < 0) return GPK_E_ARG;
  if (V && ((rows > 0 && (!s0 || !fmean)) || strideAt != 0)) return GPK_E_ARG;
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, gpk_project_workspace_bytes(rows, m, P)));
  if (rows == 0) return 0;
  const int nt = 2 * gpk_gemm_tiles_n(m);
  GemmArgs g = gemm_base(rows, m, m, 1.0, At, ldat, LqT, ldl, 0.0, nullptr, 0, P, strideAt, (long)m * ldl, 0);
  g.b_tri = 1;  // LqT[j,k] = Lq[k,j] vanishes for k < j
  g.epi = 1; g.sq_cols = m; g.c2_cols = 0;
  g.part = (double*)ws; g.part_ld = rows; g.stridePart = (long)nt * rows;
  g.C2 = (double*)ws; g.ldc2 = 0; g.strideC2 = 0;
  if (V) {
    g.stat_sumsq = s0; g.stat_mv = fmean; g.stat_V = V; g.stat_P = P;
    if (!gpk_gemm_fuses_row_stats(g)) {
      g.stat_sumsq = g.stat_mv = nullptr; g.stat_V = nullptr; g.stat_P = 0;
      const int rc = gpk_row_stats((void*)s, At, rows, m, ldat, V, nullptr, P, 1.0, 0.0, s0, fmean, nullptr);
      if (rc) return rc;
    }
  }
  return gpk_launch_gemm(s, g);
}
}  // namespace

extern "C" int gpk_project_stats(void* stream, const double* At, int rows, int m, long ldat, const double* LqT, long ldl, int P,
                                 const double* V, double* s0, double* fmean, double* ssq, void* ws, size_t ws_bytes) {
  if (!V || (rows > 0 && !ssq)) return GPK_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int rc = project_parts(s, At, rows, m, ldat, 0, LqT, ldl, P, ws, ws_bytes, V, s0, fmean);
  if (rc || rows == 0) return rc;
  const int nt = 2 * gpk_gemm_tiles_n(m);
  return gpk_launch_sum_parts(s, (const double*)ws, nt, rows, (long)nt * rows, P, ssq);
}

extern "C" int gpk_project_batched(void* stream, const double* At, int rows, int m, long ldat, long strideAt,
                                   const double* LqT, long ldl, int P, double* ssq, void* ws, size_t ws_bytes) {
  if (!ssq && rows > 0) return GPK_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int rc = project_parts(s, At, rows, m, ldat, strideAt, LqT, ldl, P, ws, ws_bytes);
  if (rc || rows == 0) return rc;
  const int nt = 2 * gpk_gemm_tiles_n(m);
  return gpk_launch_sum_parts(s, (const double*)ws, nt, rows, (long)nt * rows, P, ssq);
}

extern "C" int gpk_project(void* stream, const double* At, int rows, int m, long ldat,
                           const double* LqT, long ldl, int P, double* ssq, void* ws,
                           size_t ws_bytes) {
  return gpk_project_batched(stream, At, rows, m, ldat, 0, LqT, ldl, P, ssq, ws, ws_bytes);
}

namespace {
// Carves a caller's workspace: every piece starts on a 256-byte boundary.  Over a null workspace it only counts, which is how
// each layout below serves its *_workspace_bytes entry point and its driver alike.
struct Carver {
  uintptr_t base;
  size_t used = 0;
  double* take(size_t bytes) {
    double* p = (double*)(base + used);
    used += gpk_align_up(bytes, 256);
    return p;
  }
};
}  // namespace

// ---- fused driver: GPR.log_marginal_likelihood ----------------------------------------------------------
namespace {
struct LmlWs {
  long ld;
  double *T, *invd, *part, *logdet;
  size_t total;
};
LmlWs lml_layout(void* ws, int n, int P) {
  LmlWs w{};
  Carver c{(uintptr_t)ws};
  w.ld = (long)gpk_align_up((size_t)n, 8);
  w.T = c.take((size_t)(n + P) * w.ld * sizeof(double));
  w.invd = c.take(gpk_invd_elems(n, 1) * sizeof(double));
  w.part = c.take((size_t)GPK_REDUCE_MAXPART * sizeof(double));
  w.logdet = c.take(256);
  w.total = c.used;
  return w;
}
}  // namespace

extern "C" size_t gpk_gpr_lml_workspace_bytes(int n, int d, int P) {
  (void)d;
  return lml_layout(nullptr, n, P).total;
}

extern "C" int gpk_gpr_lml(void* stream, int family, const double* X, int n, int d, long ldx,
                           const double* Y, int P, long ldy, const double* ls_host, int ard,
                           double variance, double noise_variance, const double* noise_rows, double mean_const,
                           double* out, int* info, void* ws, size_t ws_bytes) {
  if (!X || !Y || !out || !info || n <= 0 || P <= 0) return GPK_E_ARG;
  const LmlWs w = lml_layout(ws, n, P);
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, w.total));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  // K(X,X) + noise I, lower tiles only (gpr.py:100-101); a heteroskedastic likelihood (noise_rows: one variance per data
  // row, likelihoods/scalar_continuous.py:92-111) adds its vector to the diagonal instead (model_utils.py:46-50).
  rc = gpk_kernel_matrix(stream, family, X, n, ldx, nullptr, 0, 0, d, ls_host, ard, variance,
                         noise_rows ? 0.0 : noise_variance, 1, w.T, w.ld);
  if (rc) return rc;
  if (noise_rows) {
    rc = gpk_diag_add(stream, w.T, n, w.ld, noise_rows);
    if (rc) return rc;
  }
  // (Y - m)^T as P extra rows (gpr.py:103, logdensities.py:149)
  double* alphaT = w.T + (long)n * w.ld;
  rc = gpk_launch_transpose_shift(s, Y, n, P, ldy, alphaT, w.ld, -mean_const);
  if (rc) return rc;
  // L = chol(K); extra rows -> alpha^T = (L^-1 (Y-m))^T  (gpr.py:102, logdensities.py:150)
  rc = gpk_potrf_core(s, w.T, n, P, w.ld, 1, 0, w.invd, 0, info);
  if (rc) return rc;
  // p = -0.5 sum alpha^2 - 0.5 N log 2pi - sum log diag L, summed over the P columns
  rc = gpk_sum_log_diag(stream, w.T, n, w.ld, 1, 0, w.logdet);
  if (rc) return rc;
  int cnt = 0;
  rc = gpk_launch_sumsq_stage1(s, alphaT, P, n, w.ld, 0, w.part, &cnt);
  if (rc) return rc;
  const double* parts[2] = {w.part, w.logdet};
  const int counts[2] = {cnt, 1};
  const double scales[2] = {-0.5, -(double)P};
  const double add = -0.5 * (double)n * (double)P * 1.8378770664093453;
  return gpk_launch_final(s, 2, parts, counts, scales, add, out);
}

// ---- fused drivers: one shard of SVGP.elbo -- what the forms share ----------------------------------------
namespace {
struct KernelDesc {
  int family, d;
  const double* ls_host;
  int ard;
  double variance;
};
// the arguments of a shard, as the extern "C" entry points receive them (separate kernels: `k` is filled per latent)
struct ElboArgs {
  KernelDesc k;
  const double* Z; int m; long ldz;
  const double *Xb, *Yb; int rows; long ldxb, ldyb;
  int P;
  const double *q_mu, *q_sqrt; int q_diag;
  double noise_variance; const double* noise_rows;
  double jitter, mean_const;
  double* out; int* info;
  int lik = 0;                         // 0: Gaussian (noise_variance, noise_rows); else a GPK_LIK_* code with lik_params (host)
  const double* lik_params = nullptr;
};
// the workspace of a shard.  T is the trapezoid [Kuu + jitter I ; Kfu ; ...] (separate kernels: P of them, strideT apart)
struct ElboWs {
  long ld, strideT;
  double* T;
  double* Kfu;    // extra rows of the trapezoid: Kfu in, A^T = Kfu Lm^-T out (in place)
  double* arow;   // un-whitened: [P, m] rows behind Kfu, q_mu^T in, a^T = (Lm^-1 q_mu)^T out
  double* LqT;    // whitened: tril(q_sqrt_p)^T [P][m][ld] for the projection; un-whitened: the LAST rows of the trapezoid,
                  // behind arow -- tril(q_sqrt_p)^T in, G_p^T out (full q_sqrt), or I in, Lm^-T out [m, ld] (diagonal q_sqrt)
  double *invd, *s0, *fmean, *ssq;
  double* proj;   // projection partials (full q_sqrt), or -- un-whitened with a diagonal q_sqrt -- the second solve A^T Lm^-1 [rows, ld]
  double *part0, *part1;
  double* part2;  // [GPK_REDUCE_MAXPART] partials, then up to P + 1 single terms of the un-whitened KL
  double* V;      // [m, P]
  size_t total;
};

ElboWs elbo_layout(void* ws, int m, int rows, int P, int q_diag, int whiten) {
  ElboWs w{};
  Carver c{(uintptr_t)ws};
  w.ld = (long)gpk_align_up((size_t)m, 8);
  // (minibatch rows padded to whole 32-row blocks -- the single-launch step kernel's layout, DESIGN 6 "Closed experiments whose code
  // was removed"; kept so that the workspace size does not change: the padding rows are never initialised and never read)
  const size_t rows_pad = gpk_align_up((size_t)rows, 32);
  // T [m + rows_pad rows], then -- directly behind it, NOT rounded to 256 bytes, so that the un-whitened form can use ONE trapezoid
  // [Kuu ; Kfu ; q_mu^T ; tril(q_sqrt_p)^T] with the minibatch rows unpadded -- room for P + P m more rows; the whitened form keeps
  // its LqT there, behind the P rows the un-whitened form has
  // (un-whitened with a diagonal q_sqrt: the trapezoid is [Kuu ; Kfu ; q_mu^T ; I] -- P + m more rows)
  const size_t tail_rows = q_diag ? (whiten ? 0 : (size_t)P + m + 32) : (size_t)P + (size_t)P * m + 32;
  w.T = c.take((m + rows_pad + tail_rows) * w.ld * sizeof(double));
  w.Kfu = w.T + (long)m * w.ld;
  w.arow = w.T + (long)(m + (whiten ? rows_pad : (size_t)rows)) * w.ld;
  w.LqT = w.arow + (long)P * w.ld;   // (whitened with a diagonal q_sqrt: no such rows, and nobody uses them)
  w.invd = c.take(gpk_invd_elems(m, 1) * sizeof(double));
  w.s0 = c.take((size_t)rows * sizeof(double));
  w.fmean = c.take((size_t)rows * P * sizeof(double));
  w.ssq = c.take((size_t)rows * P * sizeof(double));
  w.proj = c.take(q_diag ? (whiten ? 0 : (size_t)rows * w.ld * sizeof(double)) : gpk_project_workspace_bytes(rows, m, P));
  w.part0 = c.take((size_t)GPK_REDUCE_MAXPART * sizeof(double));
  w.part1 = c.take((size_t)GPK_REDUCE_MAXPART * sizeof(double));
  w.part2 = c.take((size_t)(GPK_REDUCE_MAXPART + 64) * sizeof(double));
  w.V = c.take((size_t)m * P * sizeof(double));
  w.total = c.used;
  return w;
}

ElboWs elbo_sep_layout(void* ws, int m, int rows, int P) {
  ElboWs w{};
  Carver c{(uintptr_t)ws};
  w.ld = (long)gpk_align_up((size_t)m, 8);
  w.strideT = (long)(m + rows) * w.ld;
  w.T = c.take((size_t)P * w.strideT * sizeof(double));
  w.Kfu = w.T + (long)m * w.ld;
  w.invd = c.take(gpk_invd_elems(m, P) * sizeof(double));
  w.LqT = c.take((size_t)P * m * w.ld * sizeof(double));
  w.s0 = c.take((size_t)rows * P * sizeof(double));
  w.fmean = c.take((size_t)rows * P * sizeof(double));
  w.ssq = c.take((size_t)rows * P * sizeof(double));
  w.proj = c.take(gpk_project_workspace_bytes(rows, m, P));
  w.part0 = c.take((size_t)GPK_REDUCE_MAXPART * sizeof(double));
  w.part1 = c.take((size_t)GPK_REDUCE_MAXPART * sizeof(double));
  w.total = c.used;
  return w;
}

// Work that depends on neither factorisation nor minibatch solve -- tril(q_sqrt)^T for the projection and the whole KL term of the
// whitened forms -- goes to the factorisation's rest-update stream as its late_work when the factorisation runs on streams of
// its own and has minibatch rows to solve beside the chain; otherwise the driver issues it on the caller's stream.
bool side_schedule(int m, int rows) { return m > GPK_NB && m < 4096 && rows > 256; }

// Kuu + jitter I (posteriors.py:835, covariances/kuus.py:29-34), lower tiles only: the chain's first leaf waits for
// nothing else, so the factorisation enqueues it on its panel stream, directly in front of that leaf
int build_kuu(hipStream_t ps, const KernelDesc& k, const ElboArgs& a, const double* Z, double* T, long ld) {
  return gpk_kernel_matrix((void*)ps, k.family, Z, a.m, a.ldz, nullptr, 0, 0, k.d, k.ls_host, k.ard, k.variance, a.jitter, 1, T, ld);
}
// Kuf^T = k(Xb, Z) as the extra rows (posteriors.py:836, covariances/kufs.py:31-34).  Only the bulk stream of the
// factorisation consumes it, so it is built THERE (ordered after everything already queued on the caller's stream)
// and the panel chain starts right after the much smaller Kuu build.
int build_kfu(hipStream_t xs, const KernelDesc& k, const ElboArgs& a, const double* Z, double* Kfu, long ld) {
  return gpk_kernel_matrix((void*)xs, k.family, a.Xb, a.rows, a.ldxb, Z, a.m, a.ldz, k.d, k.ls_host, k.ard, k.variance, 0.0, 0, Kfu, ld);
}
typedef decltype(&build_kuu) BuildFn;   // (build_kuu and build_kfu: one signature, so that the separate form can loop around either)
// un-whitened forms: Kfu and q_mu^T, the first extra rows of their one trapezoid
int build_kfu_and_q_mu_rows(hipStream_t xs, const ElboArgs& a, const ElboWs& w) {
  const int r = build_kfu(xs, a.k, a, a.Z, w.Kfu, w.ld);
  if (r) return r;
  return gpk_transpose((void*)xs, a.q_mu, a.m, a.P, a.P, w.arow, w.ld, 0, 1, 0, 0);
}
// tril(q_sqrt_p)^T, P blocks [m, ld]
int transpose_q_sqrt(hipStream_t s, const ElboArgs& a, const ElboWs& w) {
  return gpk_transpose((void*)s, a.q_sqrt, a.m, a.m, a.m, w.LqT, w.ld, 1, a.P, (long)a.m * a.m, (long)a.m * w.ld);
}

// sum_b var_exp_b -> out[0]  (likelihoods/scalar_continuous.py:139-148, svgp.py:174,181); knn_host: the kernel variance(s).
// The only stage of a shard that knows the likelihood: Gaussian in closed form, the others by Gauss-Hermite quadrature.
// slot != null (Gaussian, shared kernel): ssq is still nt slot partials [P][nt][rows] and `ticket` a zeroed word -- one launch
// sums the slots, forms the expectations and reduces them (gpk_launch_varexp_tail)
int varexp_to_out(hipStream_t s, const ElboArgs& a, const ElboWs& w, const double* knn_host, int per_latent,
                  const double* slot = nullptr, int nt = 0, int* ticket = nullptr) {
  const LatentMoments mo = gpk_latent_moments(a.Yb, a.ldyb, w.fmean, a.rows, a.P, w.s0, per_latent, w.ssq, knn_host, per_latent,
                                              a.mean_const, nullptr);
  if (slot && !a.lik)
    return gpk_launch_varexp_tail(s, mo, slot, nt, (long)nt * a.rows, a.noise_variance, a.noise_rows, w.part0, ticket, a.out);
  if (slot) GPK_TRY(gpk_launch_sum_parts(s, slot, nt, a.rows, (long)nt * a.rows, a.P, w.ssq));   // the quadrature likelihoods keep their launches
  int count = 0;
  GPK_TRY(a.lik ? gpk_launch_likelihood_varexp_stage1(s, a.lik, a.lik_params, mo, nullptr, nullptr, nullptr, w.part0, nullptr, &count)
                : gpk_launch_varexp_stage1(s, mo, a.noise_variance, a.noise_rows, w.part0, &count));
  return gpk_launch_final_one(s, w.part0, count, 1.0, 0.0, a.out);
}
// KL[q || N(0, I)] -> out[1]  (kullback_leiblers.py:45-46, 98-165)
// Its first kernel also zeroes the ticket of the shard's one-launch tail (tail_ticket): every whitened shard runs it before that
// tail, on the caller's stream or on a stream the factorisation joins before it returns.
int* tail_ticket(const ElboWs& w) { return (int*)(w.part2 + GPK_REDUCE_MAXPART + 32); }   // (part2: not otherwise used by the whitened form)
int kl_white_to_out(hipStream_t s, const ElboArgs& a, const ElboWs& w) {
  int count = 0;
  const int rc = gpk_launch_kl_white_stage1(s, a.q_mu, a.q_sqrt, a.m, a.P, a.q_diag, w.part1, &count, w.part2 ? tail_ticket(w) : nullptr);
  if (rc) return rc;
  return gpk_launch_final_one(s, w.part1, count, 0.5, -0.5 * (double)a.m * (double)a.P, a.out + 1);
}
// the late_work of the whitened forms (side_schedule), on whichever stream issues it
int transpose_q_sqrt_and_kl(hipStream_t s, const ElboArgs& a, const ElboWs& w) {
  if (!a.q_diag) {
    const int r = transpose_q_sqrt(s, a, w);
    if (r) return r;
  }
  return kl_white_to_out(s, a, w);
}

// ---- whitened; shared kernel over the P latents ----
int elbo_whitened(hipStream_t s, const ElboArgs& a, const ElboWs& w) {
  const bool side = side_schedule(a.m, a.rows);
  PotrfHooks hk;
  hk.p_prologue = [&a, &w](hipStream_t ps) { return build_kuu(ps, a.k, a, a.Z, w.T, w.ld); };
  hk.x_prologue = [&a, &w](hipStream_t xs) { return build_kfu(xs, a.k, a, a.Z, w.Kfu, w.ld); };
  if (side) hk.late_work = [&a, &w](hipStream_t bs) { return transpose_q_sqrt_and_kl(bs, a, w); };
  // Lm = chol(Kuu);  A^T = Kfu Lm^-T   (conditionals/util.py:67,125)
  int rc = gpk_potrf_core(s, w.T, a.m, a.rows, w.ld, 1, 0, w.invd, 0, a.info, hk);
  if (rc) return rc;
  if (!side) {   // (in front of the tail, whose ticket it zeroes)
    rc = transpose_q_sqrt_and_kl(s, a, w);
    if (rc) return rc;
  }
  // s0 = sum_k A^2 (util.py:133), fmean = A^T q_mu (util.py:144), q_diag: ssq = sum (A q_sqrt)^2 (:149)
  if (a.q_diag) {
    rc = gpk_row_stats((void*)s, w.Kfu, a.rows, a.m, w.ld, a.q_mu, a.q_sqrt, a.P, 1.0, 0.0, w.s0, w.fmean, w.ssq);
    if (rc) return rc;
    return a.lik ? varexp_to_out(s, a, w, &a.k.variance, 0) : varexp_to_out(s, a, w, &a.k.variance, 0, w.ssq, 1, tail_ticket(w));
  }
  // L = band_part(q_sqrt,-1,0); LTA = L^T A; ssq = sum LTA^2   (util.py:151-164), s0 and fmean out of the same GEMM
  rc = project_parts(s, w.Kfu, a.rows, a.m, w.ld, 0, w.LqT, w.ld, a.P, w.proj, gpk_project_workspace_bytes(a.rows, a.m, a.P), a.q_mu,
                     w.s0, w.fmean);
  if (rc) return rc;
  return varexp_to_out(s, a, w, &a.k.variance, 0, w.proj, 2 * gpk_gemm_tiles_n(a.m), tail_ticket(w));
}

// ---- whiten = 0 (kullback_leiblers.py:98-165 with K = Kuu, conditionals/util.py:128-167 with white = False) on ONE
// trapezoid [Kuu + jitter I ; Kfu ; q_mu^T ; tril(q_sqrt_p)^T].  The reference factors Kuu twice (once for the KL, once for
// the conditional) and solves the minibatch columns twice (Lm^-1, then Lm^-T).  Here the extra rows come back as
//     A^T = Kfu Lm^-T,   a^T = (Lm^-1 q_mu)^T,   G_p^T = (Lm^-1 Lq_p)^T   (G_p lower triangular again)
// which are the Mahalanobis / trace terms of the KL AND the whitened parameters of the same q(u): fmean = A^T a,
// sum_j (Lq^T Lm^-T A)_j^2 = sum_j (G^T A)_j^2 -- the projection kernel of the whitened path with G^T in place of Lq^T,
// no second triangular solve of the minibatch rows.
int elbo_unwhitened_full(hipStream_t s, const ElboArgs& a, const ElboWs& w) {
  const int m = a.m, P = a.P;
  PotrfHooks hk;
  hk.p_prologue = [&a, &w](hipStream_t ps) { return build_kuu(ps, a.k, a, a.Z, w.T, w.ld); };
  hk.x_prologue = [&a, &w](hipStream_t xs) {
    const int r = build_kfu_and_q_mu_rows(xs, a, w);
    return r ? r : transpose_q_sqrt(xs, a, w);
  };
  // (P = 1: the m rows of tril(q_sqrt)^T are the LAST rows of the trapezoid and upper triangular -- row j stays zero left of
  //  column j until its column group is reached, so the row solve skips them there: 3/8 of their work, round 5)
  int rc = gpk_potrf_core(s, w.T, m, a.rows + P + P * m, w.ld, 1, 0, w.invd, 0, a.info, hk, P == 1 ? m : 0, true);
  if (rc) return rc;
  rc = gpk_transpose((void*)s, w.arow, P, m, w.ld, w.V, P, 0, 1, 0, 0);           // a = Lm^-1 q_mu as [m, P]
  if (rc) return rc;
  // (s0 and fmean = A^T a out of the projection GEMM, as in the whitened form; the tail keeps its three launches -- this form has
  //  no earlier kernel that zeroes a ticket, and part2 is in use)
  rc = project_parts(s, w.Kfu, a.rows, m, w.ld, 0, w.LqT, w.ld, P, w.proj, gpk_project_workspace_bytes(a.rows, m, P), w.V, w.s0, w.fmean);
  if (rc) return rc;
  rc = gpk_launch_sum_parts(s, w.proj, 2 * gpk_gemm_tiles_n(m), a.rows, (long)2 * gpk_gemm_tiles_n(m) * a.rows, P, w.ssq);
  if (rc) return rc;
  rc = varexp_to_out(s, a, w, &a.k.variance, 0);
  if (rc) return rc;
  // KL = 0.5 |a|^2 + 0.5 sum_p |G_p|_F^2 - 0.5 M P - 0.5 sum log diag(Lq)^2 + P sum log diag(Lm)
  int cm = 0, ct = 0;
  rc = gpk_launch_sumsq_stage1(s, w.arow, P, m, w.ld, 0, w.part1, &cm);
  if (rc) return rc;
  rc = gpk_launch_sumsq_stage1(s, w.LqT, P * m, m, w.ld, 0, w.part2, &ct);
  if (rc) return rc;
  double* ldq = w.part2 + GPK_REDUCE_MAXPART;   // [P] log det q, then [1] log det Lm
  double* ldl = ldq + P;
  rc = gpk_launch_sum_log_diag_sq(s, a.q_sqrt, m, m, P, (long)m * m, ldq);
  if (rc) return rc;
  rc = gpk_sum_log_diag((void*)s, w.T, m, w.ld, 1, 0, ldl);
  if (rc) return rc;
  const double* kp[4] = {w.part1, w.part2, ldq, ldl};
  const int kc[4] = {cm, ct, P, 1};
  const double ks[4] = {0.5, 0.5, -0.5, (double)P};
  return gpk_launch_final(s, 4, kp, kc, ks, -0.5 * (double)m * (double)P, a.out + 1);
}

// ---- whiten = 0 with a DIAGONAL q_sqrt [m, P] (kullback_leiblers.py:128-165: diag branch with K; conditionals/util.py:139-149)
// on ONE trapezoid [Kuu + jitter I ; Kfu ; q_mu^T ; I]: the identity rows come back as Lm^-T (written and solved by the
// factorisation at m^3 / 3, gpk_potrf_inv's row skipping), which gives everything the reference takes from its two
// factorisations and three triangular solves:
//     A^T = Kfu Lm^-T (fvar's Knn - sum A^2),  a^T = (Lm^-1 q_mu)^T (Mahalanobis term),  (Kuu^-1)_ii = |row i of Lm^-T|^2 (trace term),
//     A2^T = A^T Lm^-1 as one triangular-K GEMM (util.py:139's second solve of the minibatch columns) -> fmean = A2^T q_mu,
//     ssq = sum_i (A2_ib q_sqrt_ip)^2 (util.py:149).
int elbo_unwhitened_diag(hipStream_t s, const ElboArgs& a, const ElboWs& w) {
  const int m = a.m, P = a.P, rows = a.rows;
  double* A2 = w.proj;   // [rows, ld]
  PotrfHooks hk;
  hk.p_prologue = [&a, &w](hipStream_t ps) { return build_kuu(ps, a.k, a, a.Z, w.T, w.ld); };
  hk.x_prologue = [&a, &w](hipStream_t xs) { return build_kfu_and_q_mu_rows(xs, a, w); };
  int rc = gpk_potrf_core(s, w.T, m, rows + P + m, w.ld, 1, 0, w.invd, 0, a.info, hk, m);
  if (rc) return rc;
  if (rows > 0) {
    GemmArgs g = gemm_base(rows, m, m, 1.0, w.Kfu, w.ld, w.LqT, w.ld, 0.0, A2, w.ld, 1, 0, 0, 0);
    g.b_tri = 1;  // LqT[j, k] = Lm^-1[k, j] vanishes for k < j
    rc = gpk_launch_gemm(s, g);
    if (rc) return rc;
    rc = gpk_row_sumsq((void*)s, w.Kfu, rows, m, w.ld, 1.0, 0.0, w.s0);
    if (rc) return rc;
    rc = gpk_row_stats((void*)s, A2, rows, m, w.ld, a.q_mu, a.q_sqrt, P, 1.0, 0.0, nullptr, w.fmean, w.ssq);
    if (rc) return rc;
  }
  rc = varexp_to_out(s, a, w, &a.k.variance, 0);
  if (rc) return rc;
  // KL = 0.5 ( |a|^2 + sum_i [(Kuu^-1)_ii sum_p w_ip^2 - sum_p log w_ip^2] - M P ) + P sum log diag(Lm)
  int cm = 0, ct = 0;
  rc = gpk_launch_sumsq_stage1(s, w.arow, P, m, w.ld, 0, w.part1, &cm);
  if (rc) return rc;
  rc = gpk_launch_kl_unwhite_diag_stage1(s, w.LqT, w.ld, m, a.q_sqrt, P, w.part2, &ct);   // trace / log det q partials
  if (rc) return rc;
  double* ldl = w.part2 + GPK_REDUCE_MAXPART;   // [1] log det Lm
  rc = gpk_sum_log_diag((void*)s, w.T, m, w.ld, 1, 0, ldl);
  if (rc) return rc;
  const double* kp[3] = {w.part1, w.part2, ldl};
  const int kc[3] = {cm, ct, 1};
  const double ks[3] = {0.5, 0.5, (double)P};
  return gpk_launch_final(s, 3, kp, kc, ks, -0.5 * (double)m * (double)P, a.out + 1);
}
}  // namespace

extern "C" size_t gpk_svgp_elbo_workspace_bytes(int m, int rows, int d, int P, int q_diag, int whiten) {
  (void)d;
  return elbo_layout(nullptr, m, rows, P, q_diag, whiten).total;
}

namespace {
// the shard behind both entry points: argument checks, workspace, then the form (whiten, q_diag) picks its schedule
int elbo_shard(void* stream, const ElboArgs& a, int whiten, void* ws, size_t ws_bytes) {
  if (!a.Z || (a.rows > 0 && (!a.Xb || !a.Yb)) || !a.q_mu || !a.q_sqrt || !a.out || !a.info || a.m <= 0 || a.rows < 0 || a.P <= 0 ||
      a.P > 16)
    return GPK_E_ARG;
  if (a.lik) {
    const int rc = gpk_likelihood_check(a.lik, a.lik_params, a.P);
    if (rc) return rc;
  }
  const ElboWs w = elbo_layout(ws, a.m, a.rows, a.P, a.q_diag, whiten);
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, w.total));
  hipStream_t s = (hipStream_t)stream;
  if (whiten) return elbo_whitened(s, a, w);
  return a.q_diag ? elbo_unwhitened_diag(s, a, w) : elbo_unwhitened_full(s, a, w);
}
}  // namespace

extern "C" int gpk_svgp_elbo_shard(void* stream, int family, const double* Z, int m, long ldz,
                                   const double* Xb, const double* Yb, int rows, long ldxb,
                                   long ldyb, int d, int P, const double* ls_host, int ard,
                                   double variance, double noise_variance, const double* noise_rows, double jitter,
                                   double mean_const, const double* q_mu, const double* q_sqrt,
                                   int q_diag, int whiten, double* out, int* info, void* ws,
                                   size_t ws_bytes) {
  const ElboArgs a{{family, d, ls_host, ard, variance}, Z, m, ldz, Xb, Yb, rows, ldxb, ldyb, P, q_mu, q_sqrt, q_diag,
                   noise_variance, noise_rows, jitter, mean_const, out, info};
  return elbo_shard(stream, a, whiten, ws, ws_bytes);
}

extern "C" int gpk_svgp_elbo_shard_lik(void* stream, int family, const double* Z, int m, long ldz, const double* Xb,
                                       const double* Yb, int rows, long ldxb, long ldyb, int d, int P, const double* ls_host,
                                       int ard, double variance, int lik, const double* lik_params_host, double jitter,
                                       double mean_const, const double* q_mu, const double* q_sqrt, int q_diag, int whiten,
                                       double* out, int* info, void* ws, size_t ws_bytes) {
  if (!lik) return GPK_E_UNSUPPORTED;   // (0 is the Gaussian stage of gpk_svgp_elbo_shard, not a likelihood code)
  ElboArgs a{{family, d, ls_host, ard, variance}, Z, m, ldz, Xb, Yb, rows, ldxb, ldyb, P, q_mu, q_sqrt, q_diag,
             0.0, nullptr, jitter, mean_const, out, info};
  a.lik = lik; a.lik_params = lik_params_host;
  return elbo_shard(stream, a, whiten, ws, ws_bytes);
}

// ---- fused driver: one shard of SVGP.elbo with SEPARATE kernels per latent (SeparateIndependent, whitened, full q_sqrt) --------
extern "C" size_t gpk_svgp_elbo_sep_workspace_bytes(int m, int rows, int d, int P) {
  (void)d;
  return elbo_sep_layout(nullptr, m, rows, P).total;
}

// The P problems of conditionals/util.py:566-629 (tf.map_fn over the latents) share nothing but the minibatch: P covariance
// pairs built straight into ONE batched trapezoid [P][(m + rows) x ld], one batched factorisation with the minibatch rows riding
// along (gpk_potrf, batch = P), one batched row-statistics launch, one batched projection, one reduction.  Composed from the
// Python mirror the same step issues ~50 launches with host gaps between them (profiles/r04_c5sep_timeline_composed.txt).
// (Measured and not kept: the extra rows solved out of place against EXPLICIT 512-column group inverses -- nine short launches
// for the inverses + one triangular-K GEMM per group instead of the fused in-group kernel: 2.15 / 2.16 against 2.14 ms.)
// The body behind gpk_svgp_elbo_shard_sep and gpk_svgp_elbo_shard_lcm: a.P latents; `tail` is the one stage that differs -- what
// turns the latent moments (w.fmean [rows, P], w.s0 / w.ssq [P, rows], the kernel variances) into out[0].
namespace {
typedef int (*SepTailFn)(hipStream_t, const ElboArgs&, const ElboWs&, const double* variance_host, const void* ctx);
int elbo_shard_separate(void* stream, const ElboArgs& a, const int* family_host, long strideZ, const double* variance_host,
                        SepTailFn tail, const void* ctx, void* ws, size_t ws_bytes) {
  const int m = a.m, rows = a.rows, P = a.P, d = a.k.d;
  if (!family_host || !a.Z || (rows > 0 && (!a.Xb || !a.Yb)) || !a.q_mu || !a.q_sqrt || !a.k.ls_host || !variance_host || !a.out ||
      !a.info || m <= 0 || rows < 0 || P <= 0 || P > 16 || d <= 0 || strideZ < 0)
    return GPK_E_ARG;
  const ElboWs w = elbo_sep_layout(ws, m, rows, P);
  GPK_TRY(gpk_check_workspace(ws, ws_bytes, w.total));
  hipStream_t s = (hipStream_t)stream;
  const int nls = a.k.ard ? d : 1;
  // (ls_host is strided by nls: there is no room for the trailing alpha of a RationalQuadratic member, gpk.h)
  for (int p = 0; p < P; ++p)
    if (family_host[p] == GPK_KERN_RQ) return GPK_E_UNSUPPORTED;
  // latent p: its kernel, its inducing points, its trapezoid
  auto each_latent = [&](BuildFn build, hipStream_t st, double* T0) -> int {
    for (int p = 0; p < P; ++p) {
      const KernelDesc kp{family_host[p], d, a.k.ls_host + (long)p * nls, a.k.ard, variance_host[p]};
      const int r = build(st, kp, a, a.Z + (long)p * strideZ, T0 + (long)p * w.strideT, w.ld);
      if (r) return r;
    }
    return 0;
  };
  const bool side = side_schedule(m, rows);
  PotrfHooks hk;
  // (the chain's first BATCHED leaf waits for the P Kuu builds and nothing else)
  hk.p_prologue = [&](hipStream_t ps) { return each_latent(build_kuu, ps, w.T); };
  hk.x_prologue = [&](hipStream_t xs) { return each_latent(build_kfu, xs, w.Kfu); };
  if (side) hk.late_work = [&a, &w](hipStream_t bs) { return transpose_q_sqrt_and_kl(bs, a, w); };
  int rc = gpk_potrf_core(s, w.T, m, rows, w.ld, P, w.strideT, w.invd, 0, a.info, hk);
  if (rc) return rc;
  if (!side) {
    rc = transpose_q_sqrt_and_kl(s, a, w);
    if (rc) return rc;
  }
  rc = gpk_launch_row_stats_sep(s, w.Kfu, w.strideT, rows, m, w.ld, a.q_mu, P, w.s0, w.fmean);
  if (rc) return rc;
  rc = gpk_project_batched(stream, w.Kfu, rows, m, w.ld, w.strideT, w.LqT, w.ld, P, w.ssq, w.proj,
                           gpk_project_workspace_bytes(rows, m, P));
  if (rc) return rc;
  return tail(s, a, w, variance_host, ctx);
}

int sep_tail_independent(hipStream_t s, const ElboArgs& a, const ElboWs& w, const double* variance_host, const void*) {
  return varexp_to_out(s, a, w, variance_host, 1);
}
// LinearCoregionalization: the P outputs of a row read all L = a.P latents of that row (mix_latent_gp); the mean constant is
// added after the mixing
struct LcmTail { int P; const double* W_host; };
int sep_tail_mixed(hipStream_t s, const ElboArgs& a, const ElboWs& w, const double* variance_host, const void* ctx) {
  const LcmTail& t = *(const LcmTail*)ctx;
  const LatentMoments g = gpk_latent_moments(a.Yb, a.ldyb, w.fmean, a.rows, a.P, w.s0, 1, w.ssq, variance_host, 1, a.mean_const, nullptr);
  int count = 0;
  GPK_TRY(gpk_launch_mixed_varexp_stage1(s, g, t.P, t.W_host, a.noise_variance, nullptr, nullptr, nullptr, w.part0, nullptr, nullptr, &count));
  return gpk_launch_final_one(s, w.part0, count, 1.0, 0.0, a.out);
}
}  // namespace

extern "C" int gpk_svgp_elbo_shard_sep(void* stream, const int* family_host, const double* Z, int m, long ldz, long strideZ,
                                       const double* Xb, const double* Yb, int rows, long ldxb, long ldyb, int d, int P,
                                       const double* ls_host, int ard, const double* variance_host, double noise_variance,
                                       const double* noise_rows, double jitter, double mean_const, const double* q_mu,
                                       const double* q_sqrt, double* out,
                                       int* info, void* ws, size_t ws_bytes) {
  const ElboArgs a{{0, d, ls_host, ard, 0.0}, Z, m, ldz, Xb, Yb, rows, ldxb, ldyb, P, q_mu, q_sqrt, 0,
                   noise_variance, noise_rows, jitter, mean_const, out, info};
  return elbo_shard_separate(stream, a, family_host, strideZ, variance_host, sep_tail_independent, nullptr, ws, ws_bytes);
}

// ---- fused driver: one shard of SVGP.elbo for a LinearCoregionalization kernel (L latents mixed into P outputs) -----------------
extern "C" size_t gpk_svgp_elbo_lcm_workspace_bytes(int m, int rows, int d, int L, int P) {
  (void)d; (void)P;   // (the mixing stage needs one set of partials, which the layout of the L latents already has)
  return elbo_sep_layout(nullptr, m, rows, L).total;
}

extern "C" int gpk_svgp_elbo_shard_lcm(void* stream, const int* family_host, const double* Z, int m, long ldz, long strideZ,
                                       const double* Xb, const double* Yb, int rows, long ldxb, long ldyb, int d, int L, int P,
                                       const double* W_host, const double* ls_host, int ard, const double* variance_host,
                                       double noise_variance, double jitter, double mean_const, const double* q_mu,
                                       const double* q_sqrt, double* out, int* info, void* ws, size_t ws_bytes) {
  if (!W_host || P <= 0 || P > 16 || !(noise_variance > 0.0)) return GPK_E_ARG;
  const ElboArgs a{{0, d, ls_host, ard, 0.0}, Z, m, ldz, Xb, Yb, rows, ldxb, ldyb, L, q_mu, q_sqrt, 0,
                   noise_variance, nullptr, jitter, mean_const, out, info};
  const LcmTail t{P, W_host};
  return elbo_shard_separate(stream, a, family_host, strideZ, variance_host, sep_tail_mixed, &t, ws, ws_bytes);
}
