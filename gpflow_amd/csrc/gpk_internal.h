// Internal declarations shared by the libgpk translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <functional>
#include "../../include/gpk.h"

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

#include <stdio.h>
#include <stdlib.h>
#include "gpk_tune.h"   // GPK_TUNE, GPK_TRACE, kGpkExp

#define GPK_HIP(call)                                                                                   \
  do {                                                                                                  \
    hipError_t e__ = (call);                                                                            \
    if (e__ != hipSuccess) {                                                                            \
      GPK_TRACE("%s:%d: %s -> %d\n", __FILE__, __LINE__, #call, (int)e__);                              \
      return (int)e__;                                                                                  \
    }                                                                                                   \
  } while (0)
// (a library call that returns 0 or an error code)
#define GPK_TRY(call)                 \
  do {                                \
    const int rc__ = (call);          \
    if (rc__) return rc__;            \
  } while (0)
#define GPK_LAUNCH_CHECK()                                                                              \
  do {                                                                                                  \
    hipError_t e__ = hipGetLastError();                                                                 \
    if (e__ != hipSuccess) {                                                                            \
      GPK_TRACE("%s:%d: kernel launch -> %d\n", __FILE__, __LINE__, (int)e__);                          \
      return (int)e__;                                                                                  \
    }                                                                                                   \
  } while (0)

static inline size_t gpk_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int gpk_cdiv(int a, int b) { return (a + b - 1) / b; }
// The workspace contract of include/gpk.h (Conventions, "workspace"), points (c) and (d): what every entry point with a `ws`
// parameter answers before anything is enqueued -- GPK_E_WORKSPACE for a null or short workspace, GPK_E_ARG for a base that is not
// 16-byte aligned (the Carver keeps its pieces 256 bytes apart RELATIVE to the base, and the block inverses, the slot partials and
// the trapezoid's rows are read and written 16 bytes at a time).
static inline int gpk_check_workspace(const void* ws, size_t ws_bytes, size_t needed) {
  if (!ws || ws_bytes < needed) return GPK_E_WORKSPACE;
  return ((uintptr_t)ws & 15) ? GPK_E_ARG : 0;
}

// ---- GEMM (gemm.hip): GemmArgs, gemm_base and the selection as data (GemmPlan, make_gemm_plan) --------
#include "gemm_plan.h"
int gpk_launch_gemm(hipStream_t s, const GemmArgs& a);
bool gpk_gemm_takes_latency_kernel(const GemmArgs& a);   // make_gemm_plan(a) picks the one-shot latency kernel (sig / wait honoured)
bool gpk_gemm_fuses_row_stats(const GemmArgs& a);        // make_gemm_plan(a) picks gemm_nt_fast<1> with the row statistics riding along (stat_* set and not this: GPK_E_UNSUPPORTED)

// fused in-group solve of `rows` right-hand-side rows against nb <= 4 leaf blocks of the factor (group_solve.hip); E / Eo point at
// the group's first column, Lgg at L[c0, c0], X at the group's first block inverse
// (batch > 1: blockIdx.y walks the problems, strides in elements)
int gpk_launch_group_solve(hipStream_t s, const double* E, long lde, double* Eo, long ldeo, int rows, const double* Lgg, long ldl,
                           const double* X, int nb, int batch = 1, long strideE = 0, long strideEo = 0, long strideL = 0,
                           long strideX = 0, int max_wgs = 0, int j0 = 0, int j1 = -1);   // max_wgs > 0: at most that many workgroups, walking the 16-row slivers
bool gpk_group_solve_takes_parts();   // a partial in-group solve (j0 > 0 or j1 < nb) exists: the progressive first group of potrf.hip asks
int gpk_gemm_tiles_n(int n);   // number of column tiles the launcher will use for n columns
int gpk_profile_gemm_is_on();  // per-launch event timing active (bench roofline leg)

// ---- leaf (leaf.hip): NB x NB Cholesky + inverse of the diagonal block --------------------------
// A: pointer to the diagonal block (row-major, lda); nb <= NB valid rows/cols.
int gpk_launch_leaf(hipStream_t s, double* A, long lda, long strideA, int nb, double* invd,
                    long strideInv, int* info, int col0, int batch, int already_factored);

// ---- factorisation (potrf.hip), as the fused drivers (drivers.hip) call it ----------------------
// The trapezoid A is [(n + extra) x n]: the top square is factored, the extra rows come back as  B L^-T.
// p_prologue: work of the CALLER that the first leaf waits for and nothing else does -- the fused drivers' Kuu build.  It is
// enqueued ON the panel stream, so the first leaf follows it back to back (0.3 us) instead of behind an event record on the caller's
// stream and a wait on the panel stream (~15 us per step, round 5).
// x_prologue: work of the CALLER that belongs on the bulk stream before the first extra-row group (the SVGP driver's Kfu
// build, transposes, KL).  It is enqueued after the first panel's chain kernels: every host call issued before the first
// leaf delays the whole step, and nothing on the bulk stream is needed for ~4 panels.
// late_work: work of the CALLER that nothing in the factorisation needs (the whitened driver's tril(q_sqrt)^T and KL term).  It is
// enqueued on the rest-update stream after the sixth panel: the first four panels are HOST-bound -- ~7 enqueue calls of 5 - 8 us
// per panel against ~55 us of kernels -- so every launch issued there delays the chain (round 5: the second leaf started 52 us
// after the first strip had finished), and the rest-update stream has a leaf's time of slack per panel.
// (All three are called while the factorisation is being enqueued, never later; an empty one is skipped.)
typedef std::function<int(hipStream_t)> StreamWork;
struct PotrfHooks {
  StreamWork x_prologue, p_prologue, late_work;
};
// tri = n: the LAST n extra rows are the identity (written by the factorisation) and come back as L^-T.  Row j of that block
// stays zero left of column j, so column group [c0, c1) only has to process its first c1 rows: n^3 / 3 flop instead of n^3.
// tri_prefilled: the caller (or its x_prologue) puts an UPPER-TRIANGULAR block there itself -- tril(q_sqrt)^T of the
// un-whitened ELBO: the same rows-stay-zero argument holds for any block that is zero left of its diagonal.
int gpk_potrf_core(hipStream_t S, double* A, int n, int extra, long lda, int batch, long strideA, double* invd, int zero_upper,
                   int* info, const PotrfHooks& hooks = PotrfHooks(), int tri = 0, bool tri_prefilled = false);

// ---- rbf.hip ---------------------------------------------------------------------------------
// (entry point gpk_kernel_matrix is defined there)

#define GPK_REDUCE_MAXPART 1024   // most stage-1 blocks (partials) of a two-stage reduction

// ---- rowops.hip: layout and row passes ---------------------------------------------------------------
int gpk_launch_zero_upper(hipStream_t s, double* A, int n, long lda, int batch, long strideA);
int gpk_launch_set_identity(hipStream_t s, double* A, int n, long lda, int batch = 1, long strideA = 0);
int gpk_launch_row_stats_sep(hipStream_t s, const double* At, long strideAt, int rows, int m, long ldat, const double* V, int P,
                             double* sumsq, double* mv);
int gpk_launch_transpose_shift(hipStream_t s, const double* in, int rows, int cols, long ldin, double* out, long ldout, double shift);

// ---- sync.hip: stream hand-offs ----------------------------------------------------------------------
int gpk_probe_concurrent_kernels(hipStream_t a, hipStream_t b, int* scratch, int* concurrent);   // init-time probe
int gpk_launch_noop(hipStream_t s);  // empty kernel (stream hand-off probe)
int gpk_launch_wait_flag(hipStream_t s, const int* ptr, int val, int* info);   // one-wave gate: returns when (int)(*ptr - val) >= 0 (bounded)
int gpk_launch_set_flag(hipStream_t s, int* ptr, int val);                     // one-thread store behind everything queued on s

// ---- reduce.hip: two-stage reductions (stage 1 leaves `count` partials in `part`) and sums of split-K partials ----
int gpk_launch_sum_parts(hipStream_t s, const double* part, int nt, int rows, long stridePart, int P, double* ssq);
int gpk_launch_final(hipStream_t s, int nterms, const double* const* part, const int* count, const double* scale, double add, double* out);
int gpk_launch_final_one(hipStream_t s, const double* part, int count, double scale, double add, double* out);   // the one-term form
int gpk_launch_sumsq_stage1(hipStream_t s, const double* A, int rows, int cols, long lda, int upper_only, double* part, int* count);
// zero_word (may be null): an int the kernel sets to 0 -- the ticket of a gpk_launch_varexp_tail that is stream-ordered behind it
int gpk_launch_kl_white_stage1(hipStream_t s, const double* q_mu, const double* q_sqrt, int m, int P, int q_diag, double* part, int* count,
                               int* zero_word = nullptr);
int gpk_launch_kl_unwhite_diag_stage1(hipStream_t s, const double* LinvT, long ldl, int m, const double* W, int P, double* part,
                                      int* count);
int gpk_launch_sum_log_diag_sq(hipStream_t s, const double* L, int n, long ldl, int batch, long strideL, double* out);

// ---- varexp.hip: the variational-expectation stages ---------------------------------------------------
// What every stage reads of element (b, p): label Y[b, p], mean fmean[b, p] + mean_const, variance knn - s0 + ssq (s0 [rows] or
// [P, rows], ssq [P, rows] or null, knn one value or one per latent: copied from knn_host); fvar_out (may be null) receives the variance.
struct LatentMoments {
  const double* Y; long ldy; const double* fmean; int rows, P;
  const double* s0; int s0_per_latent; const double* ssq;
  double knn[16]; int knn_per_latent; double mean_const; double* fvar_out;
};
LatentMoments gpk_latent_moments(const double* Y, long ldy, const double* fmean, int rows, int P, const double* s0, int s0_per_latent,
                                 const double* ssq, const double* knn_host, int knn_per_latent, double mean_const, double* fvar_out);
// Gaussian; noise_rows: per-row noise variances [rows] or nullptr (constant `noise`)
int gpk_launch_varexp_stage1(hipStream_t s, const LatentMoments& m, double noise, const double* noise_rows, double* part, int* count);
// the Gaussian tail of a shard in ONE launch: ssq[p,b] = sum of the nt slot partials slot[p][t][b] in slot order (m.ssq is not read),
// the variational expectations exactly as gpk_launch_varexp_stage1 forms them, one partial per block, and the LAST block to finish
// (ticket counter) sums the partials in index order into out[0].  *ticket must be 0 at entry and is left at the block count.
int gpk_launch_varexp_tail(hipStream_t s, const LatentMoments& m, const double* slot, int nt, long strideSlot, double noise,
                           const double* noise_rows, double* part, int* ticket, double* out);
// the mixed Gaussian stage of gpk_mixed_gaussian_varexp_sum: `g` describes the L = g.P latents (g.fmean = gmean, g.mean_const is
// added AFTER the mixing), W_host [P, L].  part0 receives `count` partials of sum VE; part1 (sum dVE/ds2) and partW (`count`
// partials [P L] of dW, block after block) may be null.  The caller has checked L, P and the noise.
// (weak: tests/potrf_schedule_run.cpp links drivers.hip against its own stubs of the launchers, one per kernel it restates; a
//  launcher without a stub there is only reached by a driver that runner does not call, and must not keep it from linking)
__attribute__((weak)) int gpk_launch_mixed_varexp_stage1(hipStream_t s, const LatentMoments& g, int P, const double* W_host, double noise, double* fmean_out,
                                   double* fvar_out, double* dgmu_out, double* part0, double* part1, double* partW, int* count);
// the quadrature stage of gpk_likelihood_varexp_sum; part1 (partials of sum dVE/dscale) may be null
int gpk_likelihood_check(int lik, const double* params, int P);   // 0, GPK_E_UNSUPPORTED (unknown code) or GPK_E_ARG (parameters, classes)
// the same answer, and the three constants the code's element body reads (lik_element.h: LikConsts), computed once on the host
int gpk_likelihood_constants(int lik, const double* params, int P, double* par0, double* par1, double* c0);
int gpk_launch_likelihood_varexp_stage1(hipStream_t s, int lik, const double* params, const LatentMoments& m, double* rows_out,
                                        double* dmu_out, double* dvar_out, double* part, double* part1, int* count);
