/* gpk.h -- C-ABI of libgpk.so: the MI355X (gfx950) dense-GP hot path behind gpflow_amd.
 *
 * The reference (GPflow 2.9.2) has no C/FFI boundary: every FLOP of this path is a TensorFlow op
 * called from Python.  Each entry point below replaces one TF-op call site (or a fused group of
 * them); the reference file:line it stands in for is cited per function (paths relative to the
 * GPflow tree).  The reference-side binding a maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *   - every matrix pointer is a DEVICE pointer to row-major fp64 (gpflow default_float,
 *     config/__config__.py:99); leading dimensions are in elements;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work,
 *     they never synchronise; scratch comes from the caller's workspace;
 *   - workspace: every entry point with a `void* ws, size_t ws_bytes` pair (gpk_project, _batched, _stats; gpk_gaussian_,
 *     gpk_likelihood_, gpk_mixed_gaussian_varexp_sum; gpk_gauss_kl_white; gpk_sumsq; gpk_gpr_lml; gpk_svgp_elbo_shard, _lik, _sep,
 *     _lcm) takes its scratch from the caller, sized by the *_workspace_bytes function named next to it, under one contract:
 *       (a) contents: what `ws` holds at entry does not matter -- zeros, NaN bytes, or what another call (of another entry point,
 *           shape or form) left there; the result is bit-identical whatever it is.  The library keeps counters and partial sums
 *           in there between the launches of ONE call; each is written by a launch of that call before it is read, never
 *           by a memset packet and never by the caller.  One workspace may therefore be reused across calls of any kind, as
 *           long as two calls that share it are ordered on their streams;
 *       (b) bounds: the call reads and writes only the first *_workspace_bytes(...) bytes of `ws`, whatever ws_bytes says;
 *       (c) refusal: ws == NULL (even where the size is 0) or ws_bytes below that size returns GPK_E_WORKSPACE, and a refused
 *           call enqueues and writes nothing: not `out`, not `info`, not `ws`;
 *       (d) alignment: `ws` must be 16-byte aligned (any device allocator's blocks are; an odd element offset into an fp64 buffer
 *           is not).  The pieces carved from it sit 256 bytes apart relative to the base and are read and written 16 bytes at a
 *           time.  A base that is not 16-byte aligned returns GPK_E_ARG, with the same nothing-written rule.  No larger alignment
 *           is required;
 *   - small hyper-parameter vectors (lengthscales) are HOST pointers, copied into kernel arguments;
 *   - empty operands: a pointer to an operand with no elements (0 rows or 0 columns) may be NULL -- a fresh empty tensor
 *     has no storage -- and the call then writes what the empty case defines: nothing for an empty output, the plain
 *     sum over no terms for a reduction (e.g. gpk_gaussian_varexp_sum with rows = 0 writes 0, gpk_svgp_elbo_shard writes
 *     [0, KL]), and beta C for gpk_gemm_nt with k = 0 (exact zeros for beta = 0; C is not read then);
 *   - return value: 0 ok, <0 bad argument (GPK_E_*), >0 HIP runtime error code (hipError_t);
 *   - numerical failure (non-positive or NaN pivot) is reported LAPACK-style through a device int
 *     `info` (0 = ok, j+1 = first bad pivot column) that the caller reads when it next syncs
 *     (TF raises InvalidArgumentError "Cholesky decomposition was not successful" at the same spot);
 *     INT_MAX = an internal stream hand-off of the factorisation timed out (0.5 s; never observed -- the bounded wait exists so
 *     that a lost hand-off cannot hang the device);
 *
 * Internal state and threading (the complete list; nothing else in the library is mutable)
 *   - gpk_potrf with n > 128 (and the two fused drivers, which call it) uses per-device state created lazily on the
 *     first such call: five internal HIP streams (P panel, high priority / X side / one placeholder that fixes the
 *     stream-to-hardware-queue layout / Bs bulk-small / B bulk, CU-masked) and a pool of timing-disabled events that grows
 *     to 2 * panels + 8, and 4 KB of device memory for hand-off words: single-leaf panels of the latency chain are handed
 *     over between these streams with hipStreamWaitValue32 / hipStreamWriteValue32 and an in-kernel poll instead of event
 *     packets (an event record / wait between two kernels of one stream costs 4.6 / 6.3 us on MI355X; the poll is bounded:
 *     after 0.5 s a waiting kernel proceeds rather than hang the device).  That first call also runs a ~1 ms self-check of the stream layout (a few hundred empty kernels;
 *     the ONLY place the library synchronises) and creates the streams again if a pair of them hands kernels over slowly
 *     (gpk_stream_selfcheck).  Afterwards no device memory is allocated and nothing synchronises: work is forked from and
 *     joined to the caller's stream with events only.  (The streams are created in an order that keeps the panel and bulk
 *     streams on different microengine pipes -- INTEGRATION.md section 4: create this state, i.e. make one such call,
 *     before other libraries of the process create their streams.)
 *   - One recursive mutex per device serialises the ENQUEUE section of these calls, so they may be issued from any
 *     number of host threads and on any caller streams; factorisations of one device share the internal streams and
 *     therefore execute one after the other on the GPU.
 *   - Every other entry point is stateless and reentrant (kernel attributes are set through thread-safe function-local
 *     statics; the GEMM launcher keeps the id of the kernel it picked last in a thread_local for the profiling facility).
 *     The library never reads the environment.
 *   - gpk_profile_gemm_* is a measurement facility for bench.py: process-global, not thread-safe, off by default.
 */
#ifndef GPK_H
#define GPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libgpk.so is built with -fvisibility=hidden: exactly the functions declared in this header are exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define GPK_NB 128 /* Cholesky inner block: diag-block inverses are GPK_NB x GPK_NB */
#define GPK_MAX_D 64 /* max input dimension of the covariance builder */

#define GPK_E_ARG (-1)
#define GPK_E_WORKSPACE (-2)
#define GPK_E_UNSUPPORTED (-3)

/* stationary kernel families (gpflow/kernels/stationaries.py) */
#define GPK_KERN_SE 0       /* SquaredExponential.K_r2 :209-210 */
#define GPK_KERN_MATERN12 1 /* :254-255 */
#define GPK_KERN_MATERN32 2 /* :281-283 */
#define GPK_KERN_MATERN52 3 /* :311-313 */
#define GPK_KERN_EXPONENTIAL 4 /* Exponential.K_r: variance exp(-r / 2), r = sqrt(max(r2, 1e-36)) */
#define GPK_KERN_RQ 5          /* RationalQuadratic.K_r2: variance (1 + r2 / (2 alpha))^-alpha, on r2 (no clamp) */
/* static families (gpflow/kernels/statics.py): no distance, X is never read (a NaN in X does not reach the output) */
#define GPK_KERN_WHITE 6    /* White.K: X2 == NULL: variance on the diagonal, 0 elsewhere;  ANY non-NULL X2: zeros -- decided by the
                             * pointer, never by comparing values */
#define GPK_KERN_CONSTANT 7 /* Constant.K: variance everywhere */
/* K(x, x) = variance for all eight families: the one assumption the fused drivers make about a kernel.
 *
 * GPK_KERN_RQ carries one more hyperparameter and no C signature changes for it: `ls_host` then holds one more TRAILING entry,
 * alpha at index (ard ? d : 1).  Every entry point that forwards one ls_host honours it (gpk_kernel_matrix, _combine, _hadamard,
 * gpk_gpr_lml, gpk_svgp_elbo_shard, _lik); alpha <= 0 or a non-finite alpha is GPK_E_ARG.  It is evaluated as
 * variance * exp(-alpha log1p(r2 / (2 alpha))).  gpk_svgp_elbo_shard_sep and _lcm stride ls_host by (ard ? d : 1) per latent and
 * answer GPK_E_UNSUPPORTED for a GPK_KERN_RQ member; the other families pass through them (ls_host is not read for the static ones
 * beyond being non-NULL; pass 1.0). */

const char* gpk_version(void);

/* ---- covariance builder ---------------------------------------------------------------------
 * K[i,j] = variance * k(r2(X1_i / ls, X2_j / ls)) (+ diag_add if i == j and X2 == NULL)
 * Replaces square_distance (utilities/ops.py:105-122, the expansion formula, kept), Stationary.scale
 * (stationaries.py:77-79), K_r2 (:209-210 ...), add_noise_cov (utilities/model_utils.py:33-38) and
 * the jitter add of Kuu (covariances/kuus.py:33).
 *   X1 [n1,d] ldx1; X2 [n2,d] ldx2 or NULL (symmetric: X2 = X1);  K [n1,n2] ldk
 *   ls: HOST pointer, d entries if ard else 1;  lower_only: with X2 == NULL write only tiles that
 *   touch the lower triangle (what the Cholesky reads). */
int gpk_kernel_matrix(void* stream, int family, const double* X1, int n1, long ldx1,
                      const double* X2, int n2, long ldx2, int d, const double* ls_host, int ard,
                      double variance, double diag_add, int lower_only, double* K, long ldk);

/* A[i,i] += v[i], i < n (v: DEVICE pointer):  add_noise_cov / add_likelihood_noise_cov with a per-row likelihood variance
 * (utilities/model_utils.py:33-38, 46-50) -- the heteroskedastic counterpart of gpk_kernel_matrix's scalar diag_add. */
int gpk_diag_add(void* stream, double* A, int n, long lda, const double* v);

/* out = G .* k(X1, X2) (op 1), G + k(X1, X2) (op 2), G .* (-2 dk/dr2)(X1, X2) (op 3) or G .* (dk/dalpha)(X1, X2) (op 4), k recomputed from the inputs (one read of G, one write; G may
 * alias out).  Replaces the tf.multiply / tf.add_n reductions of Product / Sum kernels (kernels/base.py:216-220,
 * 283-329): the second factor / term is folded into the first matrix in place instead of being materialised.
 * X2 == NULL: K(X1, X1), and diag_add goes onto the diagonal of the COMBINED result (noise / jitter).
 * op 3 is the reverse pass of the Matern family (stationaries.py:254-313: r = sqrt(max(r2, 1e-36)), K_r): with
 * r2 the SCALED squared distance, every lengthscale / input gradient contracts Kbar .* dk/dr2 with d r2 / d theta;
 * -2 dk/dr2 equals k for the SquaredExponential, so the same contraction code serves all four families.  X2 == NULL
 * writes exact zeros on the diagonal (r2_ii = 0 identically: no gradient flows through it).
 * -2 dk/dr2: Exponential variance exp(-r / 2) / (2 r), 0 where r2 <= 1e-36 (the clamp passes no gradient, a NaN r2 stays NaN);
 * RationalQuadratic variance exp(-(alpha + 1) log1p(u)), u = r2 / (2 alpha); White and Constant 0.
 * op 4: GPK_KERN_RQ only (any other family: GPK_E_UNSUPPORTED), dk/dalpha = k (u / (1 + u) - log1p(u)); X2 == NULL writes exact
 * zeros on the diagonal as op 3 does.  White, op 2, X2 given, out == G: nothing to do, returns without a launch. */
int gpk_kernel_matrix_combine(void* stream, int family, int op, const double* X1, int n1, long ldx1,
                              const double* X2, int n2, long ldx2, int d, const double* ls_host, int ard,
                              double variance, double diag_add, const double* G, long ldg, double* out, long ldo);

/* = gpk_kernel_matrix_combine(op 1) with X2 given: the elementwise factor of every kernel-parameter gradient,
 * dF/dtheta = sum_ij Kbar_ij dK_ij/dtheta with dK/dtheta = K .* (...) for the stationary kernels -- the reverse pass
 * of Stationary.K (stationaries.py:103-116, 209-210) that TF autodiff builds for optimizers/scipy.py:322-331
 * (SURVEY 8f row 1). */
int gpk_kernel_matrix_hadamard(void* stream, int family, const double* X1, int n1, long ldx1,
                               const double* X2, int n2, long ldx2, int d, const double* ls_host, int ard,
                               double variance, const double* G, long ldg, double* out, long ldo);

/* ---- trapezoidal Cholesky ---------------------------------------------------------------------
 * A is [(n + extra) x n] row-major.  Top n x n block (lower triangle read): K -> L in place,
 * K = L L^T (tf.linalg.cholesky call sites: gpr.py:102, posteriors.py:422,703, conditionals/util.py:67,
 * kullback_leiblers.py:107).  The `extra` rows below it hold right-hand sides B [extra, n] and come
 * back as B L^-T, i.e. (L^-1 B^T)^T -- tf.linalg.triangular_solve(L, B^T, lower=True)
 * (conditionals/util.py:125, logdensities.py:150, kullback_leiblers.py:114,152) fused into the
 * factorisation's panel updates.  The strict upper triangle of the top block is left untouched
 * unless zero_upper != 0.  `batch` matrices at stride strideA (SeparateIndependent: the
 * tf.map_fn loop of conditionals/util.py:618 becomes one batched launch sequence).
 * invd: [batch, ceil(n/NB), NB, NB] output, the inverses of L's diagonal blocks (reused by gpk_trsm);
 * gpk_invd_elems() gives its size in doubles.  invd must be 16-byte aligned (a buffer of gpk_invd_elems() doubles from any
 * allocator is): the inverses are stored and staged 16 bytes at a time whatever the alignment of A.  gpk_potrf, gpk_potrf_inv,
 * gpk_trtri_blocks, gpk_trsm and gpk_transpose_factor (invd and invdT) return GPK_E_ARG for one that is not, before anything
 * is launched.  A itself may have any 8-byte alignment, leading dimension and batch stride.
 * info: device int[batch] (may be NULL). */
size_t gpk_invd_elems(int n, int batch);
int gpk_potrf(void* stream, double* A, int n, int extra, long lda, int batch, long strideA,
              double* invd, int zero_upper, int* info);

/* Result of the init-time stream-layout self-check (see "Internal state and threading"): microseconds per cross-stream
 * kernel hand-off between the library's panel / side / bulk-small streams, as measured now (us_now[3]) and on the first
 * stream set (us_first[3]); *recreated = 1 if the first set was slow (> 30 us: two active hardware queues on one
 * microengine pipe) and the streams were created again.  GPK_E_UNSUPPORTED before the first factorisation with n > 128. */
int gpk_stream_selfcheck(double* us_now, double* us_first, int* recreated);
/* How the factorisation's latency chain hands over between the internal streams on the current device:
 *    2 = flag words in device memory, written and awaited by KERNELS only -- the entry signal of a GEMM kernel, a one-thread store
 *        kernel, a one-wave gate kernel, the bounded in-kernel poll of the strip -- with no queue packet between the chain's
 *        kernels (the product library, round 6);
 *    1 = the same words written / awaited with hipStreamWriteValue32 / hipStreamWaitValue32 (rounds 5; the A/B build with
 *        GPK_GATE_KERNELS=0).  Observed on ROCm 7.2.0 / gfx950: on a CU-MASKED stream such a write overtook the kernel queued
 *        before it (a wrong factor at n = 5000) -- stream memory operations were therefore only ever used on plain streams, and the
 *        product no longer uses them at all: kernels of one stream execute in order by definition;
 *    0 = events -- when the first factorisation finds that kernels of two streams do NOT run at the same time (a tool that
 *        serialises kernels, e.g. rocprofv3 --pmc, would deadlock the polls);
 *   -1 = no factorisation with n > 128 has been issued on this device yet.
 * Every wait is bounded (0.5 s); one that expires sets the status word to INT_MAX (see "info") and the call returns. */
int gpk_chain_handoff_mode(void);

/* gpk_potrf for callers that also need the explicit inverse factor (the reverse pass: gradients.py; the reference
 * gets the same quantities from the triangular solves inside TF's Cholesky gradient).  A is [n + extra + n, lda]:
 * the square block, `extra` right-hand-side rows, and n more rows that the CALL overwrites with the identity and
 * returns as L^-T (upper triangular, exact zeros below the diagonal).  Because row j of that block stays zero left
 * of column j until its column group is reached, the identity rows cost n^3/3 flop, not the n^3 of n dense rows.
 * batch 1.  Everything else as gpk_potrf. */
int gpk_potrf_inv(void* stream, double* A, int n, int extra, long lda, double* invd, int zero_upper, int* info);

/* inverses of the diagonal NB-blocks of an existing lower factor L [n,n] (for gpk_trsm on a cached
 * L: GPRPosterior cache (err, Lm), posteriors.py:415-432). invd [batch, ceil(n/NB), NB, NB]. */
int gpk_trtri_blocks(void* stream, const double* L, int n, long ldl, int batch, long strideL,
                     double* invd);

/* ---- triangular solve against an existing factor (right-side, row-major form) -------------------
 * trans = 0:  B <- B L^-T   (rows of B are right-hand sides;  = (L^-1 B^T)^T, util.py:125)
 *             pass L (lower, ldl) and invd.
 * trans = 1:  B <- B L^-1   (= (L^-T B^T)^T, triangular_solve(adjoint(Lm), A, lower=False) util.py:139)
 *             pass LT = L^T (upper, row-major) as `L` and the blockwise transposed inverses invdT as
 *             `invd`; both come from gpk_transpose_factor.
 * B [m,n] ldb, solved in place. */
int gpk_trsm(void* stream, int trans, const double* L, long ldl, const double* invd, int n,
             double* B, int m, long ldb, int batch, long strideL, long strideB);
int gpk_transpose_factor(void* stream, const double* L, long ldl, const double* invd, int n,
                         double* LT, long ldlt, double* invdT);

/* ---- GEMM  C = alpha * A * B^T + beta * C  (A [m,k], B [n,k], C [m,n]; fp64 MFMA) ----------------
 * tf.linalg.matmul call sites (conditionals/util.py:129,144,157,162; posteriors.py:734,803-818).
 * b_tri, bits 0-1: 0 dense; 1 B is upper in [n,k] (B[j,kk] == 0 for kk < j, must be stored as zeros);
 *        2 B is lower (B[j,kk] == 0 for kk > j).  Bits 4-5 (optional hint about A, m <= k): 16 = A is upper
 *        (A[i,kk] == 0 for kk < i), 32 = A is lower (A[i,kk] == 0 for kk > i), stored as zeros as well; a tile's K range
 *        is then the intersection of both structures -- the triangular x triangular products of the reverse pass
 *        (K^-1 = L^-T L^-1, the Cholesky adjoint) at half the multiply-adds.  c_lower: only tiles touching the lower
 *        triangle.  Bit 8 (256, round 6): the `batch` entries are consecutive K chunks of ONE triangular product -- entry z
 *        holds columns z k .. (z + 1) k of both operands (strideA = strideB = k on the unsplit arrays), the triangular
 *        statements refer to the unsplit column index, k must be a multiple of 16 -- and the caller sums the partial
 *        products (gpk_combine_parts).  A 2048^3 triangular x triangular product is 256 output tiles whose longest walks
 *        K = 2048 (245 us); as 4 chunks it is one round of 480 non-empty tiles (gradients.py, cholesky_adjoint). */
int gpk_gemm_nt(void* stream, int m, int n, int k, double alpha, const double* A, long lda,
                const double* B, long ldb, double beta, double* C, long ldc, int b_tri,
                int c_lower, int batch, long strideA, long strideB, long strideC);

/* out[j,i] = in[i,j]; mode 0 plain, 1 keep the lower triangle of `in` only (band_part(q_sqrt,-1,0),
 * conditionals/util.py:151, kullback_leiblers.py:120), 2 keep upper only. in [rows,cols]. */
int gpk_transpose(void* stream, const double* in, int rows, int cols, long ldin, double* out,
                  long ldout, int mode, int batch, long stride_in, long stride_out);

/* Row statistics of At [rows, m] (= A^T of the conditional), one pass over At:
 *   sumsq[b]  = beta*sumsq[b] + alpha * sum_k At[b,k]^2        (util.py:133 reduce_sum(square(A), -2))
 *   mv[b,p]   = sum_k At[b,k] V[k,p]                           (util.py:144  A^T f;  V [m,P])
 *   wsq[p,b]  = sum_k (At[b,k] W[k,p])^2                       (util.py:149,164 q_diag; W [m,P])
 * any of sumsq / (V,mv) / (W,wsq) may be NULL. */
int gpk_row_stats(void* stream, const double* At, int rows, int m, long ldat, const double* V,
                  const double* W, int P, double alpha, double beta, double* sumsq, double* mv,
                  double* wsq);
int gpk_row_sumsq(void* stream, const double* A, int rows, int cols, long lda, double alpha,
                  double beta, double* out);
/* out[i] = beta*out[i] + alpha * sum_j A[i,j] B[i,j]   (tf.reduce_sum(Kuf * matmul(Qinv, Kuf), -2),
 * posteriors.py:818, in the row-major transposed form) */
int gpk_row_dot(void* stream, const double* A, long lda, const double* B, long ldb, int rows,
                int cols, double alpha, double beta, double* out);

/* Projection onto the variational square roots (util.py:151-164, triangular-aware, never
 * materialises LTA):  ssq[p,b] = sum_j ( sum_k At[b,k] Lq_p[k,j] )^2
 * LqT [P, m, ldl] = tril(q_sqrt_p)^T, built with gpk_transpose(mode 1). */
size_t gpk_project_workspace_bytes(int rows, int m, int P);
int gpk_project(void* stream, const double* At, int rows, int m, long ldat, const double* LqT,
                long ldl, int P, double* ssq, void* ws, size_t ws_bytes);
/* The same with one At PER latent, At_p = At + p * strideAt (strideAt = 0: gpk_project): the SeparateIndependent
 * conditional (util.py:566-629), whose tf.map_fn over the P problems becomes ONE launch over the batched trapezoid. */
int gpk_project_batched(void* stream, const double* At, int rows, int m, long ldat, long strideAt,
                        const double* LqT, long ldl, int P, double* ssq, void* ws, size_t ws_bytes);
/* gpk_project together with the row statistics of the same At, as the fused SVGP drivers take them:
 *   s0[b] = sum_k At[b,k]^2,  fmean[b,p] = sum_k At[b,k] V[k,p]   (V [m,P] row-major)
 * Where the projection runs on its 128 x 128 tile and P <= 4 they come out of the GEMM itself -- no second pass over At;
 * otherwise from gpk_row_stats.  Deterministic either way: two calls on the same inputs give the same bits. */
int gpk_project_stats(void* stream, const double* At, int rows, int m, long ldat, const double* LqT, long ldl, int P,
                      const double* V, double* s0, double* fmean, double* ssq, void* ws, size_t ws_bytes);

/* ---- scalar tails (deterministic two-stage reductions) ---------------------------------------------
 * Gaussian variational expectations summed over rows and outputs
 * (likelihoods/scalar_continuous.py:139-148 then tf.reduce_sum, svgp.py:181):
 *   fvar[b,p] = knn - s0[b | p,b] + ssq[p,b]
 *   out[0] = sum_b sum_p -0.5 log 2pi - 0.5 log nv - 0.5 ((Y[b,p] - fmean[b,p] - mean_const)^2 + fvar) / nv
 * s0 [rows] or [P,rows] (s0_per_latent), may be NULL; ssq [P,rows] may be NULL; fvar_out [rows,P]
 * optional.  knn: HOST pointer, P values if knn_per_latent else 1.
 * noise_rows: DEVICE pointer to one noise variance PER ROW [rows] -- a heteroskedastic Gaussian likelihood,
 * Gaussian(variance=Function | scale=Function) evaluated at the rows (scalar_continuous.py:92-111, 139-148: nv becomes
 * nv[b]) -- or NULL for the constant `noise_variance`.  The same pair (noise_variance, noise_rows) appears in the fused
 * drivers below with the same meaning. */
size_t gpk_reduce_workspace_bytes(int n);
int gpk_gaussian_varexp_sum(void* stream, const double* Y, long ldy, const double* fmean, int rows,
                            int P, const double* s0, int s0_per_latent, const double* ssq,
                            const double* knn_host, int knn_per_latent, double noise_variance,
                            const double* noise_rows, double mean_const, double* fvar_out, double* out, void* ws,
                            size_t ws_bytes);

/* Non-Gaussian variational expectations by Gauss-Hermite quadrature -- the counterpart of gpk_gaussian_varexp_sum for the
 * scalar likelihoods of likelihoods/scalar_discrete.py and scalar_continuous.py (ScalarLikelihood.variational_expectations,
 * likelihoods/base.py, through quadrature/gauss_hermite.py with DEFAULT_NUM_GAUSS_HERMITE_POINTS = 20):
 *   fvar[b,p] = knn - s0[b | p,b] + ssq[p,b],   mu = fmean[b,p] + mean_const,   sum_h (w_h / sqrt pi) g(mu + sqrt(2 fvar) x_h)
 *   VE[b,p]   = that sum with g(f) = log p(Y[b,p] | f)
 *   out[0] = sum_b sum_p VE[b,p];   out[1] = sum_b sum_p dVE/dtheta, theta the code's one trainable parameter
 *                                     (GPK_LIK_STUDENT_T: scale; exactly 0 for a code without one; the later codes: see below)
 *   rows_out [rows]   = sum_p VE[b,p]                      (what variational_expectations returns)
 *   dmu_out, dvar_out [rows,P] = dVE/dfmean, dVE/dfvar: the exact derivatives of the quadrature sum,
 *                       sum_h (w_h / sqrt pi) g'(f_h)  and  sum_h (w_h / sqrt pi) g'(f_h) x_h / sqrt(2 fvar)
 * Operands as gpk_gaussian_varexp_sum (Y/ldy, fmean contiguous [rows,P], s0 / ssq / fvar_out optional, knn a HOST pointer,
 * 1 <= P <= 16, rows = 0 writes out = [0, 0]); rows_out, dmu_out, dvar_out optional.  lik and lik_params_host (HOST pointer):
 *   GPK_LIK_BERNOULLI_PROBIT  g = log(y == 1 ? p : 1 - p), p = 0.5 (1 + erf(f / sqrt 2)) (1 - 2e-3) + 1e-3;  no parameters (NULL)
 *   GPK_LIK_POISSON_EXP       params = {binsize}: the reference's closed form (no quadrature)
 *                             VE = y mu - exp(mu + fvar / 2) binsize - lgamma(y + 1) + y log(binsize)
 *   GPK_LIK_STUDENT_T         params = {scale, df}: g = lgamma((df+1)/2) - lgamma(df/2) - (log scale^2 + log df + log pi) / 2
 *                                                       - (df + 1) / 2 log(1 + ((y - f) / scale)^2 / df)
 * An unknown code returns GPK_E_UNSUPPORTED, a missing or non-positive parameter GPK_E_ARG.  fvar is not clamped: a negative
 * value gives NaN through the square root, as in the reference.  NaN / Inf in Y, fmean or fvar reach out and the element's
 * own rows_out / dmu_out / dvar_out entries (a non-finite label adds y - y to each of them), and nothing else.
 * Deterministic: four lanes share an element and combine in a fixed shuffle order, then the two-stage reduction.
 *
 *   GPK_LIK_MULTICLASS_ROBUSTMAX  params = {epsilon}: MultiClass with the RobustMax link (likelihoods/multiclass.py).  NOT a scalar
 *   likelihood: the P latents of a row are the P classes, coupled under one quadrature sum.  With y the row's label,
 *     s = sqrt(max(2 fvar_y, 1e-10)),  X_h = mu_y + s x_h,  d_kh = (X_h - mu_k) / sqrt(max(fvar_k, 1e-10)),
 *     c_kh = 0.5 erfc(-d_kh / sqrt 2) (1 - 2e-4) + 1e-4,  p = sum_h (w_h / sqrt pi) prod_{k != y} c_kh   (k ascending)
 *     VE_b = p log(1 - epsilon) + (1 - p) log(epsilon / (P - 1))
 *   Classes: 2 <= P <= 16; P = 1 is GPK_E_ARG.  Epsilon: 0 < epsilon < 1, else (or NULL) GPK_E_ARG.
 *   Labels: Y has ONE column: the label of row b is Y[b * ldy] for every latent; ldy >= 1 is all that is required.  A label that
 *   is not an integer in [0, P) -- NaN and +-Inf included -- makes the row's outputs NaN (rows_out[b], all P entries of dmu_out /
 *   dvar_out, its term of out[0]) and affects nothing else.  This is a choice: the reference would index garbage there.
 *   Outputs: out[0] = sum_b VE_b (a row counts once, not once per latent); out[1] = 0; rows_out[b] = VE_b; dmu_out, dvar_out
 *   [rows,P] = the exact derivatives of VE_b w.r.t. all P means and variances of the row; fvar_out[b,k] = the UNCLAMPED
 *   knn - s0 + ssq.  The optional operands and outputs and rows = 0 behave as for the other codes.
 *   Clamps: unlike the scalar likelihoods a negative (or tiny) fvar is clamped here and does not become NaN -- the reference's
 *   behaviour for this likelihood.  The clamps are comparisons: a NaN variance stays NaN.  Where a clamp is active the
 *   derivative w.r.t. that variance is exactly 0 (tf.clip_by_value under autodiff).
 *   Non-finite inputs: a NaN in fmean[b,:] or fvar[b,:] reaches row b's outputs and out[0], and no other row: the row is the
 *   unit here, not the element.
 *   Deterministic: four lanes per (row, class) group, the product over the row's classes and the sums over them are fixed-order
 *   shuffle loops inside one wave, then the two-stage reduction; no floating-point atomics.
 *
 * Four more SCALAR codes (likelihoods/scalar_continuous.py Exponential, Gamma, Beta; scalar_discrete.py Ordinal; logdensities.py).
 * Operands, optional outputs, rows = 0, P <= 16, the unclamped fvar = knn - s0 + ssq and the y - y rule for a non-finite label are
 * those of the scalar codes above.  For every code out[1] is "the sum of dVE/dtheta for the code's ONE trainable parameter"
 * (StudentT: scale, Gamma: shape, Beta: scale, Ordinal: sigma) and exactly 0 where there is none.
 * Notation: mu = fmean + mean_const, v = fvar, e = exp(-mu + v / 2).
 *   GPK_LIK_EXPONENTIAL_EXP   no parameters (NULL); closed form (no quadrature), one lane per element as Poisson:
 *                             VE = -mu - y e,  dmu = -1 + y e,  dvar = -y e / 2,  out[1] = 0
 *   GPK_LIK_GAMMA_EXP         params = {shape}, shape > 0; closed form:
 *                             VE = -shape mu - lgamma(shape) + (shape - 1) log y - y e,  dmu = -shape + y e,  dvar = -y e / 2,
 *                             dVE/dshape = -mu - psi(shape) + log y.  The host computes lgamma(shape) and psi(shape) once.
 *                             y <= 0 goes through log as it comes (-Inf or NaN, as the reference): no clamp.
 *   GPK_LIK_BETA_PROBIT       params = {scale}, scale > 0; 20-node quadrature, four lanes per element:
 *                             m = 0.5 erfc(-f / sqrt 2) (1 - 2e-3) + 1e-3,  alpha = m scale,  beta = scale - alpha,
 *                             yc = min(max(y, 1e-6), 1 - 1e-6)  (comparisons: a NaN label stays NaN),
 *                             g = (alpha - 1) log yc + (beta - 1) log(1 - yc) + lgamma(scale) - lgamma(alpha) - lgamma(beta)
 *                             g'(f) = scale 0.998 phi(f) (log yc - log(1 - yc) - psi(alpha) + psi(beta))
 *                             dg/dscale = m log yc + (1 - m) log(1 - yc) + psi(scale) - m psi(alpha) - (1 - m) psi(beta)
 *   GPK_LIK_ORDINAL           params = {sigma, n, e_0 ... e_{n-1}}: sigma > 0, 1 <= n <= 15 (n an integer held in a double), the n
 *                             edges finite and strictly increasing; anything else, or NULL, is GPK_E_ARG.  The label y is an
 *                             integer in [0, n]; with e_{-1} = -Inf and e_n = +Inf:
 *                             zl = (e_y - f) / sigma,  zr = (e_{y-1} - f) / sigma,  D = 0.998 (Phi(zl) - Phi(zr)),  g = log(D + 1e-6)
 *                             (the jitters of the two inv_probit cancel).  Phi(zl) - Phi(zr) is taken through erfc on the side
 *                             where both terms are small -- (erfc(zr / sqrt 2) - erfc(zl / sqrt 2)) / 2 when zr >= 0, else
 *                             (erfc(-zl / sqrt 2) - erfc(-zr / sqrt 2)) / 2 -- so that a far tail keeps its relative accuracy.  An
 *                             infinite edge contributes Phi = 0 or 1 and a zero density term (0 * Inf is never formed).
 *                             g'(f) = -0.998 (phi(zl) - phi(zr)) / (sigma (D + 1e-6))
 *                             dg/dsigma = -0.998 (zl phi(zl) - zr phi(zr)) / (sigma (D + 1e-6))
 *                             A label that is not an integer in [0, n] -- NaN and +-Inf included -- makes that ELEMENT's outputs
 *                             NaN (its entries of dmu_out / dvar_out, its row of rows_out, out[0] and out[1]) and affects nothing
 *                             else.  This is the MultiClass choice: the reference would index garbage.
 *   Codes 10 and 11: dmu = sum_h (w_h / sqrt pi) g'(f_h), dvar = sum_h (w_h / sqrt pi) g'(f_h) x_h / sqrt(2 v), the exact derivatives
 *   of the sum, as for Bernoulli and StudentT.  psi is gpk_digamma (csrc/digamma.h: its absolute error bound is derived there).
 *
 * Edges of the SCALAR codes, where the formulas above are taken as they stand (held by tests/test_gpu_likelihood_edges.py):
 *   fvar == 0 exactly.  Quadrature codes (1, 3, 10, 11): sqrt(2 fvar) = 0 and every node is mu, so VE and dmu are the one-point
 *   values g(mu) and g'(mu), to the rounding of the 20-term sums.  dvar = (sum_h (w_h / sqrt pi) g'(mu) x_h) / 0 is NOT finite: NaN
 *   or +-Inf, the numerator being 0 or a rounding residue.  The limit g''(mu) / 2 is not substituted and no epsilon is added under
 *   the root; a caller that differentiates w.r.t. a variance must not pass an exact 0.  Closed forms (2, 8, 9): every output is
 *   finite.  Every other element has the bits it has when this element's fvar is 1.
 *   Overflow inside a closed form: exp(mu + fvar / 2) (Poisson) or e = exp(-mu + fvar / 2) (Exponential, Gamma) is +Inf from an
 *   argument of 709.79 on.  The element's outputs are the IEEE results of the formulas in the order written: VE = -Inf, dvar = -Inf,
 *   dmu = -Inf (Poisson) or +Inf (Exponential, Gamma); with y = 0, y e = 0 * Inf = NaN in all three.  out[0] follows (-Inf, or NaN),
 *   the element's row of rows_out too, and no other element changes.
 *   GPK_LIK_GAMMA_EXP with y = 0: log y = -Inf as it comes.  VE = (shape - 1) (-Inf) + finite terms: -Inf for shape > 1, +Inf for
 *   shape < 1, NaN for shape == 1 (0 * Inf); dmu = -shape and dvar = 0 (y e = 0 exactly); dVE/dshape = -Inf, so out[1] = -Inf for
 *   every shape.
 *
 * Codes: 0 is the Gaussian stage of gpk_svgp_elbo_shard and no likelihood code.  5, 6 and 7 are unassigned and answer
 * GPK_E_UNSUPPORTED: they are kept for links of the codes 1 .. 4 should those be built (Bernoulli with the logistic link, Poisson
 * with softplus, MultiClass with Softmax), so that a family's links stay next to each other; callers and tests rely on 5 being unknown. */
#define GPK_LIK_BERNOULLI_PROBIT 1
#define GPK_LIK_POISSON_EXP 2
#define GPK_LIK_STUDENT_T 3
#define GPK_LIK_MULTICLASS_ROBUSTMAX 4
#define GPK_LIK_EXPONENTIAL_EXP 8
#define GPK_LIK_GAMMA_EXP 9
#define GPK_LIK_BETA_PROBIT 10
#define GPK_LIK_ORDINAL 11
int gpk_likelihood_varexp_sum(void* stream, int lik, const double* lik_params_host, const double* Y, long ldy,
                              const double* fmean, int rows, int P, const double* s0, int s0_per_latent, const double* ssq,
                              const double* knn_host, int knn_per_latent, double mean_const, double* fvar_out,
                              double* rows_out, double* dmu_out, double* dvar_out, double* out, void* ws, size_t ws_bytes);
/* Variational expectations of a SWITCHED likelihood (likelihoods/misc.py SwitchedLikelihood): every row is scored by the likelihood of
 * its own task, in one launch (csrc/switched/switched_varexp.hip).  Operands not named here behave exactly as they do in
 * gpk_likelihood_varexp_sum (fmean contiguous [rows,P], s0 / ssq / fvar_out / rows_out / dmu_out / dvar_out optional, knn a HOST pointer).
 *   Tasks: 1 <= T <= 16 and 1 <= P <= 16, else GPK_E_ARG.  Row b's task is t = label_of(Y[b * ldy + ylab], T), the rule of the
 *   Coregion kernel (csrc/label.h): truncation toward zero, the test -1 < x < T made on the DOUBLE before any conversion to an integer;
 *   an invalid label is -1 and never forms an address.  The value columns are Y[b * ldy + p], p < P, so ylab >= P is required, and
 *   ylab < ldy (GPK_E_ARG otherwise).
 *   Codes: codes_host[t] is a GPK_LIK_* value of a SCALAR code, or 0.  In this table, and only here, 0 means a Gaussian with
 *   params = {variance}, variance > 0 (the remark below, "0 is ... no likelihood code", stays true for every other entry point).
 *   Accepted: 0, 1 (Bernoulli), 2 (Poisson), 3 (StudentT), 8 (Exponential), 9 (Gamma), 10 (Beta).  4 (MultiClass couples a row's
 *   latents), 11 (Ordinal: an edge table per task) and 5 - 7 answer GPK_E_UNSUPPORTED.  params_host is [T][2] row-major; each member's
 *   parameters are checked by the code's own rule above (GPK_E_ARG); entries a code does not use are ignored.  A refused call writes
 *   nothing.
 *   Elements: the formulas of each code, above.  The Gaussian member, with mu = fmean + mean_const, v = fvar, s2 = its variance:
 *     VE = -0.5 log 2pi - 0.5 log s2 - 0.5 ((y - mu)^2 + v) / s2,  dmu = (y - mu) / s2,  dvar = -0.5 / s2,
 *     dVE/ds2 = -0.5 / s2 + 0.5 ((y - mu)^2 + v) / s2^2;  a non-finite label adds y - y to VE, dmu and dvar, as for the scalar codes.
 *   Outputs: out[0] = sum_b sum_p VE;  out[1 + t] = the sum over the elements of task t's rows of dVE/dtheta_t, theta_t that code's one
 *   trainable parameter (Gaussian: variance, StudentT: scale, Gamma: shape, Beta: scale), exactly 0 for a code without one and for a
 *   task with no rows.  rows_out, dmu_out, dvar_out, fvar_out keep their meaning.  rows = 0 writes out = 0 (all 1 + T entries) and
 *   nothing else.
 *   An invalid task label (NaN, +-Inf, <= -1, >= T) makes that ROW's outputs NaN -- rows_out[b], its P entries of dmu_out / dvar_out,
 *   its term of out[0] -- and touches no other row and no out[1 + t] (the row belongs to no task); fvar_out is still the unclamped
 *   knn - s0 + ssq there.  Non-finite values in Y's value columns, fmean or fvar follow the member code's rule and reach that task's
 *   out[1 + t] exactly where the rule reaches out[1] of gpk_likelihood_varexp_sum.
 *   Deterministic: no floating-point atomics, bit-identical on a rerun; each element's dmu, dvar, fvar and each row's rows_out do not
 *   depend on where the row sits or on which tasks share its wave (the sums out[] depend on the order of the rows).
 *   Scratch: parts, (1 + T) * gpk_switched_varexp_blocks(rows, P) doubles; its contents at entry do not matter and nothing past that
 *   extent is touched. */
int gpk_switched_varexp_blocks(int rows, int P);
int gpk_switched_varexp_sum(void* stream, int T, const int* codes_host, const double* params_host, const double* Y, long ldy, int ylab,
                            const double* fmean, int rows, int P, const double* s0, int s0_per_latent, const double* ssq,
                            const double* knn_host, int knn_per_latent, double mean_const, double* fvar_out, double* rows_out,
                            double* dmu_out, double* dvar_out, double* out, double* parts);
/* Gaussian variational expectations of LINEARLY MIXED latents -- the stage between the latent moments and the likelihood of a
 * LinearCoregionalization model (kernels/multioutput/kernels.py LinearCoregionalization, conditionals/util.py mix_latent_gp):
 * L latent GPs g, P outputs f = W g, W [P, L] row-major on the HOST, 1 <= L, P <= 16.  The latent operands are those of
 * gpk_gaussian_varexp_sum with L in the place of P: gmean [rows, L] contiguous, s0 [rows] or [L, rows] (s0_per_latent), ssq
 * [L, rows], either may be NULL; knn a HOST pointer, L values if knn_per_latent else 1.  Y [rows, P] with row stride ldy.
 *   gvar[b,l] = knn - s0 + ssq                                      (in this order)
 *   f[b,p]    = sum_l W[p,l] gmean[b,l] + mean_const                (l ascending; the constant is added AFTER the mixing)
 *   fvar[b,p] = sum_l W[p,l]^2 gvar[b,l]
 *   VE[b,p]   = -0.5 log 2pi - 0.5 log s2 - 0.5 ((Y[b,p] - f[b,p])^2 + fvar[b,p]) / s2,      s2 = noise_variance
 *   out[0]    = sum_b sum_p VE[b,p]
 *   out[1]    = d out[0] / d s2 = sum_bp ( -0.5 / s2 + 0.5 ((Y - f)^2 + fvar) / s2^2 )
 *   dgmu[b,l] = ( sum_p W[p,l] (Y[b,p] - f[b,p]) ) / s2             (d out[0] / d gmean[b,l]; p ascending)
 *   dW[p,l]   = ( sum_b (Y[b,p] - f[b,p]) gmean[b,l] - W[p,l] gvar[b,l] ) / s2      (d out[0] / d W[p,l]; DEVICE, [P, L])
 * d out[0] / d gvar[b,l] = -sum_p W[p,l]^2 / (2 s2) is the same for every row and is left to the caller.
 * fmean_out, fvar_out [rows, P], dgmu_out [rows, L] and dW_out are optional (NULL).  rows = 0 writes out = [0, 0] and dW = 0 and
 * reads no row operand.  GPK_E_ARG: L or P outside [1, 16], W_host / knn_host / out NULL, noise_variance not > 0 (NaN included);
 * GPK_E_WORKSPACE: ws smaller than gpk_mixed_varexp_workspace_bytes(rows, L, P).  A refused call writes nothing.
 * fvar is not clamped: a negative gvar gives a smaller (or negative) fvar, as in the reference.
 * Non-finite inputs: a NaN / Inf in gmean[b,:], gvar[b,:] or Y[b,p] travels through the arithmetic into out, into dW and into
 * those of row b's fmean / fvar / dgmu entries that depend on it (gmean[b,l]: f[b,:] and dgmu[b,:]; gvar[b,l]: fvar[b,:];
 * Y[b,p]: dgmu[b,:]; a zero weight does not shield: 0 * NaN = NaN).  It reaches no other row's per-row outputs.
 * Deterministic: max(L, P) adjacent lanes share a row, whole rows per wave pass; the sums over l and p are fixed-order shuffle
 * loops inside the wave; out and dW go through two-stage reductions (dW: one [P L] partial per stage-1 block, summed in block
 * order); no floating-point atomics, no in-kernel waits. */
size_t gpk_mixed_varexp_workspace_bytes(int rows, int L, int P);
int gpk_mixed_gaussian_varexp_sum(void* stream, const double* Y, long ldy, const double* gmean, int rows, int L, int P,
                                  const double* W_host, const double* s0, int s0_per_latent, const double* ssq,
                                  const double* knn_host, int knn_per_latent, double noise_variance, double mean_const,
                                  double* fmean_out, double* fvar_out, double* dgmu_out, double* dW_out, double* out, void* ws,
                                  size_t ws_bytes);

/* The quadrature table the kernels use: n nodes x_host and weights w_host of numpy.polynomial.hermite.hermgauss(n).  Host only
 * (no stream, no device); n = 20 is the only table: anything else returns GPK_E_UNSUPPORTED. */
int gpk_gauss_hermite(int n, double* x_host, double* w_host);

/* whitened KL (kullback_leiblers.py:98-165 with K None):
 *   out[0] = 0.5 * ( sum q_mu^2 - M*P - sum log diag(Lq)^2 + sum tril(Lq)^2 )
 * q_sqrt [P,m,m] (q_diag = 0) or [m,P] (q_diag = 1). */
int gpk_gauss_kl_white(void* stream, const double* q_mu, const double* q_sqrt, int m, int P,
                       int q_diag, double* out, void* ws, size_t ws_bytes);

/* out[b] = sum_i log(L_b[i,i]) (logdensities.py:154, kullback_leiblers.py:159-160) */
int gpk_sum_log_diag(void* stream, const double* L, int n, long ldl, int batch, long strideL,
                     double* out);
/* out[0] = sum of squares of A [rows,cols] (upper_only: c >= r) -- mahalanobis / trace terms */
int gpk_sumsq(void* stream, const double* A, int rows, int cols, long lda, int upper_only,
              double* out, void* ws, size_t ws_bytes);

/* out [m,n] = alpha * sum_p parts[p]  (parts [nparts, m, n], row stride ldp, part stride stride_part), summed in the
 * order p = 0, 1, ... (deterministic).  lower != 0: entries above the diagonal are written as zeros and never read,
 * the diagonal is multiplied by diag_scale -- i.e. tril(.) (tf.linalg.band_part(., -1, 0), conditionals/util.py:151)
 * or, with diag_scale = 0.5, the Phi(.) of the Cholesky adjoint.  The reduction step of the split-K products of the
 * reverse pass (gradients.py), where TF autodiff's matmul gradients need none. */
int gpk_combine_parts(void* stream, const double* parts, int nparts, long stride_part, int m, int n, long ldp,
                      double alpha, int lower, double diag_scale, double* out, long ldo);

/* ---- glue of the reverse pass as single launches (round 6) -------------------------------------------------
 * The reference gets all of this from TF autodiff and tf.optimizers.Adam (optimizers/scipy.py:322-331,
 * gps_for_big_data.pct.py:207-228); here the reverse pass is written out (gpflow_amd/gradients.py) and these entry
 * points replace ~70 elementwise launches of a few thousand elements each at the end of a training step.
 *
 * gpk_moment_rows:  Vt [1 + 2 d, n2] = [1; B^T; (B^T).^2] for B [n2, d] -- the right-hand side of G [1, B, B^2],
 *   the contraction that turns G = Kbar .* K into lengthscale / input gradients (stationaries.py:209-210 under autodiff). */
int gpk_moment_rows(void* stream, const double* B, long ldb, int n2, int d, double* Vt, long ldv);
/* gpk_stationary_adjoint_tail:  from R [n1, 1 + 2 d] = G [1, B, B^2] (columns: row sums, G B, G B^2), the first kernel
 *   argument A [n1, d] and the lengthscales ls_dev [d] (device):
 *     T = R[:, 1:1+d] - A .* R[:, 0]
 *     symmetric != 0 (B is A, Kbar symmetric):  Abar = 2 T / ls^2,  d/dls = -colsum(A .* Abar) / ls
 *     else:                                      Abar = T / ls^2,    d/dls = colsum(R[:, 1+d:] - A .* (R[:, 1:1+d] + T)) / ls^3
 *     d/dvariance = (sum_kbar_k ? sum_kbar_k[0] : sum(R[:, 0])) / variance
 *   Abar [n1, d]; small [1 + d] = (d/dvariance + dvar_add, d/dls).  accumulate != 0: both are ADDED to what Abar / small
 *   hold (the two adjoints of one kernel -- Kuf and Kuu -- leave their sum).  One workgroup, fixed summation order. */
int gpk_stationary_adjoint_tail(void* stream, const double* R, long ldr, const double* A, long lda, int n1, int d,
                                const double* ls_dev, double variance, int symmetric, const double* sum_kbar_k,
                                double* Abar, long ldab, double* small, int accumulate, double dvar_add);
/* ---- the Periodic kernel's input warp (periodic.hip) --------------------------------------------------------
 * Periodic over a base kernel k evaluated on r^2 (gpflow/kernels/periodic.py):  k(r^2),  r^2 = sum_j sin^2(pi (x_j - x'_j) / p_j) / l_j^2.
 * With a_j = 2 pi x_j / p_j and Phi(x) = (cos a_1, sin a_1, ..., cos a_d, sin a_d):  |Phi_j(x) - Phi_j(x')|^2 = 4 sin^2(pi (x_j - x'_j) / p_j),
 * so it is the base kernel on Phi(X) [n, 2 d] with lengthscales 2 l_j for both columns of pair j: every builder and driver above
 * takes it as a stationary leaf of width 2 d <= GPK_MAX_D.  period_host: HOST pointer, d entries if ard_period, else one (as ls_host).
 * All three return GPK_E_ARG -- before any launch -- for d <= 0, 2 d > GPK_MAX_D, a leading dimension that is too small or a period
 * that is not positive and finite.
 *
 * gpk_periodic_warp:  Phi[i, 2 j] = cos(2 pi x_ij / p_j),  Phi[i, 2 j + 1] = sin(2 pi x_ij / p_j)  as sincospi(2 x / p): x = k p gives
 *   exactly (1, 0).  X [n, d] ldx, Phi [n, 2 d] ldphi (padding beyond 2 d is never written); n == 0 returns 0 without a launch.  A NaN
 *   or Inf in x_ij makes Phi[i, 2 j] and Phi[i, 2 j + 1] NaN and nothing else. */
int gpk_periodic_warp(void* stream, const double* X, long ldx, int n, int d, const double* period_host, int ard_period, double* Phi,
                      long ldphi);
/* gpk_periodic_moment_rows:  Vt [1 + 6 d, n2] ldv = [1 ; Phi(B)^T ; (Phi(B).^2)^T ; (b .* cos)^T, (b .* sin)^T interleaved as Phi is] for
 *   B [n2, d].  The first 1 + 4 d rows are gpk_moment_rows of gpk_periodic_warp(B), bit for bit; R = G Vt^T [n1, 1 + 6 d] feeds
 *   gpk_stationary_adjoint_tail (its first 1 + 4 d columns, ldr = 1 + 6 d) and gpk_periodic_adjoint_tail. */
int gpk_periodic_moment_rows(void* stream, const double* B, long ldb, int n2, int d, const double* period_host, int ard_period, double* Vt,
                             long ldv);
/* gpk_periodic_adjoint_tail:  from the first argument X [n1, d], Phi = Phi(X) [n1, 2 d], Phibar [n1, 2 d] (the Abar of
 *   gpk_stationary_adjoint_tail at the warped inputs), R [n1, 1 + 6 d] as above (G = Kbar .* (-2 dK/dr^2)), the BASE lengthscales
 *   ls_dev [d] (device; an isotropic one repeated) and the periods:
 *     Xbar[i, j] = (2 pi / p_j) (c_ij Phibar[i, 2 j + 1] - s_ij Phibar[i, 2 j])
 *     dperiod_j  = pi / (2 p_j^2 l_j^2) sum_i [x_ij s_ij (G c')_ij - x_ij c_ij (G s')_ij - s_ij (G (b c'))_ij + c_ij (G (b s'))_ij]
 *   the total derivative of sum(Kbar .* K) w.r.t. p_j: both arguments of K, so symmetric and non-symmetric calls are the same.
 *   dperiod [d] if ard_period, else [1]: the sum over j.  accumulate != 0: Xbar and dperiod are ADDED to.  One workgroup, fixed
 *   summation order, no atomics. */
int gpk_periodic_adjoint_tail(void* stream, const double* X, long ldx, const double* Phi, long ldphi, const double* Phibar, long ldpb,
                              const double* R, long ldr, int n1, int d, const double* ls_dev, const double* period_host, int ard_period,
                              double* Xbar, long ldxb, double* dperiod, int accumulate);
/* ---- dot-product kernels (dot.hip): Linear and Polynomial (gpflow/kernels/linears.py) ----------------------------------
 * With s(x, y) = sum_j (x_j w_j) y_j and base = s + offset:
 *     GPK_DOT_LINEAR      k = s                  dk/ds = 1
 *     GPK_DOT_POLYNOMIAL  k = base^degree        dk/ds = dk/doffset = degree base^(degree - 1)
 * These are NOT GPK_KERN_* families and no fused driver takes them: K(x, x) = k(s(x, x)) depends on the row.
 * w_host: HOST pointer, d entries if ard, else one (as ls_host).  x_j w_j is formed first (X * variance of the reference: one
 * rounding), the sum over j is an fma chain in ascending j.  degree in [1, GPK_DOT_MAX_DEGREE]; the power is the product
 * base * base * ... taken left to right, never pow: a negative base behaves as the reference's integer power.  offset and degree are
 * ignored by GPK_DOT_LINEAR (pass 0.0 and 1).
 * Every entry point returns, before any launch: GPK_E_ARG for d <= 0, d > GPK_MAX_D, a negative size, a leading dimension that is
 * too small, w_host == NULL, a weight or an offset that is not finite, a Polynomial degree outside [1, 16], an op out of range;
 * GPK_E_UNSUPPORTED for a family other than the two.  Signs are not checked.  NaN / Inf propagate as through a matmul: a NaN in row
 * i of X1 makes row i of K NaN (in the symmetric build column i as well) and nothing else.
 *
 * gpk_dot_kernel_matrix: the contract of gpk_kernel_matrix -- X2 == NULL: K(X1, X1) + diag_add I; lower_only; an operand without
 *   elements may be NULL; nothing beyond n1 x n2 is written.  SYMMETRY: (x_i w) . x_j and (x_j w) . x_i differ in the last bit.  The
 *   symmetric build computes the elements on or below the diagonal and writes each to its mirror position, so its output is exactly
 *   symmetric (lower_only: bit for bit the lower triangle of the full build); with X2 given nothing is promised, as by a matmul. */
#define GPK_DOT_LINEAR 0
#define GPK_DOT_POLYNOMIAL 1
#define GPK_DOT_MAX_DEGREE 16
int gpk_dot_kernel_matrix(void* stream, int family, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d,
                          const double* w_host, int ard, double offset, int degree, double diag_add, int lower_only, double* K,
                          long ldk);
/* gpk_dot_kernel_matrix_combine:  out = G .* k (op 1), G + k (op 2) or G .* dk/ds (op 3; Linear: a copy of G), k recomputed from the
 *   inputs; out may alias G.  X2 == NULL: K(X1, X1) element by element (no mirror), diag_add onto the diagonal of the combined
 *   result for ops 1 and 2.  Unlike op 3 of gpk_kernel_matrix_combine the diagonal is NOT zeroed: s_ii depends on the parameters. */
int gpk_dot_kernel_matrix_combine(void* stream, int family, int op, const double* X1, int n1, long ldx1, const double* X2, int n2,
                                  long ldx2, int d, const double* w_host, int ard, double offset, int degree, double diag_add,
                                  const double* G, long ldg, double* out, long ldo);
/* gpk_dot_kernel_diag:  the row diagonal kd_i = k(s(x_i, x_i)) over the rows of X [n, d] ldx, summed as the builder sums it (kd is the
 *   diagonal of gpk_dot_kernel_matrix(X, NULL) without diag_add, bit for bit).  op 0: out = kd; 1: out = g .* kd; 2: out = g + kd;
 *   3: out = g .* dkd/ds_i.  g [n] (DEVICE; not read by op 0), out [n]; out may alias g. */
int gpk_dot_kernel_diag(void* stream, int family, int op, const double* X, int n, long ldx, int d, const double* w_host, int ard,
                        double offset, int degree, const double* g, double* out);
/* gpk_dot_adjoint_tail:  from R [n1, >= 1 + d] ldr = G [1, B] (column 0: the row sums of G = Kbar .* dk/ds, columns 1 .. d: G B), the
 *   first kernel argument A [n1, d] and the weights w_dev (DEVICE; d entries if ard, else one):
 *     d/dw_j     = sum_i A_ij R_i,1+j      (summed over j as well when !ard)
 *     d/doffset  = sum_i R_i0
 *     Abar_ij    = w_j R_i,1+j             (times 2 when symmetric: B is A and G symmetric, both arguments collected)
 *   dsmall [(ard ? d : 1) + 1] = (d/dw, d/doffset).  From s_ik = sum_j w_j a_ij b_kj:  dF/dw_j = sum_ik G_ik a_ij b_kj,
 *   dF/da_ij = w_j (G B)_ij.  One workgroup, fixed summation order: a second call is bit-identical. */
int gpk_dot_adjoint_tail(void* stream, const double* R, long ldr, const double* A, long lda, int n1, int d, const double* w_dev, int ard,
                         int symmetric, double* dsmall, double* Abar, long ldab);
/* ---- ArcCosine kernel (arccosine/arccosine.hip; gpflow/kernels/misc.py) -------------------------------------------------------
 * With w (weight_variances: w_host, HOST pointer, d entries if ard, else one), b (bias_variance), v (variance), eps = 1e-15:
 *     s(x, y) = sum_j (x_j w_j) y_j + b        p(x) = s(x, x)        c = s / (sqrt p(x) sqrt p(y))
 *     theta = acos(clamp(eps + (1 - 2 eps) c))
 *     J_0 = pi - theta   J_1 = sin theta + (pi - theta) cos theta   J_2 = 3 sin theta cos theta + (pi - theta)(1 + 2 cos^2 theta)
 *     K(x, y) = (v / pi) J_order(theta) p(x)^(order/2) p(y)^(order/2)        K_diag(x) = v jf p(x)^order,  jf = 1, 1, 3
 * order in {0, 1, 2}.  x_j w_j is formed first (one rounding), the sum over j is an fma chain over ascending j from 0.0, b is added
 * last; p comes from the same chain, so p of a row as first and as second argument has the same bits.  Not a GPK_KERN_* family, not a
 * GPK_DOT_* code; no fused driver takes it (K(x, x) depends on the row).
 *  1. DIAGONAL BY INDEX: with X2 == NULL the element (i, i) takes c = 1 because row index == column index, never by comparing
 *     values: its acos argument is the double 1.0 - 1e-15, its value (v / pi) J(acos(1 - eps)) p_i^order; in the adjoint stage its
 *     angular derivative is zero and only p_i^order differentiates.  K_diag (gpk_arccos_kernel_diag) is the closed form and is NOT
 *     the diagonal of K(X, X) bit for bit (a relative 1.4e-8 apart at order 0, as in the reference).
 *     (A row that holds a NaN or an Inf makes its own diagonal element NaN as well: the constant enters as fma(sqrt p sqrt q, 0, 1 - eps).)
 *  2. RANGE: the acos argument is clamped to [-1, 1] by comparisons that a NaN fails, so a NaN / Inf in a row of X1 (X2) makes
 *     exactly that row (column) of K NaN.
 *  3. (dJ/dtheta)(dtheta/d arg) = 1 / sin theta, pi - theta, 4 J_1 for orders 0, 1, 2, with cos theta = the clamped argument and
 *     sin theta = sqrt((1 - cos)(1 + cos)): acos and sqrt only.  Order 0 is infinite where the argument is +-1 off the diagonal.
 * Every entry point returns, before any launch: GPK_E_ARG for d outside 1 .. GPK_MAX_D, w_host == NULL, a weight that is negative or
 * not finite, b <= 0 or not finite, v not finite, a negative size, a leading dimension that is too small, an op out of range, a NULL
 * operand that has elements; GPK_E_UNSUPPORTED for an order outside 0 .. 2; 0 without a launch for an operand without elements.
 *
 * gpk_arccos_kernel_matrix: the contract of gpk_dot_kernel_matrix -- X2 == NULL: K(X1, X1) + diag_add I, computed on or below the
 *   diagonal and mirrored (exactly symmetric; lower_only: bit for bit the lower triangle of the full build); nothing beyond n1 x n2 is
 *   written.
 * gpk_arccos_kernel_matrix_combine: out = G .* k (op 1) or G + k (op 2), k recomputed; out may alias G; X2 == NULL: K(X1, X1) element by
 *   element with the diagonal by index, diag_add onto the diagonal of the combined result.
 * gpk_arccos_kernel_diag: over the rows of X [n, d] ldx.  op 0: out = kd; 1: g .* kd; 2: g + kd; 3: g .* dkd/dp (0, v, 6 v p).  g [n]
 *   (DEVICE; not read by op 0), out [n]; out may alias g.  A NaN / Inf in row i reaches out[i] at every order.
 * gpk_arccos_adjoint_stage: ONE pass over Kbar [n1, n2] ldkb that recomputes s, p, q, theta per 64 x 64 tile and writes
 *     G = Kbar .* dk/ds  [n1, n2] ldg (G may alias Kbar), and into parts, with tr = ceil(n1 / 64), tc = ceil(n2 / 64):
 *     parts[t * n1 + i],  t < tc                   the sum over the columns k of column tile t of Kbar_ik dk/dp_i
 *     parts[tc * n1 + t * n2 + k],  t < tr         the sum over the rows i of row tile t of Kbar_ik dk/dq_k
 *     parts[tc * n1 + tr * n2 + tY * tc + tX]      the sum over tile (tY, tX) of Kbar_ik J_ik p_i^(order/2) q_k^(order/2)
 *   parts is scratch of tc n1 + tr n2 + tr tc doubles (GPK_ARC_TILE = 64): the call writes every slot, each by exactly one workgroup in
 *   a fixed order, reads none and touches nothing beyond that extent; no atomics, a second call gives the same bits.  X2 == NULL:
 *   K(X1, X1), every element computed (no mirror), the diagonal by index.
 * gpk_arccos_adjoint_tail: one workgroup.  From R [n1, >= 1 + d] ldr = G [1, B] (column 0: row sums of G, columns 1 .. d: G B), the
 *   parts of the stage, A [n1, d] and B [n2, d] (NULL: symmetric -- B is A, Kbar symmetric, both arguments collected), with
 *   rho_i = sum_t parts[t n1 + i], gamma_k = sum_t parts[tc n1 + t n2 + k]:
 *     dsmall[0]              d/dv  = (1 / pi) sum of the tile sums
 *     dsmall[1 ..]           d/dw_j = sum_i A_ij R_i,1+j + sum_i rho_i A_ij^2 + sum_k gamma_k B_kj^2     (summed over j when !ard)
 *     dsmall[last]           d/db  = sum_i R_i0 + sum_i rho_i + sum_k gamma_k
 *     Abar_ij = w_j R_i,1+j + 2 w_j A_ij rho_i        (symmetric: 2 w_j R_i,1+j + 2 w_j A_ij (rho_i + gamma_i))
 *   dsmall [1 + (ard ? d : 1) + 1]; rg: scratch of n1 + n2 doubles (the summed rho, gamma).  Fixed summation order: a second call is
 *   bit-identical.  n1 == 0 or n2 == 0: dsmall is zeros, Abar is not written. */
#define GPK_ARC_TILE 64
int gpk_arccos_kernel_matrix(void* stream, int order, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d,
                             const double* w_host, int ard, double variance, double bias, double diag_add, int lower_only, double* K,
                             long ldk);
int gpk_arccos_kernel_matrix_combine(void* stream, int order, int op, const double* X1, int n1, long ldx1, const double* X2, int n2,
                                     long ldx2, int d, const double* w_host, int ard, double variance, double bias, double diag_add,
                                     const double* G, long ldg, double* out, long ldo);
int gpk_arccos_kernel_diag(void* stream, int order, int op, const double* X, int n, long ldx, int d, const double* w_host, int ard,
                           double variance, double bias, const double* g, double* out);
int gpk_arccos_adjoint_stage(void* stream, int order, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d,
                             const double* w_host, int ard, double variance, double bias, const double* Kbar, long ldkb, double* G,
                             long ldg, double* parts);
int gpk_arccos_adjoint_tail(void* stream, const double* R, long ldr, const double* A, long lda, int n1, const double* B, long ldb, int n2,
                            int d, const double* w_host, int ard, const double* parts, double* rg, double* dsmall, double* Abar,
                            long ldab);
/* ---- ChangePoints kernel (changepoints/changepoints.hip; gpflow/kernels/changepoints.py) ---------------------------------------
 * A combination that switches between T = C + 1 member kernels along ONE input column x.  With the locations l_0 <= ... <= l_{C-1}
 * (loc_host) and the steepness s_j > 0 (steep_host), both HOST pointers with C entries, C <= GPK_CP_MAX_MEMBERS - 1:
 *     sig_j(x) = 1 / (1 + exp(-s_j (x - l_j)))          1 - sig_j(x) = 1 / (1 + exp(+s_j (x - l_j)))
 *     a_i(x) = sig_{i-1}(x) (1 - sig_i(x)),  i = 0 .. C  (sig_{-1} = 1, 1 - sig_C = 1)
 *     K(x, y) = sum_i a_i(x) k_i(x, y) a_i(y)            K_diag(x) = sum_i a_i(x)^2 k_i(x, x)
 *  1. 1 - sig_j is its own reciprocal, never a subtraction.
 *  2. A saturated sigmoid is exactly 0 or 1 (exp overflows to Inf, underflows to 0): its member contributes exactly 0, or its full value.
 *  3. The exponent is s (x - l) + (x - x): a NaN or an Inf in x makes every weight of that row NaN, hence exactly that row (column)
 *     of K, and nothing else.
 *  4. The tile passes form w = a_r b_c FIRST, then w * Ki: with b == NULL (b is a) an exactly symmetric Ki stays exactly symmetric.
 * Every entry point returns, before any launch: GPK_E_UNSUPPORTED for C > GPK_CP_MAX_MEMBERS - 1; GPK_E_ARG for C < 0, a NULL
 * loc_host / steep_host with C > 0, a location or steepness that is not finite, a steepness <= 0, locations that are not sorted, a
 * negative size, a leading dimension that is too small, an op out of range, a NULL operand that has elements; 0 without a launch for
 * an operand without elements.  No atomics; a second call gives the same bits; nothing beyond the stated extents is written.
 *
 * gpk_changepoint_weights: A [T, n] lda (>= n), row i = a_i(x_r), from the switch column x_r = x[r ldx] (pass the column's address).
 * gpk_changepoint_fold: over Ki [n1, n2] ldki with a [n1], b [n2] (DEVICE; b == NULL: b is a, n2 is n1, and diag_add goes onto the
 *   diagonal).  op 0: out = (a b^T) .* Ki;  op 1: out = acc + (a b^T) .* Ki.  out may alias Ki (op 0) or acc (op 1).  One pass: Ki and
 *   acc are read once, out is written once.  acc is not read by op 0.
 * gpk_changepoint_adjoint_stage: ONE pass over Kbar [n1, n2] ldkb and Ki [n1, n2] ldki that writes G = Kbar .* (a b^T) [n1, n2] ldg
 *   (the seed of the member's own adjoint; G may alias Ki; Kbar is never written) and into parts, with tr = ceil(n1 / 64),
 *   tc = ceil(n2 / 64):
 *     parts[t * n1 + r],  t < tc               the sum over the columns c of column tile t of Kbar_rc Ki_rc b_c
 *     parts[tc * n1 + t * n2 + c],  t < tr     the sum over the rows r of row tile t of Kbar_rc Ki_rc a_r
 *   parts is scratch of tc n1 + tr n2 doubles (GPK_CP_TILE = 64): the call writes every slot, each by exactly one workgroup in a
 *   fixed order, reads none and touches nothing beyond that extent.  b == NULL: every element is computed (no mirror) and both sets
 *   are filled.
 * gpk_changepoint_adjoint_tail: for ONE argument (the rows, or the columns) with its switch column x [n] ldx.  The weight adjoints are
 *     abar_i[r] = init[i ldinit + r] + sum_{t < ntiles} parts[i member_stride + t n + r]        i = 0 .. C, t ascending
 *   (init [T, n] ldinit may be NULL: zeros; ntiles == 0: parts is not read and may be NULL; for the rows pass the stage's parts and
 *   ntiles = tc, for the columns parts + tc n1 and ntiles = tr; member_stride: from member i's parts to member i + 1's).  With
 *   tbar_j = abar_{j+1} a_{j+1} (1 - sig_j) - abar_j a_j sig_j:
 *     dsmall[j]     = d/dl_j = -s_j sum_r tbar_j          dsmall[C + j] = d/ds_j = sum_r tbar_j (x_r - l_j)          j = 0 .. C-1
 *     xbar[r]       = sum_j s_j tbar_j
 *   Two launches: one thread per row, each workgroup of 256 rows leaving its 2 C sums in red (scratch of ceil(n / 256) 2 C doubles,
 *   every slot written by one workgroup in a fixed order); then ONE workgroup adds them in block order.  C == 0 or n == 0: 0,
 *   nothing is written. */
#define GPK_CP_TILE 64
#define GPK_CP_MAX_MEMBERS 16
int gpk_changepoint_weights(void* stream, const double* x, int n, long ldx, int C, const double* loc_host, const double* steep_host,
                            double* A, long lda);
int gpk_changepoint_fold(void* stream, int op, const double* a, const double* b, int n1, int n2, const double* Ki, long ldki,
                         const double* acc, long ldacc, double diag_add, double* out, long ldo);
int gpk_changepoint_adjoint_stage(void* stream, const double* a, const double* b, int n1, int n2, const double* Kbar, long ldkb,
                                  const double* Ki, long ldki, double* G, long ldg, double* parts);
int gpk_changepoint_adjoint_tail(void* stream, const double* x, int n, long ldx, int C, const double* loc_host, const double* steep_host,
                                 const double* parts, long member_stride, int ntiles, const double* init, long ldinit, double* red,
                                 double* dsmall, double* xbar);
/* ---- Coregion kernel (coregion/coregion.hip; gpflow/kernels/misc.py `Coregion`) --------------------------------------------------
 * The intrinsic-coregionalisation (multi-task) kernel over ONE input column that carries the row's task label.  With W [P, R]
 * (unconstrained) and kappa [P] (positive), P = output_dim <= GPK_COREGION_MAX_OUTPUTS, R = rank <= GPK_COREGION_MAX_RANK:
 *     B = W W^T + diag(kappa)  [P, P]        K(x, y) = B[l(x), l(y)]        K_diag(x) = B[l(x), l(x)]
 * LABELS.  The label l of a row is its one column converted as the reference's tf.cast(., int32) converts it: truncation toward zero
 * (2.7 -> 2, -0.5 -> 0).  A label is VALID when the DOUBLE satisfies -1 < x < P; the test is made on the double, before any
 * conversion to an integer.  Anything else (NaN, +-Inf, x <= -1, x >= P) is an invalid label: it never forms an address, and it follows
 * the library's NaN rule -- a NaN in row i of X1 makes row i of K NaN and nothing else: an invalid label in row i of X1 makes row i of
 * K NaN (in the symmetric build, and for X2, the column as well), kd_i NaN and column i of E NaN, and touches nothing else.
 * B is a TYPED operand (DEVICE, [P, P] row-major, ldb >= P; exactly the P x P elements are read or written), not a workspace.
 * No entry point uses atomics or reads the environment.  Not a GPK_KERN_* family, not a GPK_DOT_* code; no fused driver takes it.
 * Every entry point returns, before any launch and with nothing written: GPK_E_ARG for P <= 0, P > GPK_COREGION_MAX_OUTPUTS, R <= 0,
 * R > GPK_COREGION_MAX_RANK, a negative size, a leading dimension that is too small (ldx < 1), an op out of range, a NULL operand
 * that has elements; 0 without a launch where there is nothing to do.
 *
 * gpk_coregion_output_covariance: one workgroup.  W (DEVICE, [P, R] ldw), kappa (DEVICE, [P]) -> B [P, P] ldb.  B[a, b] is an fma
 *   chain over r ascending from 0.0 of W[a, r] * W[b, r]; on the diagonal kappa[a] is added last.  Products commute, so B is EXACTLY
 *   symmetric; a second call gives the same bits.
 * gpk_coregion_kernel_matrix: the contract of gpk_dot_kernel_matrix over the label columns X1 [n1, 1] ldx1, X2 [n2, 1] ldx2 and B --
 *   X2 == NULL: K(X1, X1) + diag_add I; lower_only: only the elements on or below the diagonal are written; an operand without
 *   elements may be NULL; nothing beyond n1 x n2 is written; any ldk and alignment (K misaligned or ldk odd: scalar stores).  One
 *   64 x 64 tile per workgroup, which stages B and the tile's 64 + 64 labels in LDS; an element is one LDS gather and one global store
 *   and has the BITS of B[l_i, l_k], so the symmetric build is exactly symmetric without a mirror pass and lower_only is bit for bit
 *   the lower triangle of the full build.  diag_add is ignored when X2 is given.
 * gpk_coregion_kernel_matrix_combine: out = G .* k (op 1) or G + k (op 2); out may alias G; X2 == NULL: diag_add goes onto the
 *   diagonal of the combined result.  No derivative op: no parameter enters through a scalar argument.
 * gpk_coregion_kernel_diag: kd_i = B[l_i, l_i], read from B: bit for bit the diagonal of gpk_coregion_kernel_matrix(X, NULL) with
 *   diag_add = 0.  op 0: out = kd; 1: g .* kd; 2: g + kd.  g [n] (DEVICE; not read by op 0), out [n]; out may alias g.
 * gpk_coregion_onehot_rows: E [P, n] lde, E[a, i] = 1 where l_i == a, else 0 (column i all NaN for an invalid label): the right-hand
 *   side of the adjoint's contractions, as gpk_moment_rows is for the dot-product kernels.
 * gpk_coregion_adjoint_tail: one workgroup.  With Bbar[a, b] = sum_{i: l_i = a} sum_{k: l'_k = b} Kbar[i, k] ([P, P] ldbb, DEVICE) and W:
 *     dW [P, R] lddw = (Bbar + Bbar^T) W  -- dW[a, r] is an fma chain over b ascending of (Bbar[a, b] + Bbar[b, a]) * W[b, r]
 *     dkappa [P]     = diag(Bbar)
 *   The same formulas serve K(X, X) with a symmetric Kbar: Bbar already collects both arguments.  Fixed summation order: a second call
 *   is bit-identical. */
#define GPK_COREGION_MAX_OUTPUTS 64
#define GPK_COREGION_MAX_RANK 64
int gpk_coregion_output_covariance(void* stream, const double* W, long ldw, const double* kappa, int P, int R, double* B, long ldb);
int gpk_coregion_kernel_matrix(void* stream, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, const double* B,
                               long ldb, int P, double diag_add, int lower_only, double* K, long ldk);
int gpk_coregion_kernel_matrix_combine(void* stream, int op, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2,
                                       const double* B, long ldb, int P, double diag_add, const double* G, long ldg, double* out,
                                       long ldo);
int gpk_coregion_kernel_diag(void* stream, int op, const double* X, int n, long ldx, const double* B, long ldb, int P, const double* g,
                             double* out);
int gpk_coregion_onehot_rows(void* stream, const double* X, int n, long ldx, int P, double* E, long lde);
int gpk_coregion_adjoint_tail(void* stream, const double* Bbar, long ldbb, const double* W, long ldw, int P, int R, double* dW, long lddw,
                              double* dkappa);
/* gpk_adam_step:  tf.keras Adam on one variable of n doubles, in place:  g' = maximise ? -g : g,
 *   m = beta1 m + (1 - beta1) g',  v = beta2 v + (1 - beta2) g'^2,  p -= step m / (sqrt(v) + epsilon),
 *   step = lr sqrt(1 - beta2^t) / (1 - beta1^t) computed by the caller. */
int gpk_adam_step(void* stream, double* p, const double* g, double* m, double* v, long n, double beta1, double beta2,
                  double epsilon, double step, int maximise);
/* gpk_lowrank_axpy:  out [m, n] = alpha X + U V^T  for thin U [m, k], V [n, k], k <= 16 (out may be X): the first two terms of
 *   At_bar = r q_mu^T - 2 c P At + 2 c sum_p W_p Lq_p^T in one pass (the GEMM that adds the third has beta = 1). */
int gpk_lowrank_axpy(void* stream, double alpha, const double* X, long ldx, const double* U, long ldu, const double* V, long ldv,
                     int m, int n, int k, double* out, long ldo);
/* gpk_symmetrize:  S = (S + S^T) / 2 in place, S [n, n] -- the last step of the Cholesky adjoint. */
int gpk_symmetrize(void* stream, double* S, int n, long lds);

/* ---- fused drivers -----------------------------------------------------------------------------------
 * GPR.log_marginal_likelihood (gpr.py:91-107), stationary kernel, Gaussian noise, constant mean:
 * builds K(X,X)+noise*I (lower) with (Y-mean)^T as extra rows into ws, factors, reduces.
 *   out[0] = LML (summed over the P columns of Y); info: device int.
 * noise_rows (device, [n]) != NULL: K(X,X) + diag(noise_rows) instead -- add_likelihood_noise_cov with
 * likelihood.variance_at(X) (utilities/model_utils.py:46-50, gpr.py:100-101). */
size_t gpk_gpr_lml_workspace_bytes(int n, int d, int P);
int gpk_gpr_lml(void* stream, int family, const double* X, int n, int d, long ldx, const double* Y,
                int P, long ldy, const double* ls_host, int ard, double variance,
                double noise_variance, const double* noise_rows, double mean_const, double* out, int* info,
                void* ws, size_t ws_bytes);

/* One shard of SVGP.elbo (svgp.py:166-181), whitened, one kernel shared by all P latents
 * (IndependentPosteriorSingleOutput posteriors.py:828-841 and the SharedIndependent branch :849-861):
 *   out[0] = sum over this shard's rows of var_exp   (all-reduced across ranks by the caller)
 *   out[1] = KL (replicated; identical on every rank)
 * q_diag: q_sqrt is [m,P] instead of [P,m,m].
 * whiten = 0 (full q_sqrt): KL against N(0, Kuu) (kullback_leiblers.py:98-165 with K) and the un-whitened conditional
 * (conditionals/util.py:128-167, white = False) on ONE factorisation -- [Kuu ; Kfu ; q_mu^T ; tril(q_sqrt_p)^T] as one
 * trapezoid; the reference factors Kuu twice and solves the minibatch columns twice.  whiten = 0 with q_diag (round 5;
 * kullback_leiblers.py:128-165 diag branch, util.py:139-149): the trapezoid is [Kuu ; Kfu ; q_mu^T ; I], the identity rows
 * return Lm^-T, whose row norms are diag(Kuu^-1) (trace term) and which turns the second solve of the minibatch columns
 * into one triangular-K GEMM.  The workspace query takes the same (q_diag, whiten) pair as the call. */
size_t gpk_svgp_elbo_workspace_bytes(int m, int rows, int d, int P, int q_diag, int whiten);
int gpk_svgp_elbo_shard(void* stream, int family, const double* Z, int m, long ldz, const double* Xb,
                        const double* Yb, int rows, long ldxb, long ldyb, int d, int P,
                        const double* ls_host, int ard, double variance, double noise_variance,
                        const double* noise_rows, double jitter, double mean_const, const double* q_mu,
                        const double* q_sqrt, int q_diag, int whiten, double* out, int* info,
                        void* ws, size_t ws_bytes);

/* gpk_svgp_elbo_shard with a non-Gaussian likelihood: (lik, lik_params_host) as in gpk_likelihood_varexp_sum take the place
 * of (noise_variance, noise_rows); out[0] is then the sum of the quadrature variational expectations.  Every form of the shard
 * (whitened or not, full or diagonal q_sqrt), its schedule and its workspace (gpk_svgp_elbo_workspace_bytes) are the same:
 * only the last stage differs.  GPK_LIK_MULTICLASS_ROBUSTMAX: Yb has ONE column (the labels), P >= 2 is the number of classes. */
int gpk_svgp_elbo_shard_lik(void* stream, int family, const double* Z, int m, long ldz, const double* Xb, const double* Yb,
                            int rows, long ldxb, long ldyb, int d, int P, const double* ls_host, int ard, double variance,
                            int lik, const double* lik_params_host, double jitter, double mean_const, const double* q_mu,
                            const double* q_sqrt, int q_diag, int whiten, double* out, int* info, void* ws, size_t ws_bytes);

/* The same for SEPARATE kernels per latent (SeparateIndependent, conditionals/util.py:566-629 behind
 * SeparateIndependentPosterior posteriors.py:863-887), whitened, full q_sqrt [P,m,m]: P covariance pairs into one batched
 * trapezoid, ONE batched factorisation / row-statistics / projection launch sequence instead of the reference's tf.map_fn.
 * family_host [P], variance_host [P], ls_host [P][d] (ard) or [P]: HOST arrays.  Z: latent p's inducing points at
 * Z + p * strideZ (strideZ = 0: shared).  info: P device ints (one factorisation status per latent). */
size_t gpk_svgp_elbo_sep_workspace_bytes(int m, int rows, int d, int P);
int gpk_svgp_elbo_shard_sep(void* stream, const int* family_host, const double* Z, int m, long ldz, long strideZ,
                            const double* Xb, const double* Yb, int rows, long ldxb, long ldyb, int d, int P,
                            const double* ls_host, int ard, const double* variance_host, double noise_variance,
                            const double* noise_rows, double jitter, double mean_const, const double* q_mu,
                            const double* q_sqrt, double* out, int* info, void* ws, size_t ws_bytes);

/* The same schedule for a LinearCoregionalization model: L latent GPs (one kernel each, as above, with L in the place of P: q_mu
 * [m, L], q_sqrt [L, m, m], info L ints) mixed into the P columns of Yb by W_host [P, L] (HOST, row-major), f = W g + mean_const.
 * Factorisation, row statistics and projection are those of gpk_svgp_elbo_shard_sep over the L latents; the last stage is
 * gpk_mixed_gaussian_varexp_sum's.  out[0] = the shard's sum of variational expectations, out[1] = the KL over the L latents.
 * Whitened, full q_sqrt, constant noise variance.  1 <= L, P <= 16. */
size_t gpk_svgp_elbo_lcm_workspace_bytes(int m, int rows, int d, int L, int P);
int gpk_svgp_elbo_shard_lcm(void* stream, const int* family_host, const double* Z, int m, long ldz, long strideZ,
                            const double* Xb, const double* Yb, int rows, long ldxb, long ldyb, int d, int L, int P,
                            const double* W_host, const double* ls_host, int ard, const double* variance_host,
                            double noise_variance, double jitter, double mean_const, const double* q_mu, const double* q_sqrt,
                            double* out, int* info, void* ws, size_t ws_bytes);

/* ---- result mailbox in mapped host memory ------------------------------------------------------------------------
 * Copies n doubles from device memory `src` (and one int from `info`, may be NULL) into `host_dst`, a buffer of PINNED,
 * device-mapped host memory (hipHostMalloc / torch pin_memory) laid out as { double vals[n]; int32 info; int32 seq; },
 * then -- after a system-scope release -- writes `seq` last.  The caller spins on host_dst's `seq` word instead of
 * enqueueing device-to-host copies and synchronising the stream: the scalar of SVGP.elbo (svgp.py:181, read by
 * every optimiser step and by monitoring) lands in host memory a few microseconds after the last kernel of the step.
 * (Two blit copies + hipStreamSynchronize cost 90 - 150 us per step on MI355X, profiles/r03_step_timeline.txt.)
 * n <= 16.  One tiny kernel on `stream`; never synchronises. */
int gpk_publish_host(void* stream, const double* src, int n, const int* info, void* host_dst, int seq);

/* ---- the full variational GP (gpflow/models/vgp.py:36-180): product of two lower-triangular matrices ------------------------
 * With L [n, ldl] (the Cholesky factor of K(X, X) + jitter I) and S_r = S + r * stride_s [n, lds], r < R (the q_sqrt of the model),
 * both row-major and LOWER triangular, the product  P_r = L S_r  is lower triangular again,
 *     P_r[i, j] = sum_{k = j .. i} L[i, k] S_r[k, j]        (j <= i),
 * and the marginal variance of the model's q(f) is its row sum of squares (vgp.py:149-152 through conditionals/util.py:151-164 with
 * white = True and Lm = L):
 *     ssq[r, i] = sum_{j <= i} P_r[i, j]^2                   ssq [R, n], the `ssq` operand of gpk_*_varexp_sum.
 * Triangle: only entries with column <= row are READ, of L and of every S_r; what is stored above either diagonal (NaN, Inf,
 * garbage) never reaches a result -- the band_part(q_sqrt, -1, 0) of the reference, by construction.  A term of the sum above is
 * formed exactly when j <= k <= i: a NaN at L[i0, k0] reaches P_r[i0, j] for j <= k0 (and so ssq[r, i0] for every r) and nothing
 * else; a NaN at S_r[k0, j0] reaches P_r[i, j0] for i >= k0 (and so ssq[r, i] for i >= k0) and nothing else.
 * Outputs, each optional, at least one:
 *   ssq   [R, n] (with `parts`): the product is not stored;
 *   T     [R, n, ldt] (batch stride stride_t): T_r[i, j] = rowscale[r, i] * P_r[i, j] for j <= i (rowscale [R, n], may be NULL: 1);
 *         nothing is written above the diagonal or into the padding (ldt > n).  This is the seed of the reverse pass,
 *         T_bar = 2 diag(dF/dfvar) L S.
 * parts [R, gpk_tril_product_tiles(n), n]: scratch of the row sums -- entry [r, t, i] is the sum over the columns of tile column t
 *   (GPK_TRIL_TILE columns each) for t <= i / GPK_TRIL_TILE; the call writes every entry it later reads (its contents at entry do not
 *   matter), touches nothing outside that extent, and sums the tile columns in the order t = 0, 1, ...: no floating-point atomics,
 *   two calls on the same inputs give the same bits.  Needed with ssq, ignored (may be NULL) without.
 * One 128 x 128 output tile per workgroup, fp64 MFMA over the tile-block range j .. i only (n^3 / 3 multiply-adds per r; the
 * 16 x 16 blocks on the two diagonals by VALU under the exact predicate), the tiles with the longest K range first.
 * GPK_E_ARG before anything is enqueued: n < 0, R < 0, ldl / lds / ldt < n, L or S NULL, neither ssq nor T, ssq without parts,
 * rowscale without T.  n == 0 or R == 0: returns 0, nothing is enqueued or written. */
#define GPK_TRIL_TILE 128
int gpk_tril_product_tiles(int n);   /* ceil(n / GPK_TRIL_TILE) */
int gpk_tril_product(void* stream, const double* L, int n, long ldl, const double* S, long lds, long stride_s, int R,
                     double* ssq, double* parts, const double* rowscale, double* T, long ldt, long stride_t);

/* Optional per-launch timing of the GEMM kernel (HIP events on the launch stream) for the roofline
 * leg of bench.py: enable(1) starts recording, collect() synchronises and returns the summed kernel
 * time, launch count and ALGORITHMIC flops (useful multiply-adds only) since enable. */
void gpk_profile_gemm_enable(int on);
int gpk_profile_gemm_collect(double* total_ms, long* launches, double* flops);
/* same, restricted to launches with at least min_flops algorithmic flops; keep != 0 keeps the records */
int gpk_profile_gemm_collect_min(double min_flops, int keep, double* total_ms, long* launches, double* flops);
/* same, restricted to launches of ONE kernel -- kind 1 gemm_nt_small, 2 gemm_nt_fast<0,false>, 3 <0,true>, 4 <1,false>,
 * 5 <1,true>, 6 gemm_nt_kernel -- so that the HIP-event average can be compared with rocprofv3's per-kernel average;
 * records are kept */
int gpk_profile_gemm_collect_kind(int kind, double min_flops, double* total_ms, long* launches, double* flops);
/* phase spanned by the launches with >= min_flops (first start .. last end) and the algorithmic flops of ALL recorded
 * launches issued in between, on any stream: chip-wide rate of a phase in which several streams share the machine */
int gpk_profile_gemm_window(double min_flops, double* window_ms, double* flops_all, double* flops_matching,
                            long* launches_all);

/* micro-benchmarks used by bench.py / profiles (fp64 MFMA issue rate, HBM write stream) */
int gpk_bench_mfma_f64(void* stream, int blocks, int iters, double* sink);
int gpk_bench_stream_store(void* stream, double* out, long n_doubles);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GPK_H */
