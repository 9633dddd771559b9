// Covariance builder of the stationary families for WIDE inputs, 1 <= d <= GPK_WIDE_MAX_D columns (gpk_wide_kernel_matrix,
// gpk_wide_kernel_matrix_combine: include/gpk.h), gfx950.  rbf.hip stages both whole d-column slabs of a 64 x 64 tile in LDS and
// does its d products per element on the VALU: right for d ~ 1 .. 16, where the build is bound by its stores, and impossible past
// d = 64.  At d = 65 .. 1024 the build is a GEMM with a transcendental epilogue (2 d flops per element against 8 bytes written):
// this file puts the dot products on the fp64 matrix pipe and walks the columns in slabs.
//
// Work split.  One T x T output tile per 256-thread workgroup, T = 128 or 64; the four waves (2 x 2) own a square quarter each,
// WT = T / 2, as NB x NB blocks of v_mfma_f64_16x16x4_f64 (NB = WT / 16; A frag: row = lane & 15, k = lane >> 4, the B^T frag the
// same; D: col = lane & 15, row = (lane >> 4) + 4 reg -- gemm.hip).  T = 128 is the primary tile: 16 accumulators per wave and half
// the LDS traffic per MFMA of T = 64.  T = 64 is launched when the 128-tile grid would have fewer workgroups than the device has
// compute units (wide_tile below: a function of n1, n2 and the symmetric flag alone).
//
// K loop.  A slab is BK = 16 columns of both operands.  Thread t stages EPT = T / 16 consecutive columns of tile row t / TPR of each
// operand (TPR = 16 / EPT threads per row; 16-byte loads where the operand allows them), divides each by its lengthscale -- TRUE
// division, as rbf.hip and the reference, so r2 keeps the rounding structure of X / ls -- and writes the scaled values to LDS in the
// layout the MFMA fragments are read from.  Two LDS buffers: the global loads of slab s + 1 are issued before the MFMAs of slab s and
// written to the other buffer after them, one barrier per slab.  Columns past d are zero-filled with a divisor of 1.0, rows past
// n1 / n2 are zero-filled.
//
// LDS layout.  Both slabs are [T][16] with rows LD = 18 doubles apart (+ 2 doubles per 16-row group: lds_off), so the 32-lane groups
// of a fragment's ds_read_b64 hit distinct banks.  The ROWS are permuted at staging so that a lane's accumulators are neighbours in
// memory: tile row 16 i + 4 a + b of X1 sits in LDS row 16 i + a + 4 b (the D rows (lane >> 4) + 4 reg of a lane are then the four
// consecutive tile rows 16 i + 4 (lane >> 4) + reg), and column (lane & 15) NB + j of a wave's WT columns sits in LDS row 16 j +
// (lane & 15) of X2's slab (a lane's NB blocks are NB consecutive columns).  Direct and mirrored stores are then 16-byte stores.
//
// Norms.  The squared norm of every tile row and column is accumulated from the SCALED values as they are staged: the staging thread
// (row, column phase t % TPR) keeps one register partial per operand across the slabs, the partials meet in LDS after the last slab
// and are added in phase order.  The order depends on the column alone: a row's norm has the same bits as a row and as a column, in
// every tile, and a rerun is bit-identical.  No atomics.
//
// Epilogue, in the accumulator registers: r2 = (-2 dot) + (n_i + n_j) (rbf.hip's association), the profiles of kern_profile.h,
// diag_add / the COMB ops / the by-index zero diagonal / the NaN rule exactly as rbf_kernel has them.
//
// Symmetric build (X2 == NULL, plain build): only tiles on or below the diagonal run.  An off-diagonal tile is also written
// transposed unless lower_only; a diagonal tile writes its lower half and mirrors it inside the tile, so K == K^T holds by
// construction and does not rest on dot[i][j] and dot[j][i] leaving the matrix pipe with the same bits.
#include "../gpk_internal.h"
#include "../kern_profile.h"
#include <cmath>

namespace {

constexpr int BK = 16;   // columns per slab
constexpr int LD = 18;   // doubles between LDS rows of a slab

struct WideArgs {
  const double* X1; long ldx1; int n1;
  const double* X2; long ldx2; int n2;
  int d;
  double* K; long ldk;
  double variance, diag_add, alpha;
  int sym, lower_only, ard;
  const double* ls;           // DEVICE: d entries if ard, else one
  const double* G; long ldg;  // COMB instantiations only
  int comb_diag;              // COMB: X2 is X1 and diag_add goes onto the diagonal of the combined result
};

template <int T>
struct Geo {
  static constexpr int WT = T / 2, NB = WT / 16, EPT = T / 16, TPR = BK / EPT;
  static constexpr int SLAB = T * LD + 2 * (T / 16);    // doubles of one operand's slab (lds_off of the last row + its 16 columns)
  static constexpr size_t LDS = (size_t)4 * SLAB * sizeof(double);   // two operands, two buffers
  static_assert(2 * T * TPR + 2 * T <= 4 * SLAB, "the norm partials and the norms reuse the slabs");
};

__device__ __forceinline__ int lds_off(int lrow) { return lrow * LD + 2 * (lrow >> 4); }
// tile row of X1 -> LDS row: 16 i + 4 a + b -> 16 i + a + 4 b
__device__ __forceinline__ int lds_row_a(int r) { return (r & ~15) | ((r >> 2) & 3) | ((r & 3) << 2); }
// tile column (row of X2's slab) -> LDS row: wave half wc, c = l NB + j -> wc WT + 16 j + l
template <int T>
__device__ __forceinline__ int lds_row_b(int c) {
  constexpr int WT = Geo<T>::WT, NB = Geo<T>::NB;
  const int wc = c / WT, cc = c % WT;
  return wc * WT + (cc % NB) * 16 + cc / NB;
}

// COMB as rbf_kernel: 0 plain build; 1 / 2: out = G .* k / G + k; 3: G .* (-2 dk/dr2); 4 (GPK_KERN_RQ): G .* dk/dalpha.
// (two workgroups per CU: one's staging and epilogue under the other's MFMAs)
template <int T, int FAMILY, int COMB>
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ __launch_bounds__(256) void wide_kernel(const WideArgs p) {
  using G_ = Geo<T>;
  constexpr int WT = G_::WT, NB = G_::NB, EPT = G_::EPT, TPR = G_::TPR, SLAB = G_::SLAB;
  extern __shared__ __attribute__((aligned(16))) double sm[];   // [2 buffers][2 operands][SLAB]

  if (p.sym && blockIdx.x > blockIdx.y) return;   // strictly upper tile: skipped (lower_only) or written by its mirror
  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, l15 = lane & 15, lq = lane >> 4;
  const int d = p.d;

  // ---- staging slots --------------------------------------------------------------------------
  const int srow = tid / TPR, scol = (tid % TPR) * EPT;
  const int g1 = r0 + srow, g2 = c0 + srow;
  const double* __restrict__ x1 = p.X1 + (long)g1 * p.ldx1 + scol;
  const double* __restrict__ x2 = p.X2 + (long)g2 * p.ldx2 + scol;
  const bool in1 = g1 < p.n1, in2 = g2 < p.n2;
  const bool vec1 = in1 && ((p.ldx1 & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.X1) & 15) == 0);
  const bool vec2 = in2 && ((p.ldx2 & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.X2) & 15) == 0);
  const int so1 = lds_off(lds_row_a(srow)) + scol, so2 = SLAB + lds_off(lds_row_b<T>(srow)) + scol;
  const double l0 = p.ls[0];

  double ra[EPT], rb[EPT], rl[EPT];
  auto gload = [&](int ks) {
    const bool inside = ks + scol + EPT <= d;   // none of this thread's columns is past d
    if (vec1 && inside) {
#pragma unroll
      for (int e = 0; e < EPT; e += 2) {
        const d2 v = *reinterpret_cast<const d2*>(x1 + ks + e);
        ra[e] = v[0]; ra[e + 1] = v[1];
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) ra[e] = (in1 && ks + scol + e < d) ? x1[ks + e] : 0.0;
    }
    if (vec2 && inside) {
#pragma unroll
      for (int e = 0; e < EPT; e += 2) {
        const d2 v = *reinterpret_cast<const d2*>(x2 + ks + e);
        rb[e] = v[0]; rb[e + 1] = v[1];
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) rb[e] = (in2 && ks + scol + e < d) ? x2[ks + e] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) rl[e] = (ks + scol + e < d) ? (p.ard ? p.ls[ks + scol + e] : l0) : 1.0;
  };
  double nrm1 = 0.0, nrm2 = 0.0;   // this thread's share of |row srow|^2 of either operand, over its column phase of every slab
  auto lstore = [&](double* buf) {
#pragma unroll
    for (int e = 0; e < EPT; e += 2) {
      const double a0 = ra[e] / rl[e], a1 = ra[e + 1] / rl[e + 1];
      const double b0 = rb[e] / rl[e], b1 = rb[e + 1] / rl[e + 1];
      nrm1 = fma(a0, a0, nrm1); nrm1 = fma(a1, a1, nrm1);
      nrm2 = fma(b0, b0, nrm2); nrm2 = fma(b1, b1, nrm2);
      *reinterpret_cast<d2*>(&buf[so1 + e]) = (d2){a0, a1};
      *reinterpret_cast<d2*>(&buf[so2 + e]) = (d2){b0, b1};
    }
  };

  d4 acc[NB][NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  // MFMA fragments: block i of the wave's rows is LDS rows wr WT + 16 i .. + 15 of X1's slab, block j LDS rows wc WT + 16 j .. of X2's
  int fa[NB], fb[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    fa[i] = lds_off(wr * WT + i * 16 + l15) + lq;
    fb[i] = SLAB + lds_off(wc * WT + i * 16 + l15) + lq;
  }

  const int nslab = (d + BK - 1) / BK;
  gload(0);
  lstore(sm);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const double* cur = sm + (s & 1) * 2 * SLAB;
    const bool more = s + 1 < nslab;
    if (more) gload((s + 1) * BK);                     // in flight under this slab's arithmetic
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      double a[NB], b[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) a[i] = cur[fa[i] + kk * 4];
#pragma unroll
      for (int j = 0; j < NB; ++j) b[j] = cur[fb[j] + kk * 4];
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) lstore(sm + ((s + 1) & 1) * 2 * SLAB);   // (its last readers passed the barrier that ended slab s - 1)
    __syncthreads();
  }

  // ---- norms: partials in phase order (the slabs are no longer read) ---------------------------
  double* part = sm;                  // [2][T][TPR]
  double* nrm = sm + 2 * T * TPR;     // [2][T]: rows, then columns, by TILE index
  part[srow * TPR + (tid % TPR)] = nrm1;
  part[T * TPR + srow * TPR + (tid % TPR)] = nrm2;
  __syncthreads();
  if (tid < 2 * T) {
    double s = part[tid * TPR];
#pragma unroll
    for (int ph = 1; ph < TPR; ++ph) s += part[tid * TPR + ph];
    nrm[tid] = s;
  }
  __syncthreads();

  // ---- epilogue ----------------------------------------------------------------------------------
  const bool aligned = ((p.ldk & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.K) & 15) == 0);
  const bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && aligned;
  const bool mirror = p.sym && !p.lower_only;
  const bool diag_mirror = mirror && r0 == c0;   // the lower half and, inside the tile, its transpose
  const int tc0 = wc * WT + l15 * NB;            // this lane's NB consecutive tile columns
  double nj[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) nj[j] = nrm[T + tc0 + j];
  bool gvec = false;
  if constexpr (COMB != 0) gvec = full && ((p.ldg & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.G) & 15) == 0);

  // one row of this lane's block: the NB values of global row r0 + tr, accumulator row g of block row i
  auto row_values = [&](int i, int g, int tr, double* out) {
    const int gr = r0 + tr;
    const double ni = nrm[tr];
    double gv[NB];
    if constexpr (COMB != 0) {
      if (gvec) {
#pragma unroll
        for (int j = 0; j < NB; j += 2) {
          const d2 t = *reinterpret_cast<const d2*>(p.G + (long)gr * p.ldg + c0 + tc0 + j);
          gv[j] = t[0]; gv[j + 1] = t[1];
        }
      } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) gv[j] = (gr < p.n1 && c0 + tc0 + j < p.n2) ? p.G[(long)gr * p.ldg + c0 + tc0 + j] : 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int gc = c0 + tc0 + j;
      const double r2 = (-2.0 * acc[i][j][g]) + (ni + nj[j]);
      double k = (COMB == 4)   ? kern_dalpha_rq(r2, p.variance, p.alpha)
                 : (COMB == 3) ? kern_dr2<FAMILY>(r2, p.variance, p.alpha)
                               : kern_eval<FAMILY>(r2, p.variance, p.alpha);
      if (p.sym && gr == gc) k += p.diag_add;
      if constexpr (COMB != 0) {
        k = (COMB == 2) ? k + gv[j] : k * gv[j];
        if (p.comb_diag && gr == gc) k = (COMB >= 3) ? 0.0 : k + p.diag_add;
      }
      out[j] = k;
    }
  };
  auto store_row = [&](int gr, const double* v) {
    if (full) {
#pragma unroll
      for (int j = 0; j < NB; j += 2) *reinterpret_cast<d2*>(p.K + (long)gr * p.ldk + c0 + tc0 + j) = (d2){v[j], v[j + 1]};
    } else if (gr < p.n1) {
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (c0 + tc0 + j < p.n2) p.K[(long)gr * p.ldk + c0 + tc0 + j] = v[j];
    }
  };

#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int tr0 = wr * WT + i * 16 + 4 * lq;   // this lane's four consecutive tile rows of block row i
    if constexpr (COMB != 0) {   // no mirror (the combine ops sweep the full square): a row is stored as soon as it is formed
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        double v[NB];
        row_values(i, g, tr0 + g, v);
        store_row(r0 + tr0 + g, v);
      }
    } else {
      double v[4][NB];
#pragma unroll
      for (int g = 0; g < 4; ++g) row_values(i, g, tr0 + g, v[g]);
      if (diag_mirror) {   // element by element: (gr, gc) for gc <= gr, and its transpose
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int gr = r0 + tr0 + g;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const int gc = c0 + tc0 + j;
            if (gr < p.n1 && gc <= gr) {
              p.K[(long)gr * p.ldk + gc] = v[g][j];
              if (gc < gr) p.K[(long)gc * p.ldk + gr] = v[g][j];
            }
          }
        }
        continue;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) store_row(r0 + tr0 + g, v[g]);
      if (mirror && r0 != c0) {   // transposed copy: rows c0 + tc0 + j, columns r0 + tr0 .. + 3
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int gr = c0 + tc0 + j;
          if (full) {
            d2* out = reinterpret_cast<d2*>(p.K + (long)gr * p.ldk + r0 + tr0);
            out[0] = (d2){v[0][j], v[1][j]};
            out[1] = (d2){v[2][j], v[3][j]};
          } else if (gr < p.n1) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
              if (r0 + tr0 + g < p.n2) p.K[(long)gr * p.ldk + r0 + tr0 + g] = v[g][j];
          }
        }
      }
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------
// The tile: 128, unless the 128-tile grid would run fewer workgroups than the device has compute units.  A function of (n1, n2, sym)
// alone -- nothing else selects a kernel.
int wide_tile(int n1, int n2, bool sym, int cus) {
  const long nb1 = gpk_cdiv(n1, 128), nb2 = gpk_cdiv(n2, 128);
  const long tiles = sym ? nb1 * (nb1 + 1) / 2 : nb1 * nb2;
  return tiles < cus ? 64 : 128;
}

// (asked per call: the count belongs to the device that is current now, and the lookup is a cached attribute of the runtime)
int compute_units(int* cus) {
  int dev = 0, n = 0;
  GPK_HIP(hipGetDevice(&dev));
  GPK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  *cus = n > 0 ? n : 1;
  return 0;
}

template <int T, int FAMILY, int COMB>
int launch_tile(hipStream_t st, const WideArgs& a) {
  if (gpk_cdiv(a.n1, T) > 65535) return GPK_E_ARG;   // (grid.y: n1 <= 65535 T rows, include/gpk.h)
  static const hipError_t at = hipFuncSetAttribute(reinterpret_cast<const void*>(wide_kernel<T, FAMILY, COMB>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)Geo<T>::LDS);
  GPK_HIP(at);
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((wide_kernel<T, FAMILY, COMB>), grid, dim3(256), Geo<T>::LDS, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

template <int FAMILY, int COMB>
int launch_family(hipStream_t st, const WideArgs& a) {
  int cus = 0;
  GPK_TRY(compute_units(&cus));
  return wide_tile(a.n1, a.n2, a.sym != 0, cus) == 128 ? launch_tile<128, FAMILY, COMB>(st, a) : launch_tile<64, FAMILY, COMB>(st, a);
}

template <int COMB>
int launch_combine(hipStream_t st, int family, const WideArgs& a) {
  switch (family) {
    case GPK_KERN_SE: return launch_family<GPK_KERN_SE, COMB>(st, a);
    case GPK_KERN_MATERN12: return launch_family<GPK_KERN_MATERN12, COMB>(st, a);
    case GPK_KERN_MATERN32: return launch_family<GPK_KERN_MATERN32, COMB>(st, a);
    case GPK_KERN_MATERN52: return launch_family<GPK_KERN_MATERN52, COMB>(st, a);
    case GPK_KERN_EXPONENTIAL: return launch_family<GPK_KERN_EXPONENTIAL, COMB>(st, a);
    case GPK_KERN_RQ: return launch_family<GPK_KERN_RQ, COMB>(st, a);
  }
  return GPK_E_UNSUPPORTED;
}

// what both entry points answer before they look at op, G or K: 0 to go on, 1 for "nothing to do", or the refusal
int check_operands(WideArgs& a, int family, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d,
                   const double* ls_dev, int ard, double alpha, double variance) {
  if (!ls_dev || n1 < 0 || (X2 && n2 < 0) || d <= 0 || d > GPK_WIDE_MAX_D) return GPK_E_ARG;
  if (family < GPK_KERN_SE || family > GPK_KERN_RQ) return GPK_E_UNSUPPORTED;   // (White, Constant: gpk_kernel_matrix, they never read X)
  if (family == GPK_KERN_RQ && (!(alpha > 0.0) || !std::isfinite(alpha))) return GPK_E_ARG;
  if (n1 == 0 || (X2 && n2 == 0)) return 1;
  if (!X1 || (n1 > 1 && ldx1 < d) || (X2 && n2 > 1 && ldx2 < d)) return GPK_E_ARG;
  a.X1 = X1; a.ldx1 = ldx1; a.n1 = n1;
  a.X2 = X2 ? X2 : X1; a.ldx2 = X2 ? ldx2 : ldx1; a.n2 = X2 ? n2 : n1;
  a.d = d; a.ls = ls_dev; a.ard = ard;
  a.alpha = (family == GPK_KERN_RQ) ? alpha : 1.0;
  a.variance = variance;
  return 0;
}

}  // namespace

extern "C" int gpk_wide_kernel_matrix(void* stream, int family, const double* X1, int n1, long ldx1, const double* X2, int n2,
                                      long ldx2, int d, const double* ls_dev, int ard, double alpha, double variance,
                                      double diag_add, int lower_only, double* K, long ldk) {
  WideArgs a{};
  const int rc = check_operands(a, family, X1, n1, ldx1, X2, n2, ldx2, d, ls_dev, ard, alpha, variance);
  if (rc) return rc < 0 ? rc : 0;
  if (!K || (a.n1 > 1 && ldk < a.n2)) return GPK_E_ARG;
  a.K = K; a.ldk = ldk;
  a.sym = (X2 == nullptr);
  a.diag_add = diag_add; a.lower_only = lower_only;
  return launch_combine<0>((hipStream_t)stream, family, a);
}

extern "C" int gpk_wide_kernel_matrix_combine(void* stream, int family, int op, const double* X1, int n1, long ldx1,
                                              const double* X2, int n2, long ldx2, int d, const double* ls_dev, int ard,
                                              double alpha, double variance, double diag_add, const double* G, long ldg,
                                              double* out, long ldo) {
  WideArgs a{};
  const int rc = check_operands(a, family, X1, n1, ldx1, X2, n2, ldx2, d, ls_dev, ard, alpha, variance);
  if (rc < 0) return rc;
  if (op < 1 || op > 4) return GPK_E_ARG;
  if (op == 4 && family != GPK_KERN_RQ) return GPK_E_UNSUPPORTED;
  if (rc) return 0;
  if (!G || !out || (a.n1 > 1 && (ldg < a.n2 || ldo < a.n2))) return GPK_E_ARG;
  a.K = out; a.ldk = ldo; a.G = G; a.ldg = ldg;
  a.comb_diag = (X2 == nullptr);
  a.diag_add = a.comb_diag ? diag_add : 0.0;
  hipStream_t st = (hipStream_t)stream;
  if (op == 4) return launch_family<GPK_KERN_RQ, 4>(st, a);
  if (op == 3) return launch_combine<3>(st, family, a);
  return op == 1 ? launch_combine<1>(st, family, a) : launch_combine<2>(st, family, a);
}
