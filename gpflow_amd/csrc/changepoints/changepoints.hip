// The ChangePoints kernel (gpflow/kernels/changepoints.py): a combination that switches between T = C + 1 member kernels along ONE
// input column x, gfx950.
//
//   sig_j(x) = 1 / (1 + exp(-s_j (x - l_j)))        1 - sig_j(x) = 1 / (1 + exp(+s_j (x - l_j)))       j = 0 .. C-1, l sorted
//   a_i(x)   = sig_{i-1}(x) (1 - sig_i(x))          i = 0 .. C        (sig_{-1} = 1, 1 - sig_C = 1)
//   K(x, y)  = sum_i a_i(x) k_i(x, y) a_i(y)
//
// Contract (restated in include/gpk.h):
//  1. NO CANCELLATION.  1 - sig_j is its own reciprocal, never a subtraction: the far side of a change point goes to 0 smoothly.
//  2. SATURATION IS EXACT.  exp overflows to +Inf and underflows to 0, so a saturated sigmoid is exactly 1 or 0 and its member
//     contributes its full value or exactly nothing.
//  3. NaN / Inf.  z = s (x - l) + (x - x): the last term is 0.0 for a finite x (the sum is then s (x - l), one rounding) and NaN for a
//     NaN or an Inf, so such a row's weights are all NaN -- and with them exactly that row (column) of K.
//  4. SYMMETRY.  The tile kernels form w = a_r b_c FIRST and then w * Ki: with b == NULL (b is a) an exactly symmetric Ki stays
//     exactly symmetric.
//
// The weights are vectors of length n: the tile kernels are pure streaming passes over n1 x n2 matrices -- the pair tile of
// pair_tile.h (64 x 64 per 256-thread workgroup, 4 x 4 elements per thread) without its slabs: the tile's 64 + 64 weights are staged in
// LDS once.  Each matrix operand is read once and `out` written once; an element is read and written by the same thread, so `out` may
// alias an input.
#include "../pair_tile.h"
#include <cmath>

namespace {

using namespace pair_tile;
static_assert(T == GPK_CP_TILE, "include/gpk.h states the tile of the adjoint stage's partials");
constexpr int MAXC = GPK_CP_MAX_MEMBERS - 1;

struct CpPoints {
  int C;
  double loc[MAXC], steep[MAXC];
};

// sig_j and 1 - sig_j at x (contract 1 - 3); `poison` = x - x
__device__ __forceinline__ void cp_sigmoid(double x, double poison, double l, double s, double& sig, double& comp) {
  const double z = s * (x - l) + poison;
  sig = 1.0 / (1.0 + exp(-z));
  comp = 1.0 / (1.0 + exp(z));
}

// ---- the weights A [T, n]: one thread per row of the switch column ----------------------------------------------------------
struct CpWeightArgs {
  const double* x; long ldx; int n;
  double* A; long lda;
  CpPoints pt;
};

__global__ __launch_bounds__(256) void changepoint_weights_kernel(CpWeightArgs p) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= p.n) return;
  const double x = p.x[(long)r * p.ldx];
  const double poison = x - x;
  double prev = 1.0 + poison;   // sig_{-1}
  for (int j = 0; j < p.pt.C; ++j) {
    double sig, comp;
    cp_sigmoid(x, poison, p.pt.loc[j], p.pt.steep[j], sig, comp);
    p.A[(long)j * p.lda + r] = prev * comp;
    prev = sig;
  }
  p.A[(long)p.pt.C * p.lda + r] = prev;   // 1 - sig_C = 1
}

// ---- the tile pass ----------------------------------------------------------------------------------------------------------
// MODE 0: out = (a b^T) .* Ki.   1: out = Q + (a b^T) .* Ki (Q: acc).   2: the adjoint stage -- out = Q .* (a b^T) (Q: Kbar) and the
// tile's partial sums of Q Ki b_c (by row) and Q Ki a_r (by column).
struct CpTileArgs {
  const double* a; const double* b; int n1, n2;
  const double* Ki; long ldki;
  const double* Q; long ldq;
  double* out; long ldo;
  double diag_add; int sym;   // sym: b is a, diag_add goes onto the diagonal (MODE 0 / 1)
  double* parts; int tc;      // MODE 2
};

template <int MODE>
__global__ __launch_bounds__(256) void changepoint_tile_kernel(CpTileArgs p) {
  __shared__ double s_a[T], s_b[T];
  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  if (tid < T) {   // padding weights are 0.0: a padding element is 0 and never stored
    s_a[tid] = (r0 + tid < p.n1) ? p.a[r0 + tid] : 0.0;
  } else if (tid < 2 * T) {
    const int c = tid - T;
    s_b[c] = (c0 + c < p.n2) ? p.b[c0 + c] : 0.0;
  }
  __syncthreads();
  double ar[4], bc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ar[i] = s_a[ty * 4 + i];
    bc[i] = s_b[tx * 4 + i];
  }
  bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && (((p.ldki | p.ldo) & 1) == 0) &&
              (((reinterpret_cast<uintptr_t>(p.Ki) | reinterpret_cast<uintptr_t>(p.out)) & 15) == 0);
  if (MODE != 0) full = full && ((p.ldq & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.Q) & 15) == 0);

  double k[4][4], q[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
    if (full) {
      const d2* src = reinterpret_cast<const d2*>(p.Ki + (long)gr * p.ldki + c0 + tx * 4);
      const d2 k01 = src[0], k23 = src[1];
      k[i][0] = k01.x; k[i][1] = k01.y; k[i][2] = k23.x; k[i][3] = k23.y;
      if (MODE != 0) {
        const d2* qs = reinterpret_cast<const d2*>(p.Q + (long)gr * p.ldq + c0 + tx * 4);
        const d2 q01 = qs[0], q23 = qs[1];
        q[i][0] = q01.x; q[i][1] = q01.y; q[i][2] = q23.x; q[i][3] = q23.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gc = c0 + tx * 4 + j;
        const bool in = gr < p.n1 && gc < p.n2;
        k[i][j] = in ? p.Ki[(long)gr * p.ldki + gc] : 0.0;
        if (MODE != 0) q[i][j] = in ? p.Q[(long)gr * p.ldq + gc] : 0.0;
      }
    }
  }

  double v[4][4];
  double rs[4] = {0.0, 0.0, 0.0, 0.0}, cs[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = c0 + tx * 4 + j;
      const double w = ar[i] * bc[j];
      if constexpr (MODE == 2) {
        const bool in = gr < p.n1 && gc < p.n2;
        v[i][j] = q[i][j] * w;
        const double e = q[i][j] * k[i][j];
        rs[i] += in ? e * bc[j] : 0.0;   // (a padding element never enters a sum)
        cs[j] += in ? e * ar[i] : 0.0;
      } else {
        double o = w * k[i][j];
        if (MODE == 1) o = q[i][j] + o;
        if (p.sym && gr == gc) o += p.diag_add;
        v[i][j] = o;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
    if (full) {
      d2* out = reinterpret_cast<d2*>(p.out + (long)gr * p.ldo + c0 + tx * 4);
      out[0] = (d2){v[i][0], v[i][1]};
      out[1] = (d2){v[i][2], v[i][3]};
    } else if (gr < p.n1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gc = c0 + tx * 4 + j;
        if (gc < p.n2) p.out[(long)gr * p.ldo + gc] = v[i][j];
      }
    }
  }

  if constexpr (MODE == 2) {
    // The tile's partial sums, each by ONE thread in a fixed order: a thread's four elements left to right (above), then the sixteen
    // threads of a row (column) in ascending tx (ty).  Slots:
    //   parts[bx * n1 + r]              row r's sum over the columns of column tile bx
    //   parts[tc * n1 + by * n2 + c]    column c's sum over the rows of row tile by
    __shared__ double red_r[T * 16], red_c[T * 16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red_r[(ty * 4 + i) * 16 + tx] = rs[i];
      red_c[(tx * 4 + i) * 16 + ty] = cs[i];
    }
    __syncthreads();
    if (tid < 2 * T) {
      const int r = tid & (T - 1);
      const double* src = tid < T ? red_r : red_c;
      double acc = 0.0;
#pragma unroll
      for (int u = 0; u < 16; ++u) acc += src[r * 16 + u];
      if (tid < T) {
        if (r0 + r < p.n1) p.parts[(long)blockIdx.x * p.n1 + r0 + r] = acc;
      } else {
        if (c0 + r < p.n2) p.parts[(long)p.tc * p.n1 + (long)blockIdx.y * p.n2 + c0 + r] = acc;
      }
    }
  }
}

// ---- the adjoint tail -------------------------------------------------------------------------------------------------------
// Rows: one thread per row r of the switch column.  abar_i[r] = init_i[r] + sum_t parts_i[t n + r] (t ascending), then with
// tbar_j = abar_{j+1} a_{j+1} (1 - sig_j) - abar_j a_j sig_j:  xbar[r] = sum_j s_j tbar_j, and the workgroup's sums of tbar_j and of
// tbar_j (x - l_j) go to red[block (2 C) + j] and red[block (2 C) + C + j]: the 256 threads' terms meet in LDS, sixteen threads add
// sixteen each in thread order, thread 0 adds theirs.  Sum: ONE workgroup adds the blocks' entries of `red` in block order.
constexpr int TAIL_THREADS = 256;
struct CpTailArgs {
  const double* x; long ldx; int n;
  const double* parts; long member_stride; int ntiles;
  const double* init; long ldinit;
  double* red; int nblocks;
  double* dsmall; double* xbar;
  CpPoints pt;
};

__device__ __forceinline__ double cp_abar(const CpTailArgs& p, int i, int r) {
  double acc = p.init ? p.init[(long)i * p.ldinit + r] : 0.0;
  const double* src = p.parts + (long)i * p.member_stride + r;
  for (int t = 0; t < p.ntiles; ++t) acc += src[(long)t * p.n];
  return acc;
}

__global__ __launch_bounds__(TAIL_THREADS) void changepoint_tail_rows_kernel(CpTailArgs p) {
  __shared__ double sh_l[TAIL_THREADS], sh_s[TAIL_THREADS];
  const int t = threadIdx.x, r = blockIdx.x * TAIL_THREADS + t, C = p.pt.C;
  const bool in = r < p.n;
  const double x = in ? p.x[(long)r * p.ldx] : 0.0;
  const double poison = x - x;
  double sig_prev = 1.0 + poison, sig = 0.0, comp = 1.0, comp_next = 1.0;   // sig_{j-1}; sig_j, 1 - sig_j; 1 - sig_{j+1}
  if (C > 0) cp_sigmoid(x, poison, p.pt.loc[0], p.pt.steep[0], sig, comp);
  double ab = (in && C > 0) ? cp_abar(p, 0, r) : 0.0;   // abar_j
  double xb = 0.0;
  for (int j = 0; j < C; ++j) {
    double sig_next = 0.0;
    comp_next = 1.0;
    if (j + 1 < C) cp_sigmoid(x, poison, p.pt.loc[j + 1], p.pt.steep[j + 1], sig_next, comp_next);
    const double ab_next = in ? cp_abar(p, j + 1, r) : 0.0;
    const double a_j = sig_prev * comp, a_next = sig * comp_next;
    const double tb = in ? (ab_next * a_next) * comp - (ab * a_j) * sig : 0.0;
    xb += p.pt.steep[j] * tb;
    sh_l[t] = tb;
    sh_s[t] = in ? tb * (x - p.pt.loc[j]) : 0.0;
    __syncthreads();
    if (t < 32) {   // threads 0 .. 15: tbar; 16 .. 31: tbar (x - l)
      double* sh = t < 16 ? sh_l : sh_s;
      const int u = t & 15;
      double acc = 0.0;
      for (int q = 0; q < 16; ++q) acc += sh[u * 16 + q];
      sh[u * 16] = acc;   // (its own first entry, read by no other thread in this step)
    }
    __syncthreads();
    if (t == 0 || t == 16) {
      const double* sh = t == 0 ? sh_l : sh_s;
      double acc = 0.0;
      for (int q = 0; q < 16; ++q) acc += sh[q * 16];
      p.red[(long)blockIdx.x * 2 * C + (t == 0 ? j : C + j)] = acc;
    }
    __syncthreads();
    sig_prev = sig; sig = sig_next; comp = comp_next; ab = ab_next;
  }
  if (in) p.xbar[r] = xb;
}

__global__ __launch_bounds__(64) void changepoint_tail_sum_kernel(CpTailArgs p) {
  const int q = threadIdx.x, C = p.pt.C;
  if (q >= 2 * C) return;
  double acc = 0.0;
  for (int b = 0; b < p.nblocks; ++b) acc += p.red[(long)b * 2 * C + q];
  const int j = q < C ? q : q - C;
  p.dsmall[q] = q < C ? -p.pt.steep[j] * acc : acc;
}

// what every entry point checks of the change points before it looks at the operands
int read_points(CpPoints& pt, int C, const double* loc_host, const double* steep_host) {
  if (C < 0) return GPK_E_ARG;
  if (C > MAXC) return GPK_E_UNSUPPORTED;
  if (C > 0 && (!loc_host || !steep_host)) return GPK_E_ARG;
  pt.C = C;
  for (int j = 0; j < MAXC; ++j) {
    pt.loc[j] = 0.0;
    pt.steep[j] = 1.0;
  }
  for (int j = 0; j < C; ++j) {
    if (!std::isfinite(loc_host[j]) || !std::isfinite(steep_host[j]) || !(steep_host[j] > 0.0)) return GPK_E_ARG;
    if (j > 0 && loc_host[j] < loc_host[j - 1]) return GPK_E_ARG;   // sorted on the host
    pt.loc[j] = loc_host[j];
    pt.steep[j] = steep_host[j];
  }
  return 0;
}

template <int MODE>
int launch_tile(hipStream_t st, const CpTileArgs& a) {
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((changepoint_tile_kernel<MODE>), grid, dim3(256), 0, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" int gpk_changepoint_weights(void* stream, const double* x, int n, long ldx, int C, const double* loc_host,
                                       const double* steep_host, double* A, long lda) {
  CpWeightArgs a{};
  GPK_TRY(read_points(a.pt, C, loc_host, steep_host));
  if (n < 0 || ldx < 1 || lda < n) return GPK_E_ARG;
  if (n == 0) return 0;
  if (!x || !A) return GPK_E_ARG;
  a.x = x; a.ldx = ldx; a.n = n; a.A = A; a.lda = lda;
  const dim3 grid((unsigned)gpk_cdiv(n, 256));
  hipLaunchKernelGGL(changepoint_weights_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_changepoint_fold(void* stream, int op, const double* a, const double* b, int n1, int n2, const double* Ki, long ldki,
                                    const double* acc, long ldacc, double diag_add, double* out, long ldo) {
  if (op < 0 || op > 1 || n1 < 0 || (b && n2 < 0)) return GPK_E_ARG;
  const int m2 = b ? n2 : n1;
  if (ldki < m2 || ldo < m2 || (op == 1 && ldacc < m2)) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;
  if (!a || !Ki || !out || (op == 1 && !acc)) return GPK_E_ARG;
  CpTileArgs t{};
  t.a = a; t.b = b ? b : a; t.n1 = n1; t.n2 = m2; t.Ki = Ki; t.ldki = ldki; t.Q = acc; t.ldq = ldacc; t.out = out; t.ldo = ldo;
  t.sym = (b == nullptr); t.diag_add = t.sym ? diag_add : 0.0;
  return op == 0 ? launch_tile<0>((hipStream_t)stream, t) : launch_tile<1>((hipStream_t)stream, t);
}

extern "C" int gpk_changepoint_adjoint_stage(void* stream, const double* a, const double* b, int n1, int n2, const double* Kbar, long ldkb,
                                             const double* Ki, long ldki, double* G, long ldg, double* parts) {
  if (n1 < 0 || (b && n2 < 0)) return GPK_E_ARG;
  const int m2 = b ? n2 : n1;
  if (ldkb < m2 || ldki < m2 || ldg < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;
  if (!a || !Kbar || !Ki || !G || !parts) return GPK_E_ARG;
  CpTileArgs t{};
  t.a = a; t.b = b ? b : a; t.n1 = n1; t.n2 = m2; t.Ki = Ki; t.ldki = ldki; t.Q = Kbar; t.ldq = ldkb; t.out = G; t.ldo = ldg;
  t.parts = parts; t.tc = gpk_cdiv(m2, T);
  return launch_tile<2>((hipStream_t)stream, t);
}

extern "C" int gpk_changepoint_adjoint_tail(void* stream, const double* x, int n, long ldx, int C, const double* loc_host,
                                            const double* steep_host, const double* parts, long member_stride, int ntiles,
                                            const double* init, long ldinit, double* red, double* dsmall, double* xbar) {
  CpTailArgs a{};
  GPK_TRY(read_points(a.pt, C, loc_host, steep_host));
  if (n < 0 || ldx < 1 || ntiles < 0 || (ntiles > 0 && member_stride < (long)ntiles * n) || (init && ldinit < n)) return GPK_E_ARG;
  if (n == 0 || C == 0) return 0;   // no row, or no change point: nothing depends on the locations (xbar is not written)
  if (!x || !red || !dsmall || !xbar || (ntiles > 0 && !parts)) return GPK_E_ARG;
  a.x = x; a.ldx = ldx; a.n = n; a.parts = parts; a.member_stride = member_stride; a.ntiles = ntiles; a.init = init; a.ldinit = ldinit;
  a.red = red; a.nblocks = gpk_cdiv(n, TAIL_THREADS); a.dsmall = dsmall; a.xbar = xbar;
  const dim3 grid((unsigned)gpk_cdiv(n, TAIL_THREADS));
  hipLaunchKernelGGL(changepoint_tail_rows_kernel, grid, dim3(TAIL_THREADS), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(changepoint_tail_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}
