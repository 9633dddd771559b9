// Device code of the round 1 - 5 leaf (description at the top of leaf.hip), reduced to what the library uses it for: the inverse of
// the 128 x 128 diagonal block of an EXISTING factor (leaf_kernel<true>), and the tile helpers that the round-6 leaf (leaf2_device.h)
// shares with it.  Its Cholesky arithmetic went with the A/B-only kernels that ran it: DESIGN 6, "Closed experiments whose code was
// removed".
#pragma once
#include "gpk_internal.h"

namespace gpk_leaf {

constexpr int NB = GPK_NB;
constexpr int LD = NB + 2;     // 130: A-layout fragment reads hit 64 distinct banks
constexpr int SB = 16;         // sub-block
constexpr int NSB = NB / SB;   // 8
constexpr int XLD = SB + 1;    // row stride of the dense diagonal tiles of X
constexpr int NT = 512;        // 8 waves
constexpr int NW = NT / 64;
constexpr int XD_OFF = NB * LD;                  // doubles: [NSB][SB][XLD]
constexpr int LDS_DOUBLES = XD_OFF + NSB * SB * XLD;
constexpr size_t LEAF_LDS = (size_t)LDS_DOUBLES * sizeof(double);

__device__ __forceinline__ double readlane_d(double v, int lane) {
  union { double d; int i[2]; } u;
  u.d = v;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], lane);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], lane);
  return u.d;
}

// 1/sqrt(p): v_rsq_f64 (2^-23 relative) + ONE third-order step  y (1 + e/2 + 3e^2/8),  e = 1 - p y^2
// (error 5/16 e^3 ~ 2^-70).  Five dependent fp64 ops instead of the seven of two Newton steps: the
// dependent-issue latency of fp64 VALU ops (~38 cycles) times the 128 pivots IS the leaf's critical path.
__device__ __forceinline__ double rsqrt_nr(double p) {
  const double y = __builtin_amdgcn_rsq(p);
  const double t = p * y;
  const double e = fma(-t, y, 1.0);
  const double q = fma(0.375, e, 0.5);
  const double s = y * e;
  return fma(s, q, y);
}

__device__ __forceinline__ d4 mfma4(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// ---- 16x16 diagonal tile of an existing factor: its inverse in the registers of one wave ---------------------
// c = lane & 15, g = lane >> 4.  On entry d[e] = L[c][4e+g] (zero above the diagonal).  On exit x[e] = X[4e+g][c]
// (X = L^-1, exact zeros above the diagonal).
template <int P>
__device__ __forceinline__ void diag_panel(const d4& d, d4& x, int c, int g) {
  if constexpr (P < 4) {
    // 4x4 pivot block  s[a][b] = L[4P+a][4P+b]  (a >= b), wave-uniform: d[P] of lane (c = 4P+a, g = b)
    auto pick = [&](int a, int b) -> double { return readlane_d(d[P], 4 * P + a + 16 * b); };
    const double s00 = pick(0, 0), s10 = pick(1, 0), s20 = pick(2, 0), s30 = pick(3, 0);
    const double s11 = pick(1, 1), s21 = pick(2, 1), s31 = pick(3, 1);
    const double s22 = pick(2, 2), s32 = pick(3, 2), s33 = pick(3, 3);
    const int slot = (c < 4 && g <= c) ? c * 4 + g : -1;  // lane (m = c, k = g) holds Y[m][k] of the A-operand
    const double l10 = s10, l20 = s20, l30 = s30, l21 = s21, l31 = s31, l32 = s32;
    const double r0 = 1.0 / s00, r1 = 1.0 / s11, r2 = 1.0 / s22, r3 = 1.0 / s33;
    // Y = inv(L4), lower triangular
    const double y10 = -r1 * (l10 * r0);
    const double y21 = -r2 * (l21 * r1);
    const double y32 = -r3 * (l32 * r2);
    const double y20 = -r2 * fma(l21, y10, l20 * r0);
    const double y31 = -r3 * fma(l32, y21, l31 * r1);
    const double y30 = -r3 * fma(l32, y20, fma(l31, y10, l30 * r0));
    // flat select chain on the per-lane slot index (no divergent control flow: every Y value is wave-uniform)
    double yop = 0.0;
    yop = (slot == 0) ? r0 : yop;
    yop = (slot == 4) ? y10 : yop;
    yop = (slot == 5) ? r1 : yop;
    yop = (slot == 8) ? y20 : yop;
    yop = (slot == 9) ? y21 : yop;
    yop = (slot == 10) ? r2 : yop;
    yop = (slot == 12) ? y30 : yop;
    yop = (slot == 13) ? y31 : yop;
    yop = (slot == 14) ? y32 : yop;
    yop = (slot == 15) ? r3 : yop;
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    const double lp = d[P];   // panel of L: reg P of lane (n, g) = L[n][4P+g]
    // new rows of X:  Xp[m][n] = sum_k Y[m][k] Xtmp[4P+k][n]  ->  reg 0 of lane (n, g) = X[4P+g][n]
    const d4 u = mfma4(yop, x[P], zero);
    const double xp = u[0];
    if constexpr (P < 3) x = mfma4(-lp, xp, x);  // Xtmp[m][:] -= L[m][4P+k] X[4P+k][:]
    x[P] = xp;
    diag_panel<P + 1>(d, x, c, g);
  }
}

__device__ __forceinline__ void diag16(double* __restrict__ S, int k, int lane) {
  const int c = lane & 15, g = lane >> 4;
  const int kb = k * SB;
  d4 d, x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = g + 4 * e;  // the other index
    d[e] = (c >= j) ? S[(kb + c) * LD + kb + j] : 0.0;           // L[c][4e+g]
    x[e] = (j == c) ? 1.0 : 0.0;
  }
  diag_panel<0>(d, x, c, g);
  double* __restrict__ Xd = S + XD_OFF + k * (SB * XLD);
#pragma unroll
  for (int e = 0; e < 4; ++e) Xd[(4 * e + g) * XLD + c] = x[e];   // X[j][c]
}

// ---- 16x16 tile products on LDS-resident operands --------------------------------------------------------
// A tile reference: element (r, q) lives at S[base + r * rs + q * cs].
struct TRef { int base, rs, cs; };
__device__ __forceinline__ TRef tile_L(int i, int j) { return {i * SB * LD + j * SB, LD, 1}; }       // L_ij[r][q]
__device__ __forceinline__ TRef tile_X(int i, int j) { return {j * SB * LD + i * SB, 1, LD}; }       // X_ij (i>j), stored transposed
__device__ __forceinline__ TRef tile_Xd(int k) { return {XD_OFF + k * SB * XLD, XLD, 1}; }          // X_kk dense
__device__ __forceinline__ TRef tr(TRef t) { return {t.base, t.cs, t.rs}; }                          // transposed view

struct Frag { double a[4], b[4]; };
// operands of  D[m][n] += sum_q A[m][q] * B[n][q]   (NT form; pass tr(B) for a plain product)
__device__ __forceinline__ void frag_load(const double* __restrict__ S, TRef A, TRef B, int lane, Frag& f) {
  const int r = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    f.a[kk] = S[A.base + r * A.rs + (4 * kk + kq) * A.cs];
    f.b[kk] = S[B.base + r * B.rs + (4 * kk + kq) * B.cs];
  }
}
template <bool NEG>
__device__ __forceinline__ d4 frag_mma(const Frag& f, d4 acc) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) acc = mfma4(NEG ? -f.a[kk] : f.a[kk], f.b[kk], acc);
  return acc;
}
__device__ __forceinline__ d4 tile_load(const double* __restrict__ S, TRef C, int lane) {
  const int c = lane & 15, g = lane >> 4;
  d4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = S[C.base + (g + 4 * e) * C.rs + c * C.cs];
  return v;
}
__device__ __forceinline__ void tile_store(double* __restrict__ S, TRef C, int lane, d4 v) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) S[C.base + (g + 4 * e) * C.rs + c * C.cs] = v[e];
}
// second factor already in registers in D layout (T[q][n]: lane (n, g) reg kk = T[4kk+g][n]):
//   D[m][n] += sum_q A[m][q] * T[q][n]
template <bool NEG>
__device__ __forceinline__ d4 reg_mma(const double* __restrict__ S, TRef A, d4 t, int lane, d4 acc) {
  const int r = lane & 15, kq = lane >> 4;
  double a[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) a[kk] = S[A.base + r * A.rs + (4 * kk + kq) * A.cs];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) acc = mfma4(NEG ? -a[kk] : a[kk], t[kk], acc);
  return acc;
}

// ---- pieces of the recursive-doubling assembly of X = L^-1 (X21 = -X22 (L21 X11) at block sizes 16, 32, 64) ------
// level 1, node p: tile (2p+1, 2p); one wave, the intermediate T stays in registers
__device__ __forceinline__ void inv_level1(double* __restrict__ S, int p, int lane) {
  Frag f;
  frag_load(S, tile_L(2 * p + 1, 2 * p), tr(tile_Xd(2 * p)), lane, f);            // T = L21 X11
  const d4 t = frag_mma<false>(f, (d4){0.0, 0.0, 0.0, 0.0});
  const d4 r = reg_mma<true>(S, tile_Xd(2 * p + 1), t, lane, (d4){0.0, 0.0, 0.0, 0.0});  // -X22 T
  tile_store(S, tile_X(2 * p + 1, 2 * p), lane, r);
}
// level 2, node q (blocks 4q..4q+3): tile X21(a, b), one wave per (b, a)
__device__ __forceinline__ void inv_level2(double* __restrict__ S, int q, int b, int a, int lane) {
  const int r0 = 4 * q + 2, c0 = 4 * q;  // tile coordinates of the node's L21 / X21 block
  // T(t, b) = sum_{s >= b} L21(t, s) X11(s, b),  t = 0..a   (X11(s,b): s == b diagonal tile, s > b off-diagonal)
  d4 t0 = {0.0, 0.0, 0.0, 0.0}, t1 = {0.0, 0.0, 0.0, 0.0};
  for (int s2 = b; s2 < 2; ++s2) {
    const TRef xs = (s2 == b) ? tile_Xd(c0 + b) : tile_X(c0 + s2, c0 + b);
    Frag f;
    frag_load(S, tile_L(r0, c0 + s2), tr(xs), lane, f);
    t0 = frag_mma<false>(f, t0);
    if (a == 1) {
      frag_load(S, tile_L(r0 + 1, c0 + s2), tr(xs), lane, f);
      t1 = frag_mma<false>(f, t1);
    }
  }
  // X21(a, b) = -sum_{t <= a} X22(a, t) T(t, b)
  d4 r = {0.0, 0.0, 0.0, 0.0};
  if (a == 0) {
    r = reg_mma<true>(S, tile_Xd(r0), t0, lane, r);
  } else {
    r = reg_mma<true>(S, tile_X(r0 + 1, r0), t0, lane, r);
    r = reg_mma<true>(S, tile_Xd(r0 + 1), t1, lane, r);
  }
  tile_store(S, tile_X(r0 + a, c0 + b), lane, r);
}
// level 3, phase 1: T(t, b) = sum_{s=b}^{3} L(4+t, s) X(s, b), parked (transposed, like X) in the X21 region
__device__ __forceinline__ void inv_level3_T(double* __restrict__ S, int t, int b, int lane) {
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int s2 = b; s2 < 4; ++s2) {
    const TRef xs = (s2 == b) ? tile_Xd(b) : tile_X(s2, b);
    Frag f;
    frag_load(S, tile_L(4 + t, s2), tr(xs), lane, f);
    acc = frag_mma<false>(f, acc);
  }
  tile_store(S, tile_X(4 + t, b), lane, acc);
}
// level 3, phase 2: X21(a, b) = -sum_{t=0}^{a} X22(a, t) T(t, b)   (result returned, stored after a barrier)
__device__ __forceinline__ d4 inv_level3_X(const double* __restrict__ S, int a, int b, int lane) {
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int t = 0; t <= a; ++t) {
    const TRef xa = (t == a) ? tile_Xd(4 + a) : tile_X(4 + a, 4 + t);
    Frag f;
    frag_load(S, xa, tr(tile_X(4 + t, b)), lane, f);
    acc = frag_mma<true>(f, acc);
  }
  return acc;
}

// The inverse as a device function (one workgroup of NT threads, LDS block S of LEAF_LDS bytes): A is never written.
__device__ __forceinline__ void leaf_body(double* __restrict__ S, const double* __restrict__ A, long lda, int nb,
                                          double* __restrict__ inv) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nsb = (nb + SB - 1) / SB;

  // ---- load: lower triangle of A (identity beyond nb), zero strict upper; all loads issued up front ----
  {
    // thread t owns the column pair (2 (t & 63), +1) of rows (t >> 6) + 8 it
    const int jp = 2 * (tid & 63), r0 = tid >> 6;
    const bool vec = ((lda & 1) == 0) && ((reinterpret_cast<uintptr_t>(A) & 15) == 0);
    constexpr int NIT = NB / NW;
    d2 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = r0 + NW * it;
      v[it] = (d2){0.0, 0.0};
      if (i < nb && jp <= i) {
        const double* src = A + (long)i * lda + jp;
        if (vec && jp + 1 < nb) v[it] = *reinterpret_cast<const d2*>(src);
        else { v[it].x = src[0]; if (jp + 1 < nb) v[it].y = src[1]; }
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = r0 + NW * it;
      d2 w = v[it];
      if (jp > i) w.x = 0.0; else if (i >= nb) w.x = (jp == i) ? 1.0 : 0.0;
      if (jp + 1 > i) w.y = 0.0; else if (i >= nb) w.y = (jp + 1 == i) ? 1.0 : 0.0;
      *reinterpret_cast<d2*>(&S[i * LD + jp]) = w;
    }
    // diagonal tiles of X beyond the factored range are the identity
    for (int e = tid; e < NSB * SB * XLD; e += NT) {
      const int r = (e / XLD) % SB, q = e % XLD;
      S[XD_OFF + e] = (r == q) ? 1.0 : 0.0;
    }
  }
  __syncthreads();

  if (wave < nsb) diag16(S, wave, lane);
  __syncthreads();

  // ---- off-diagonal tiles of X by recursive doubling:  X21 = -X22 (L21 X11) ----------------------------------
  if (wave < 4) inv_level1(S, wave, lane);
  __syncthreads();
  inv_level2(S, wave >> 2, (wave >> 1) & 1, wave & 1, lane);
  __syncthreads();
  // level 3 phase 1: 16 T tiles, two per wave
#pragma unroll
  for (int h = 0; h < 2; ++h) inv_level3_T(S, 2 * (wave & 1) + h, wave >> 1, lane);
  __syncthreads();
  {
    // level 3 phase 2: 16 tiles, two per wave, pairing heavy with light rows: wave -> b = wave>>1, a in (1,2) or (0,3)
    d4 rr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int b = wave >> 1;
      const int a = (wave & 1) ? (1 + h) : (3 * h);
      rr[h] = inv_level3_X(S, a, b, lane);
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int b = wave >> 1;
      const int a = (wave & 1) ? (1 + h) : (3 * h);
      tile_store(S, tile_X(4 + a, b), lane, rr[h]);
    }
  }
  __syncthreads();

  // ---- write the inverse block ------------------------------------------------------------------------
  {
    const int jp = 2 * (tid & 63), r0 = tid >> 6;
    constexpr int NIT = NB / NW;
    const double* __restrict__ Xd = S + XD_OFF;
#pragma unroll 4
    for (int it = 0; it < NIT; ++it) {
      const int i = r0 + NW * it;
      auto xval = [&](int j) -> double {
        if (j > i) return 0.0;
        if ((j >> 4) == (i >> 4)) return Xd[(i >> 4) * (SB * XLD) + (i & 15) * XLD + (j & 15)];
        return S[j * LD + i];
      };
      d2 xv;
      xv.x = xval(jp);
      xv.y = xval(jp + 1);
      *reinterpret_cast<d2*>(&inv[i * NB + jp]) = xv;
    }
  }
}

}  // namespace gpk_leaf
