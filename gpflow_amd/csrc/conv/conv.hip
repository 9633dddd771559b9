// The Convolutional kernel over inducing patches (gpflow/kernels/convolutional.py, covariances/kufs.py, InducingPatches), gfx950.
//
// An input row is an image [H, W, C], channel fastest; a patch is an h x w window of ONE channel (stride 1, no padding), P = C oh ow of
// them per image (oh = H - h + 1, ow = W - w + 1), ordered by channel, window row, window column.  With the base kernel
// k(a, b) = v exp(-|a - b|^2 / (2 l^2)) and the patch weights w [P]:
//     Kfu[n, m]  = (1 / P)   sum_p     w_p      k(z_m, x_n^[p])
//     K_diag[n]  = (1 / P^2) sum_{p,q} w_p w_q  k(x_n^[p], x_n^[q])          (p == q by index: k = v, no distance formed)
//
// Patches are never written anywhere.  A workgroup stages ONE image in LDS, divided by l, and addresses patch element (p, k) inside it
// as base(p) + off(k): base(p) = ((i W) + j) C + c from the patch's (channel, window row, window column), off(k) = ((di W) + dj) C from
// the element's place in the window -- a table of patch_len entries in LDS, built once per workgroup.
//
// The dot products are v_mfma_f64_16x16x4_f64 tiles (A fragment: row = lane & 15, k = lane >> 4; B fragment: column = lane & 15,
// k = lane >> 4; D: column = lane & 15, row = (lane >> 4) + 4 reg).  The B operand -- sixteen patches -- is GATHERED from the LDS image,
// one ds_read_b64 per lane and k step, patch_len zero-padded to a multiple of 4 by selects (a padding lane reads a clamped, valid
// address and contributes an exact zero).  The same gathered values give the patch norms: each lane squares what it feeds the matrix
// pipe, two butterfly steps over the four k groups finish |x^[p]|^2 in the lane that owns column p.
//   Kfu      256 threads = 4 waves own one image and 64 inducing patches, 16 per wave, whose A fragments (z / l) stay in REGISTERS for
//            the whole sweep over the image's P patches.  Per 16-patch tile: patch_len / 4 MFMAs, then r2 = (|z|^2 + |x|^2) - 2 z.x,
//            exp, times w_p, added into four registers per lane (one per output row); after the sweep four butterfly steps over the
//            sixteen columns, one scale by v / P, one store per output element.
//   K_diag   one workgroup per image; the tiles with q <= p of the P x P patch Gram are dealt round-robin to the 4 waves, BOTH
//            operands gathered from LDS.  Off-diagonal pairs count twice, p == q is w_p^2 by index.  One value per image: lane sums,
//            six butterfly steps, the four waves in wave order.
//   adjoints recompute stages with typed partials and a one-launch tail (below).  No atomics anywhere: a second call gives the same bits.
//
// NaN / Inf: an image is only ever read by the workgroup(s) that own it, and every pixel lies in at least one patch, whose norm is then
// not finite: exactly the rows of Kfu and the entries of K_diag of that image are non-finite (every Kfu term and the by-index diagonal
// carry |x|^2 - |x|^2, 0.0 for a finite patch: an Inf pixel under negative z would otherwise give r2 = +Inf and exp = 0).  No fmax / fmin: r2 is not clamped (rbf.hip: the SquaredExponential takes r2 as it comes).
#include "../gpk_internal.h"
#include <cmath>

namespace {

constexpr int MBLK = 64;                 // inducing patches per workgroup (16 per wave)
constexpr int MAXNK = GPK_MAX_D / 4;     // k steps of one dot product
constexpr int GT_LD = 17;                // row stride of a wave's 16 x 16 seed tile in LDS
constexpr int KFU_ADJ_CHUNKS = 32;       // image chunks of the Kfu adjoint (its dZ partials are [chunks, M, patch_len4])
constexpr int KDIAG_ADJ_CHUNKS = 128;    // image chunks of the K_diag adjoint
static_assert(MBLK == GPK_CONV_MBLOCK, "include/gpk.h states the M block");

__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }

struct Geom {
  int W, C, w, oh, ow, P, plen, nk, npix;   // nk = ceil(plen / 4)
};

struct ConvArgs {
  Geom g;
  const double* X; long ldx; int N;
  const double* Z; long ldz; int M;
  const double* wts;
  double ls, variance;
  double* out; long ldo;                // Kfu [N, M] / K_diag [N]
  const double* G; long ldg;            // Kfu adjoint: dF/dKfu [N, M];  K_diag adjoint: c [N]
  int nchunk;
  double *pZ, *psg, *pw, *ps;           // partials (see the adjoint kernels)
  double *dsmall, *dZ, *dw; long lddz;  // tail outputs
  int nwg;
};

__device__ __forceinline__ int patch_base(const Geom& g, int p) {
  const int per = g.oh * g.ow;
  const int c = p / per, r = p - c * per;
  const int i = r / g.ow, j = r - i * g.ow;
  return (i * g.W + j) * g.C + c;
}

// image n -> LDS, divided by the lengthscale (true division, as rbf.hip); the offset table: -1 marks the zero padding of patch_len
__device__ __forceinline__ void stage_image(const ConvArgs& p, int n, double* img) {
  const double* src = p.X + (long)n * p.ldx;
  for (int e = threadIdx.x; e < p.g.npix; e += 256) img[e] = src[e] / p.ls;
}
__device__ __forceinline__ void stage_offsets(const Geom& g, int* off) {
  const int k = threadIdx.x;
  if (k < GPK_MAX_D) off[k] = k < g.plen ? ((k / g.w) * g.W + (k % g.w)) * g.C : -1;
}

// element k of patch p (p < P is `valid`; the address is in bounds either way)
__device__ __forceinline__ double patch_elem(const double* img, int base, bool valid, int o) {
  const double v = img[base + (o < 0 ? 0 : o)];
  return (valid && o >= 0) ? v : 0.0;
}

__device__ __forceinline__ double group_sum(double x) {   // over the four k groups (lane >> 4): the sum lands in all four
  x += __shfl_xor(x, 16);
  x += __shfl_xor(x, 32);
  return x;
}
__device__ __forceinline__ double column_sum(double x) {  // over the sixteen columns (lane & 15)
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 8);
  return x;
}

// this wave's sixteen inducing patches as A fragments a[kk] (row = lane & 15, k = 4 kk + (lane >> 4)), divided by l; zr[r] = |z|^2 of D row r
__device__ __forceinline__ void load_z(const ConvArgs& p, int m0, int lane, double (&a)[MAXNK], double (&zr)[4]) {
  const int row = m0 + (lane & 15), grp = lane >> 4;
  double zn = 0.0;
#pragma unroll
  for (int kk = 0; kk < MAXNK; ++kk) {
    a[kk] = 0.0;
    if (kk < p.g.nk) {
      const int k = 4 * kk + grp;
      if (row < p.M && k < p.g.plen) a[kk] = p.Z[(long)row * p.ldz + k] / p.ls;
      zn = fma(a[kk], a[kk], zn);
    }
  }
  zn = group_sum(zn);
#pragma unroll
  for (int r = 0; r < 4; ++r) zr[r] = __shfl(zn, grp + 4 * r);
}

// one 16 x 16 tile of z . x: the sixteen patches from p0 gathered from LDS; returns their squared norm for this lane's column
__device__ __forceinline__ double dot_tile(const Geom& g, const double* img, const int* off, const double (&a)[MAXNK], int p0, int lane,
                                           d4& d) {
  const int pc = p0 + (lane & 15), grp = lane >> 4;
  const bool valid = pc < g.P;
  const int base = patch_base(g, valid ? pc : g.P - 1);
  double xn = 0.0;
  d = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < MAXNK; ++kk) {
    if (kk < g.nk) {
      const double b = patch_elem(img, base, valid, off[4 * kk + grp]);
      xn = fma(b, b, xn);
      d = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b, d, 0, 0, 0);
    }
  }
  return group_sum(xn);
}

// ---- Kfu ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_kfu_kernel(ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* img = sm;
  int* off = reinterpret_cast<int*>(sm + p.g.npix);
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.y * MBLK + wave * 16;
  stage_image(p, n, img);
  stage_offsets(p.g, off);
  __syncthreads();
  if (m0 >= p.M) return;   // (no barrier below)
  double a[MAXNK], zr[4], acc[4] = {0.0, 0.0, 0.0, 0.0};
  load_z(p, m0, lane, a, zr);
  for (int p0 = 0; p0 < p.g.P; p0 += 16) {
    d4 d;
    const double xn = dot_tile(p.g, img, off, a, p0, lane, d);
    const int pc = p0 + (lane & 15);
    const bool valid = pc < p.g.P;
    const double w = valid ? p.wts[pc] : 0.0;
    const double poison = xn - xn;   // 0.0 for a finite patch, NaN for one with a NaN or an Inf: r2 = +Inf must not end as exp = 0
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double r2 = fma(-2.0, d[r], zr[r] + xn) + poison;
      const double e = w * exp(-0.5 * r2);
      acc[r] += valid ? e : 0.0;
    }
  }
  const double scale = p.variance / (double)p.g.P;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double s = column_sum(acc[r]);
    const int row = m0 + (lane >> 4) + 4 * r;
    if ((lane & 15) == 0 && row < p.M) p.out[(long)n * p.ldo + row] = s * scale;
  }
}

// ---- K_diag -------------------------------------------------------------------------------------------------------------------
// rows and columns of one tile of the patch Gram, both gathered: d, the column's norm / weight, and per D row r the norm / weight
struct GramTile {
  d4 d;
  double bn, wb, an[4], wa[4];
};
__device__ __forceinline__ void gram_tile(const ConvArgs& p, const double* img, const int* off, int tp, int tq, int lane, GramTile& t) {
  const Geom& g = p.g;
  const int pa = tp * 16 + (lane & 15), pb = tq * 16 + (lane & 15), grp = lane >> 4;
  const bool va = pa < g.P, vb = pb < g.P;
  const int basea = patch_base(g, va ? pa : g.P - 1), baseb = patch_base(g, vb ? pb : g.P - 1);
  double an = 0.0, bn = 0.0;
  t.d = (d4){0.0, 0.0, 0.0, 0.0};
  for (int kk = 0; kk < g.nk; ++kk) {
    const int o = off[4 * kk + grp];
    const double a = patch_elem(img, basea, va, o), b = patch_elem(img, baseb, vb, o);
    an = fma(a, a, an);
    bn = fma(b, b, bn);
    t.d = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, t.d, 0, 0, 0);
  }
  an = group_sum(an);
  t.bn = group_sum(bn);
  t.wb = vb ? p.wts[pb] : 0.0;
  const double wa = va ? p.wts[pa] : 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    t.an[r] = __shfl(an, grp + 4 * r);
    t.wa[r] = __shfl(wa, grp + 4 * r);
  }
}

__device__ __forceinline__ double wave_sum(double x) {
  x = column_sum(x);
  return group_sum(x);
}

__global__ __launch_bounds__(256) void conv_kdiag_kernel(ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* img = sm;
  double* red = sm + p.g.npix;   // [4]
  int* off = reinterpret_cast<int*>(red + 4);
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  stage_image(p, n, img);
  stage_offsets(p.g, off);
  __syncthreads();
  const int ntile = cdiv_dev(p.g.P, 16);
  double acc = 0.0;
  int cnt = 0;
  for (int tp = 0; tp < ntile; ++tp)
    for (int tq = 0; tq <= tp; ++tq, ++cnt) {
      if ((cnt & 3) != wave) continue;
      GramTile t;
      gram_tile(p, img, off, tp, tq, lane, t);
      const int pcol = tq * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int prow = tp * 16 + (lane >> 4) + 4 * r;
        const bool in = prow < p.g.P && pcol < p.g.P;
        const double ww = t.wa[r] * t.wb;
        double term = 0.0;
        if (in && prow > pcol) {
          const double r2 = fma(-2.0, t.d[r], t.an[r] + t.bn);
          term = 2.0 * (ww * exp(-0.5 * r2));
        } else if (in && prow == pcol) {
          term = ww + (t.bn - t.bn);   // by index: k = v (the scale below); |x|^2 - |x|^2 carries a NaN / Inf patch
        }
        acc += term;
      }
    }
  acc = wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) p.out[n] = (((red[0] + red[1]) + red[2]) + red[3]) * (p.variance / ((double)p.g.P * (double)p.g.P));
}

// ---- the Kfu adjoint ----------------------------------------------------------------------------------------------------------
// With E = exp(-r2 / 2), gg_{nmp} = G[n, m] w_p E (so that g of the derivation is (v / P) gg):
//   dv = sum gg / P        dl = (v / P) sum gg r2 / l        dZ[m, :] = (v / P) (1 / l) (sum_{n,p} gg x~_p - z~_m sum_{n,p} gg)
//   dw_p = (v / P) sum_{n,m} G[n, m] E
// Workgroup (chunk, M block): images n = chunk, chunk + nchunk, ...  Per 16-patch tile the seed tile gg [16 m x 16 p] of each wave goes
// through LDS from the D layout into A fragments, and sum_p gg x~_p is a SECOND matrix product [16 x 16] . [16 x patch_len] with the
// patches gathered again (B fragment: column = patch element, k = patch), accumulated in registers over the whole chunk.  Partials:
//   pZ  [nchunk, M, 4 nk]    sum_{n in chunk, p} gg x~_p            psg [nchunk, M]   sum_{n in chunk, p} gg
//   pw  [nwg, P]             sum_{n in chunk, m in block} G E       ps  [nwg, 2]      sum gg, sum gg r2
// each slot written by one thread of one workgroup; the tail adds them in index order.
__global__ __launch_bounds__(256) void conv_kfu_adjoint_kernel(ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const Geom& g = p.g;
  double* img = sm;
  double* dw = img + g.npix;             // [P]
  double* gt = dw + g.P;                 // [4][16][GT_LD]
  double* wt = gt + 4 * 16 * GT_LD;      // [4][16]
  double* red = wt + 64;                 // [8]
  int* off = reinterpret_cast<int*>(red + 8);
  const int chunk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, col = lane & 15;
  const int m0 = blockIdx.y * MBLK + wave * 16;
  const int wg = blockIdx.y * gridDim.x + blockIdx.x;
  const int nkt = cdiv_dev(g.plen, 16);
  for (int e = threadIdx.x; e < g.P; e += 256) dw[e] = 0.0;
  stage_offsets(g, off);
  double a[MAXNK], zr[4];
  load_z(p, m0, lane, a, zr);
  d4 dz[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) dz[kt] = (d4){0.0, 0.0, 0.0, 0.0};
  double sg[4] = {0.0, 0.0, 0.0, 0.0}, s_g = 0.0, s_gr2 = 0.0;
  double* mygt = gt + wave * 16 * GT_LD;

  for (int n = chunk; n < p.N; n += p.nchunk) {
    __syncthreads();   // (the previous image's last reads)
    stage_image(p, n, img);
    __syncthreads();
    double Gr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + grp + 4 * r;
      Gr[r] = row < p.M ? p.G[(long)n * p.ldg + row] : 0.0;
    }
    for (int p0 = 0; p0 < g.P; p0 += 16) {
      d4 d;
      const double xn = dot_tile(g, img, off, a, p0, lane, d);
      const int pc = p0 + col;
      const bool valid = pc < g.P;
      const double w = valid ? p.wts[pc] : 0.0;
      double wsum = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool in = valid && (m0 + grp + 4 * r < p.M);
        const double r2 = fma(-2.0, d[r], zr[r] + xn) + (xn - xn);   // (as the forward: an Inf patch is NaN, never exp = 0)
        const double ge = in ? Gr[r] * exp(-0.5 * r2) : 0.0;
        const double gg = in ? ge * w : 0.0;
        wsum += ge;
        sg[r] += gg;
        s_g += gg;
        s_gr2 += in ? gg * r2 : 0.0;
        mygt[(grp + 4 * r) * GT_LD + col] = gg;
      }
      wsum = group_sum(wsum);
      if (grp == 0) wt[wave * 16 + col] = wsum;
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double a2 = mygt[col * GT_LD + 4 * s + grp];
        const int pp = p0 + 4 * s + grp;
        const bool vp = pp < g.P;
        const int base2 = patch_base(g, vp ? pp : g.P - 1);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          if (kt < nkt) {
            const double b2 = patch_elem(img, base2, vp, off[kt * 16 + col]);
            dz[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, dz[kt], 0, 0, 0);
          }
      }
      if (wave == 0 && lane < 16 && p0 + lane < g.P) dw[p0 + lane] += ((wt[lane] + wt[16 + lane]) + wt[32 + lane]) + wt[48 + lane];
      __syncthreads();
    }
  }

  const int kp = 4 * g.nk;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = m0 + grp + 4 * r;
    const double s = column_sum(sg[r]);
    if (row < p.M) {
      if (col == 0) p.psg[(long)chunk * p.M + row] = s;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const int k = kt * 16 + col;
        if (kt < nkt && k < kp) p.pZ[((long)chunk * p.M + row) * kp + k] = dz[kt][r];
      }
    }
  }
  s_g = wave_sum(s_g);
  s_gr2 = wave_sum(s_gr2);
  if (lane == 0) {
    red[2 * wave] = s_g;
    red[2 * wave + 1] = s_gr2;
  }
  __syncthreads();
  if (threadIdx.x < 2) p.ps[(long)wg * 2 + threadIdx.x] = ((red[threadIdx.x] + red[2 + threadIdx.x]) + red[4 + threadIdx.x]) + red[6 + threadIdx.x];
  for (int e = threadIdx.x; e < g.P; e += 256) p.pw[(long)wg * g.P + e] = dw[e];
}

// one thread per output: dZ [M, patch_len], dw [P], dsmall [2] = (dv, dl)
__global__ __launch_bounds__(256) void conv_kfu_adjoint_tail_kernel(ConvArgs p) {
  const Geom& g = p.g;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long nz = (long)p.M * g.plen;
  const double vp = p.variance / (double)g.P;
  const int kp = 4 * g.nk;
  if (idx < nz) {
    const int m = (int)(idx / g.plen), k = (int)(idx - (long)m * g.plen);
    double s = 0.0, sgs = 0.0;
    for (int c = 0; c < p.nchunk; ++c) {
      s += p.pZ[((long)c * p.M + m) * kp + k];
      sgs += p.psg[(long)c * p.M + m];
    }
    const double z = p.Z[(long)m * p.ldz + k] / p.ls;
    p.dZ[(long)m * p.lddz + k] = (vp / p.ls) * (s - z * sgs);
  } else if (idx < nz + g.P) {
    const int q = (int)(idx - nz);
    double s = 0.0;
    for (int b = 0; b < p.nwg; ++b) s += p.pw[(long)b * g.P + q];
    p.dw[q] = vp * s;
  } else if (idx < nz + g.P + 2) {
    const int q = (int)(idx - nz - g.P);
    double s = 0.0;
    for (int b = 0; b < p.nwg; ++b) s += p.ps[(long)b * 2 + q];
    p.dsmall[q] = q == 0 ? s / (double)g.P : vp * s / p.ls;
  }
}

// ---- the K_diag adjoint -------------------------------------------------------------------------------------------------------
// With S_p = sum_q w_q E(p, q) (q == p by index: E = 1) and c_n = dF/dK_diag[n]:
//   dv = (1 / P^2) sum_n c_n sum_p w_p S_p     dl = (v / P^2) sum_n c_n sum_{p != q} w_p w_q E r2 / l     dw_p = (2 v / P^2) sum_n c_n S_p
// Workgroup = chunk of images; a wave owns the row tiles tp = wave, wave + 4, ... of the FULL P x P sweep (every S_p is finished by one
// wave, so the LDS sums dw[p] have one writer).  Partials pw [nchunk, P], ps [nchunk, 2], added by the tail in chunk order.
__global__ __launch_bounds__(256) void conv_kdiag_adjoint_kernel(ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const Geom& g = p.g;
  double* img = sm;
  double* dw = img + g.npix;   // [P]
  double* red = dw + g.P;      // [8]
  int* off = reinterpret_cast<int*>(red + 8);
  const int chunk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, col = lane & 15;
  const int ntile = cdiv_dev(g.P, 16);
  for (int e = threadIdx.x; e < g.P; e += 256) dw[e] = 0.0;
  stage_offsets(g, off);
  double s_k = 0.0, s_r = 0.0;
  for (int n = chunk; n < p.N; n += p.nchunk) {
    __syncthreads();
    stage_image(p, n, img);
    __syncthreads();
    const double cn = p.G[n];
    for (int tp = wave; tp < ntile; tp += 4) {
      double rs[4] = {0.0, 0.0, 0.0, 0.0}, wrow[4] = {0.0, 0.0, 0.0, 0.0};
      for (int tq = 0; tq < ntile; ++tq) {
        GramTile t;
        gram_tile(p, img, off, tp, tq, lane, t);
        const int pcol = tq * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int prow = tp * 16 + grp + 4 * r;
          const bool in = prow < g.P && pcol < g.P;
          wrow[r] = t.wa[r];
          if (in && prow != pcol) {
            const double r2 = fma(-2.0, t.d[r], t.an[r] + t.bn);
            const double e = t.wb * exp(-0.5 * r2);
            rs[r] += e;
            s_r += cn * ((t.wa[r] * e) * r2);
          } else if (in) {
            rs[r] += t.wb + (t.bn - t.bn);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int prow = tp * 16 + grp + 4 * r;
        const double S = column_sum(rs[r]);
        if (col == 0 && prow < g.P) {
          dw[prow] += cn * S;
          s_k += cn * (wrow[r] * S);
        }
      }
    }
  }
  s_k = wave_sum(s_k);
  s_r = wave_sum(s_r);
  if (lane == 0) {
    red[2 * wave] = s_k;
    red[2 * wave + 1] = s_r;
  }
  __syncthreads();
  if (threadIdx.x < 2) p.ps[(long)chunk * 2 + threadIdx.x] = ((red[threadIdx.x] + red[2 + threadIdx.x]) + red[4 + threadIdx.x]) + red[6 + threadIdx.x];
  for (int e = threadIdx.x; e < g.P; e += 256) p.pw[(long)chunk * g.P + e] = dw[e];
}

__global__ __launch_bounds__(256) void conv_kdiag_adjoint_tail_kernel(ConvArgs p) {
  const Geom& g = p.g;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const double pp = (double)g.P * (double)g.P;
  if (idx < g.P) {
    double s = 0.0;
    for (int c = 0; c < p.nchunk; ++c) s += p.pw[(long)c * g.P + idx];
    p.dw[idx] = (2.0 * p.variance / pp) * s;
  } else if (idx < g.P + 2) {
    const int q = (int)(idx - g.P);
    double s = 0.0;
    for (int c = 0; c < p.nchunk; ++c) s += p.ps[(long)c * 2 + q];
    p.dsmall[q] = q == 0 ? s / pp : (p.variance / pp) * s / p.ls;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// the limits of include/gpk.h: H W C <= GPK_CONV_MAX_PIXELS, h w <= GPK_MAX_D, 1 <= h <= H, 1 <= w <= W
int read_geometry(Geom& g, int H, int W, int C, int h, int w) {
  if (H < 1 || W < 1 || C < 1 || h < 1 || w < 1 || h > H || w > W) return GPK_E_ARG;
  if ((long)H * W * C > GPK_CONV_MAX_PIXELS || (long)h * w > GPK_MAX_D) return GPK_E_ARG;
  g.W = W; g.C = C; g.w = w; g.oh = H - h + 1; g.ow = W - w + 1;
  g.P = C * g.oh * g.ow; g.plen = h * w; g.nk = gpk_cdiv(g.plen, 4); g.npix = H * W * C;
  return 0;
}

int read_base(ConvArgs& a, double variance, double lengthscale) {
  if (!std::isfinite(variance) || !std::isfinite(lengthscale) || !(lengthscale > 0.0)) return GPK_E_ARG;
  a.variance = variance; a.ls = lengthscale;
  return 0;
}

int kfu_adjoint_chunks(int N) { return N < KFU_ADJ_CHUNKS ? N : KFU_ADJ_CHUNKS; }
int kdiag_adjoint_chunks(int N) { return N < KDIAG_ADJ_CHUNKS ? N : KDIAG_ADJ_CHUNKS; }

template <auto KERNEL>
hipError_t allow_adjoint_lds() {   // image + dw + seed tiles: up to 75 KB of dynamic LDS
  static const hipError_t at = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)((2 * GPK_CONV_MAX_PIXELS + 4 * 16 * GT_LD + 64 + 8) * sizeof(double) + GPK_MAX_D * sizeof(int)));
  return at;
}
}  // namespace

extern "C" int gpk_conv_kfu(void* stream, const double* X, int N, long ldx, int H, int W, int C, int h, int w, const double* Z, int M,
                            long ldz, const double* weights, double variance, double lengthscale, double* Kfu, long ldk) {
  ConvArgs a{};
  GPK_TRY(read_geometry(a.g, H, W, C, h, w));
  GPK_TRY(read_base(a, variance, lengthscale));
  if (N < 0 || M < 0 || ldx < a.g.npix || ldz < a.g.plen || ldk < M) return GPK_E_ARG;
  if (N == 0 || M == 0) return 0;
  if (!X || !Z || !weights || !Kfu) return GPK_E_ARG;
  a.X = X; a.ldx = ldx; a.N = N; a.Z = Z; a.ldz = ldz; a.M = M; a.wts = weights; a.out = Kfu; a.ldo = ldk;
  const size_t lds = (size_t)a.g.npix * sizeof(double) + GPK_MAX_D * sizeof(int);
  hipLaunchKernelGGL(conv_kfu_kernel, dim3((unsigned)N, (unsigned)gpk_cdiv(M, MBLK)), dim3(256), lds, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_conv_kdiag(void* stream, const double* X, int N, long ldx, int H, int W, int C, int h, int w, const double* weights,
                              double variance, double lengthscale, double* out) {
  ConvArgs a{};
  GPK_TRY(read_geometry(a.g, H, W, C, h, w));
  GPK_TRY(read_base(a, variance, lengthscale));
  if (N < 0 || ldx < a.g.npix) return GPK_E_ARG;
  if (N == 0) return 0;
  if (!X || !weights || !out) return GPK_E_ARG;
  a.X = X; a.ldx = ldx; a.N = N; a.wts = weights; a.out = out;
  const size_t lds = (size_t)(a.g.npix + 4) * sizeof(double) + GPK_MAX_D * sizeof(int);
  hipLaunchKernelGGL(conv_kdiag_kernel, dim3((unsigned)N), dim3(256), lds, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gpk_conv_kfu_partials_len(int N, int M, int H, int W, int C, int h, int w) {
  Geom g;
  if (read_geometry(g, H, W, C, h, w) || N < 0 || M < 0) return 0;
  const size_t nc = (size_t)kfu_adjoint_chunks(N), nwg = nc * (size_t)gpk_cdiv(M, MBLK);
  return nc * (size_t)M * (size_t)(4 * g.nk + 1) + nwg * (size_t)(g.P + 2);
}

extern "C" int gpk_conv_kfu_adjoint(void* stream, const double* X, int N, long ldx, int H, int W, int C, int h, int w, const double* Z,
                                    int M, long ldz, const double* weights, double variance, double lengthscale, const double* G,
                                    long ldg, double* parts, double* dsmall, double* dZ, long lddz, double* dw) {
  ConvArgs a{};
  GPK_TRY(read_geometry(a.g, H, W, C, h, w));
  GPK_TRY(read_base(a, variance, lengthscale));
  if (N < 0 || M < 0 || ldx < a.g.npix || ldz < a.g.plen || ldg < M || lddz < a.g.plen) return GPK_E_ARG;
  if (!dsmall || !dw || (M > 0 && (!Z || !dZ))) return GPK_E_ARG;
  const bool work = N > 0 && M > 0;
  if (work && (!X || !weights || !G || !parts)) return GPK_E_ARG;
  a.X = X; a.ldx = ldx; a.N = N; a.Z = Z; a.ldz = ldz; a.M = M; a.wts = weights; a.G = G; a.ldg = ldg;
  a.dsmall = dsmall; a.dZ = dZ; a.lddz = lddz; a.dw = dw;
  a.nchunk = work ? kfu_adjoint_chunks(N) : 0;
  const int mblocks = gpk_cdiv(M, MBLK);
  a.nwg = a.nchunk * mblocks;
  const int kp = 4 * a.g.nk;
  a.pZ = parts;
  a.psg = a.pZ + (size_t)a.nchunk * M * kp;
  a.pw = a.psg + (size_t)a.nchunk * M;
  a.ps = a.pw + (size_t)a.nwg * a.g.P;
  if (work) {
    GPK_HIP(allow_adjoint_lds<conv_kfu_adjoint_kernel>());
    const size_t lds = (size_t)(a.g.npix + a.g.P + 4 * 16 * GT_LD + 64 + 8) * sizeof(double) + GPK_MAX_D * sizeof(int);
    hipLaunchKernelGGL(conv_kfu_adjoint_kernel, dim3((unsigned)a.nchunk, (unsigned)mblocks), dim3(256), lds, (hipStream_t)stream, a);
    GPK_LAUNCH_CHECK();
  }
  const long items = (long)M * a.g.plen + a.g.P + 2;
  hipLaunchKernelGGL(conv_kfu_adjoint_tail_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gpk_conv_kdiag_partials_len(int N, int H, int W, int C, int h, int w) {
  Geom g;
  if (read_geometry(g, H, W, C, h, w) || N < 0) return 0;
  return (size_t)kdiag_adjoint_chunks(N) * (size_t)(g.P + 2);
}

extern "C" int gpk_conv_kdiag_adjoint(void* stream, const double* X, int N, long ldx, int H, int W, int C, int h, int w,
                                      const double* weights, double variance, double lengthscale, const double* c, double* parts,
                                      double* dsmall, double* dw) {
  ConvArgs a{};
  GPK_TRY(read_geometry(a.g, H, W, C, h, w));
  GPK_TRY(read_base(a, variance, lengthscale));
  if (N < 0 || ldx < a.g.npix || !dsmall || !dw) return GPK_E_ARG;
  if (N > 0 && (!X || !weights || !c || !parts)) return GPK_E_ARG;
  a.X = X; a.ldx = ldx; a.N = N; a.wts = weights; a.G = c; a.dsmall = dsmall; a.dw = dw;
  a.nchunk = kdiag_adjoint_chunks(N);
  a.pw = parts;
  a.ps = parts + (size_t)a.nchunk * a.g.P;
  if (N > 0) {
    GPK_HIP(allow_adjoint_lds<conv_kdiag_adjoint_kernel>());
    const size_t lds = (size_t)(a.g.npix + a.g.P + 8) * sizeof(double) + GPK_MAX_D * sizeof(int);
    hipLaunchKernelGGL(conv_kdiag_adjoint_kernel, dim3((unsigned)a.nchunk), dim3(256), lds, (hipStream_t)stream, a);
    GPK_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(conv_kdiag_adjoint_tail_kernel, dim3((unsigned)gpk_cdiv(a.g.P + 2, 256)), dim3(256), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}
