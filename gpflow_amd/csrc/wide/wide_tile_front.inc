// wide_tile.h, fragment 1 of 3 -- the first statements of a tile kernel's body: staging, the K loop, the norms, the edge predicates.
// Reads T, p, NPH, PAD and the WIDE_* macros of the including file; leaves the names wide_tile.h lists.
  using G_ = Geo<T>;
  constexpr int WT = G_::WT, NB = G_::NB, EPT = G_::EPT, TPR = G_::TPR, SLAB = G_::SLAB;
  constexpr int PW = BK / NPH, PPT = EPT / PW;   // columns of a norm phase; phases (register partials) per staging thread
  static_assert(PW * NPH == BK && PPT * PW == EPT, "a staging thread's columns are whole phases");
  static_assert(2 * T * NPH + 2 * T <= 4 * SLAB, "the norm partials and the norms reuse the slabs");
  extern __shared__ __attribute__((aligned(16))) double sm[];   // [2 buffers][2 operands][SLAB]

  if (WIDE_SYM && blockIdx.x > blockIdx.y) return;   // strictly upper tile: skipped (lower_only) or written by its mirror
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
  const double s0 = WIDE_SCALES[0];

  double ra[EPT], rb[EPT], rs[EPT];
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
    for (int e = 0; e < EPT; ++e) rs[e] = (ks + scol + e < d) ? (p.ard ? WIDE_SCALES[ks + scol + e] : s0) : PAD;
  };
  // this thread's share of the norm of row srow of either operand: one chain per column phase, over every slab
  double np1[PPT], np2[PPT];
#pragma unroll
  for (int f = 0; f < PPT; ++f) np1[f] = np2[f] = 0.0;
  auto lstore = [&](double* buf) {
#pragma unroll
    for (int e = 0; e < EPT; e += 2) {
      const double a0 = WIDE_STAGE(ra[e], rs[e]), a1 = WIDE_STAGE(ra[e + 1], rs[e + 1]);
      const double b0 = WIDE_STAGE(rb[e], rs[e]), b1 = WIDE_STAGE(rb[e + 1], rs[e + 1]);
      double& n1 = np1[WIDE_PARTIAL_OF(e)];
      double& n2 = np2[WIDE_PARTIAL_OF(e)];
      n1 = WIDE_NORM_TERM(a0, ra[e], n1); n1 = WIDE_NORM_TERM(a1, ra[e + 1], n1);
      n2 = WIDE_NORM_TERM(b0, rb[e], n2); n2 = WIDE_NORM_TERM(b1, rb[e + 1], n2);
      *reinterpret_cast<d2*>(&buf[so1 + e]) = (d2){a0, a1};
      *reinterpret_cast<d2*>(&buf[so2 + e]) = (d2){WIDE_SECOND(b0, rb[e]), WIDE_SECOND(b1, rb[e + 1])};
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

  // ---- norms: a row's phase partials in phase order, then the file's finish (the slabs are no longer read) ----
  double* part = sm;                  // [2][T][NPH]
  double* nrm = sm + 2 * T * NPH;     // [2][T]: rows, then columns, by TILE index
#pragma unroll
  for (int f = 0; f < PPT; ++f) {
    part[srow * NPH + WIDE_FIRST_PHASE + f] = np1[f];
    part[(T + srow) * NPH + WIDE_FIRST_PHASE + f] = np2[f];
  }
  __syncthreads();
  if (tid < 2 * T) {
    double s = part[tid * NPH];
#pragma unroll
    for (int ph = 1; ph < NPH; ++ph) s += part[tid * NPH + ph];
    WIDE_NORM_FINISH(s);
  }
  __syncthreads();

  // ---- epilogue ----------------------------------------------------------------------------------
  const bool aligned = ((p.ldk & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.K) & 15) == 0);
  const bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && aligned;
  const bool mirror = WIDE_SYM && !p.lower_only;
  const bool diag_mirror = mirror && r0 == c0;   // the lower half and, inside the tile, its transpose
  const int tc0 = wc * WT + l15 * NB;            // this lane's NB consecutive tile columns
