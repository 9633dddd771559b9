// pair_tile.h, staging: the tile's rows of X1 and X2 into the [d][T] slabs, padding rows 0.0; thread t handles (row t / d, column t % d)
// and on by 256
  for (int e = tid; e < T * d; e += 256) {
    const int row = e / d, dd = e - row * d;
    PAIR_STAGE_LOCALS
    const int g1 = r0 + row, g2 = c0 + row;
    x1t[dd * T + row] = (g1 < p.n1) ? PAIR_STAGE_FIRST(p.X1[(long)g1 * p.ldx1 + dd]) : 0.0;
    x2t[dd * T + row] = (g2 < p.n2) ? PAIR_STAGE_SECOND(p.X2[(long)g2 * p.ldx2 + dd]) : 0.0;
  }
  __syncthreads();
