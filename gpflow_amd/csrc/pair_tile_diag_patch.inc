// pair_tile.h, a patch on the diagonal of a diagonal tile (tx == ty) takes its upper entries from its lower ones
  if (diag_tile && tx == ty) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i + 1; j < 4; ++j) v[i][j] = v[j][i];
  }
