// pair_tile.h, the row stores: a thread's four rows of v, 32 contiguous bytes each where `full`
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
    if (full) {
      d2* out = reinterpret_cast<d2*>(PAIR_OUT + (long)gr * PAIR_LDO + c0 + tx * 4);
      out[0] = (d2){v[i][0], v[i][1]};
      out[1] = (d2){v[i][2], v[i][3]};
    } else if (gr < p.n1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gc = c0 + tx * 4 + j;
        if (PAIR_WRITTEN(gr, gc)) PAIR_OUT[(long)gr * PAIR_LDO + gc] = v[i][j];
      }
    }
  }
