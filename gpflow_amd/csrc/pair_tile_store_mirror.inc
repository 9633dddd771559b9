// pair_tile.h, the transposed copy: rows c0 + tx*4 + j, columns r0 + ty*4 + i   (symmetric build: n1 == n2)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gr = c0 + tx * 4 + j;
    if (full) {
      d2* out = reinterpret_cast<d2*>(PAIR_OUT + (long)gr * PAIR_LDO + r0 + ty * 4);
      out[0] = (d2){v[0][j], v[1][j]};
      out[1] = (d2){v[2][j], v[3][j]};
    } else if (gr < p.n1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int gc = r0 + ty * 4 + i;
        if (gc < p.n2) PAIR_OUT[(long)gr * PAIR_LDO + gc] = v[i][j];
      }
    }
  }
