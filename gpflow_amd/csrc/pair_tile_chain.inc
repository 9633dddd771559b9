// pair_tile.h, the chain: dot[i][j] = sum_dd PAIR_FIRST(x1t[dd][ty * 4 + i]) * x2t[dd][tx * 4 + j], an fma chain over ascending dd from 0.0
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) dot[i][j] = 0.0;
  for (int dd = 0; dd < d; ++dd) {
    const d2* a2 = reinterpret_cast<const d2*>(&x1t[dd * T + ty * 4]);
    const d2* b2 = reinterpret_cast<const d2*>(&x2t[dd * T + tx * 4]);
    const d2 a01 = a2[0], a23 = a2[1], b01 = b2[0], b23 = b2[1];
    const double a[4] = {PAIR_FIRST(a01.x), PAIR_FIRST(a01.y), PAIR_FIRST(a23.x), PAIR_FIRST(a23.y)};
    const double b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dot[i][j] = fma(a[i], b[j], dot[i][j]);
  }
