// wide_tile.h, fragment 3 of 3 -- after the file's row_values: the stores of the tile, block row by block row, with both mirror paths.
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
    if constexpr (!BUILD) {   // no mirror (these sweep the full rectangle): a row is stored as soon as it is formed
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
      if (mirror && r0 != c0) {   // transposed copy: rows c0 + tc0 + j, columns r0 + tr0 .. + 3   (sym: n1 == n2)
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
