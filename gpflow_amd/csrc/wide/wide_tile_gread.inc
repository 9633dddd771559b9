// wide_tile.h, fragment 2 of 3 -- inside the file's row_values(i, g, tr, out), after `gr = r0 + tr`: gv[j], the NB values of G that
// sit under this lane's NB outputs of global row gr (BUILD: nothing is read).
    double gv[NB];
    if constexpr (!BUILD) {
      if (gvec) {
#pragma unroll
        for (int j = 0; j < NB; j += 2) {
          const d2 t = *reinterpret_cast<const d2*>(p.G + (long)gr * p.ldg + c0 + tc0 + j);
          gv[j] = t[0]; gv[j + 1] = t[1];
        }
      } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) gv[j] = (gr < p.n1 && c0 + tc0 + j < p.n2) ? p.G[(long)gr * p.ldg + c0 + tc0 + j] : 0.0;
      }
    }
