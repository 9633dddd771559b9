// pair_tile.h, `full`: the tile is whole and every row of it can be written in 16-byte stores
  const bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && ((PAIR_LDO & 1) == 0) &&
                    ((reinterpret_cast<uintptr_t>(PAIR_OUT) & 15) == 0);
