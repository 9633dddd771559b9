// pair_tile.h, after a tile kernel: the macros it defined for the fragments end with it
#undef PAIR_STAGE_LOCALS
#undef PAIR_STAGE_FIRST
#undef PAIR_STAGE_SECOND
#undef PAIR_FIRST
#undef PAIR_OUT
#undef PAIR_LDO
#undef PAIR_WRITTEN
