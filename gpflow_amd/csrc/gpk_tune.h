// Tunables of libgpk.  No HIP header here: the schedule plan (potrf_plan.h) is host arithmetic and compiles without one.
#pragma once
#include <stdio.h>
#include <stdlib.h>

// Tunables.  The PRODUCT build (libgpk.so) has none at run time: every GPK_TUNE is its compile-time default and the
// library never reads the environment.  Only the A/B build (`make exp` -> libgpk_exp.so, -DGPK_EXPERIMENTAL, used by
// tools/ab*.sh on the GPU box and never loaded by the package unless GPK_LIBRARY points at it) reads GPK_<NAME> once.
#ifdef GPK_EXPERIMENTAL
#define GPK_TUNE(name, def)                                                                      \
  ([]() -> int {                                                                                 \
    static const int v__ = getenv("GPK_" #name) ? atoi(getenv("GPK_" #name)) : (int)(def);       \
    return v__;                                                                                  \
  }())
#define GPK_TRACE(...)                                        \
  do {                                                        \
    if (GPK_TUNE(DEBUG, 0)) fprintf(stderr, "[gpk] " __VA_ARGS__); \
  } while (0)
#else
#define GPK_TUNE(name, def) ((int)(def))
#define GPK_TRACE(...) do { } while (0)
#endif

// kGpkExp: host branches that only exist in the A/B build are constant-folded away in the product library.
#ifdef GPK_EXPERIMENTAL
constexpr bool kGpkExp = true;
#else
constexpr bool kGpkExp = false;
#endif
