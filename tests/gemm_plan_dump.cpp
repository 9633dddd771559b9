// Prints the launch plan of GEMM calls: tests/test_gemm_plan.py builds this with plain g++ (no ROCm include path -- which is the check
// that gemm_plan.h needs no HIP header) and reads the lines back.
//   gemm_plan_dump key=value ...     one call
//   gemm_plan_dump @FILE             one call per line of FILE (the same key=value words)
// Keys: the GemmArgs scalars by name (m n k epi b_tri ...; defaults: gemm_base(m, n, k, alpha = -1, beta = 1) for epi 0, alpha = 1,
// beta = 0 and no C for epi 1, lda = ldb = ldc = 2048 + 8 or k / n rounded up if larger), and
//   align=0 aligned operands   1 odd lda   2 A aligned to 8 bytes only
//   stats=1  stat_sumsq / stat_mv / stat_V set, stat_P = batch (stat_P=... overrides)
// Pointers are fabricated: no memory is touched.  Each plan is printed as `key value` lines and a closing `end` line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../gpflow_amd/csrc/gemm_plan.h"

static const char* name(GemmKernel k) {
  switch (k) {
    case GemmKernel::none: return "none";
    case GemmKernel::small: return "small";
    case GemmKernel::pre64: return "pre64";
    case GemmKernel::generic: return "generic";
    case GemmKernel::fast: return "fast";
    default: return "unsupported";
  }
}

static int dump(const std::vector<std::string>& words) {
  int m = 0, n = 0, k = 0, epi = 0, align = 0, stats = 0, stat_P = -1, batch = 1;
  double alpha = 0.0, beta = 0.0;
  bool have_alpha = false, have_beta = false;
  GemmArgs o{};   // the flags given by name
  for (const std::string& w : words) {
    const size_t eq = w.find('=');
    if (eq == std::string::npos) return 2;
    const std::string key = w.substr(0, eq);
    const char* val = w.c_str() + eq + 1;
    const int iv = atoi(val);
    if (key == "m") m = iv;
    else if (key == "n") n = iv;
    else if (key == "k") k = iv;
    else if (key == "epi") epi = iv;
    else if (key == "align") align = iv;
    else if (key == "stats") stats = iv;
    else if (key == "stat_P") stat_P = iv;
    else if (key == "batch") batch = iv;
    else if (key == "alpha") { alpha = atof(val); have_alpha = true; }
    else if (key == "beta") { beta = atof(val); have_beta = true; }
    else if (key == "c_lower") o.c_lower = iv;
    else if (key == "b_tri") o.b_tri = iv;
    else if (key == "a_tri") o.a_tri = iv;
    else if (key == "b_tri_off") o.b_tri_off = iv;
    else if (key == "k_off_step") o.k_off_step = iv;
    else if (key == "stagger_first") o.stagger_first = iv;
    else if (key == "no_small") o.no_small = iv;
    else if (key == "small_loop") o.small_loop = iv;
    else if (key == "max_wgs") o.max_wgs = iv;
    else if (key == "tile_queue") o.tile_queue = iv;
    else if (key == "tile64") o.tile64 = iv;
    else return 2;
  }
  if (!have_alpha) alpha = epi == 1 ? 1.0 : -1.0;
  if (!have_beta) beta = epi == 1 ? 0.0 : 1.0;
  // fabricated operands: 4 KiB-aligned addresses far apart, rows of at least 2056 doubles
  long lda = k > 2048 ? k + 8 : 2056, ldb = lda, ldc = n > 2048 ? n + 8 : 2056;
  uintptr_t pa = (uintptr_t)1 << 32, pb = (uintptr_t)2 << 32, pc = (uintptr_t)3 << 32;
  if (align == 1) lda += 1;
  if (align == 2) pa += 8;
  double* C = (epi == 1 && beta == 0.0) ? nullptr : reinterpret_cast<double*>(pc);
  GemmArgs g = gemm_base(m, n, k, alpha, reinterpret_cast<const double*>(pa), lda, reinterpret_cast<const double*>(pb), ldb, beta, C,
                         ldc, batch, 0, batch > 1 ? (long)n * ldb : 0, batch > 1 ? (long)m * ldc : 0);
  g.c_lower = o.c_lower; g.b_tri = o.b_tri; g.a_tri = o.a_tri; g.b_tri_off = o.b_tri_off; g.k_off_step = o.k_off_step;
  g.stagger_first = o.stagger_first; g.no_small = o.no_small; g.small_loop = o.small_loop; g.max_wgs = o.max_wgs;
  g.tile_queue = o.tile_queue; g.tile64 = o.tile64;
  g.epi = epi;
  if (epi == 1) { g.sq_cols = n; g.part = reinterpret_cast<double*>((uintptr_t)4 << 32); g.part_ld = m; }
  if (stats) {
    g.stat_sumsq = reinterpret_cast<double*>((uintptr_t)5 << 32);
    g.stat_mv = reinterpret_cast<double*>((uintptr_t)6 << 32);
    g.stat_V = reinterpret_cast<const double*>((uintptr_t)7 << 32);
    g.stat_P = stat_P >= 0 ? stat_P : g.batch;
  }
  const GemmPlan p = make_gemm_plan(g);
  const GemmTileShape t = gemm_tile_shape(p.tile);
  printf("kernel %s\n", name(p.kernel));
  if (p.kernel == GemmKernel::generic) printf("tile %d,%d,%d,%d\n", t.bm, t.bn, t.wgm, t.wgn);
#define I(f) printf(#f " %ld\n", (long)p.f)
  I(epi); I(pair); I(queue); I(sp); I(kind); I(gx); I(gy); I(total); I(compact); I(ldk); I(grid_x); I(grid_y); I(grid_z); I(threads);
  I(lds_bytes); I(tile_snake); I(stagger_first); I(stagger_ticks); I(pair_k_align); I(tail_first1); I(tail_tiles); I(tail_grid_x);
  I(queue_wgs); I(queue_fetches);
#undef I
  printf("lower_tiles_128 %d\nend\n", gemm_lower_tiles(gemm_cdiv(n, 128), gemm_cdiv(m, 128)));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && argv[1][0] == '@') {
    FILE* f = fopen(argv[1] + 1, "r");
    if (!f) return 2;
    char line[1024];
    while (fgets(line, sizeof line, f)) {
      std::vector<std::string> words;
      for (char* w = strtok(line, " \n"); w; w = strtok(nullptr, " \n")) words.push_back(w);
      const int rc = dump(words);
      if (rc) return rc;
    }
    fclose(f);
    return 0;
  }
  return dump(std::vector<std::string>(argv + 1, argv + argc));
}
