// The `key=value` words that describe one GEMM call, shared by tests/gemm_plan_dump.cpp (prints the plan, no device) and
// tests/gemm_launch_run.hip (prints the plan and runs the call): one parser, one rule for the leading dimensions, one way to fill
// the GemmArgs and one plan format, so the two cannot diverge.  Plain C++17, no HIP header.
// Keys: the GemmArgs scalars by name (m n k epi b_tri ...; defaults: gemm_base(m, n, k, alpha = -1, beta = 1) for epi 0, alpha = 1,
// beta = 0 and no C for epi 1, lda = ldb = ldc = 2048 + 8 or k / n rounded up if larger), and
//   align=0 aligned operands   1 odd lda   2 A aligned to 8 bytes only
//   stats=1  stat_sumsq / stat_mv / stat_V set, stat_P = batch (stat_P=... overrides)
//   sig=1    sig_ptr set, sig_val = 7          wait=1  wait_ptr / wait_info set, wait_val = 3 (the runner: the word already holds it)
//   dir=PATH directory of the operand files (the runner only)
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../gpflow_amd/csrc/gemm_plan.h"

struct GemmCase {
  int m = 0, n = 0, k = 0, epi = 0, align = 0, stats = 0, stat_P = -1, batch = 1, sig = 0, wait = 0;
  double alpha = 0.0, beta = 0.0;
  GemmArgs o{};   // the flags given by name
  std::string dir;
};
constexpr int kGemmCaseSigVal = 7, kGemmCaseWaitVal = 3;

// false: a word without '=' or with an unknown key
static inline bool gemm_case_parse(const std::vector<std::string>& words, GemmCase& c) {
  bool have_alpha = false, have_beta = false;
  for (const std::string& w : words) {
    const size_t eq = w.find('=');
    if (eq == std::string::npos) return false;
    const std::string key = w.substr(0, eq);
    const char* val = w.c_str() + eq + 1;
    const int iv = atoi(val);
    if (key == "m") c.m = iv;
    else if (key == "n") c.n = iv;
    else if (key == "k") c.k = iv;
    else if (key == "epi") c.epi = iv;
    else if (key == "align") c.align = iv;
    else if (key == "stats") c.stats = iv;
    else if (key == "stat_P") c.stat_P = iv;
    else if (key == "batch") c.batch = iv;
    else if (key == "sig") c.sig = iv;
    else if (key == "wait") c.wait = iv;
    else if (key == "dir") c.dir = val;
    else if (key == "alpha") { c.alpha = atof(val); have_alpha = true; }
    else if (key == "beta") { c.beta = atof(val); have_beta = true; }
    else if (key == "c_lower") c.o.c_lower = iv;
    else if (key == "b_tri") c.o.b_tri = iv;
    else if (key == "a_tri") c.o.a_tri = iv;
    else if (key == "b_tri_off") c.o.b_tri_off = iv;
    else if (key == "k_off_step") c.o.k_off_step = iv;
    else if (key == "stagger_first") c.o.stagger_first = iv;
    else if (key == "no_small") c.o.no_small = iv;
    else if (key == "small_loop") c.o.small_loop = iv;
    else if (key == "max_wgs") c.o.max_wgs = iv;
    else if (key == "tile_queue") c.o.tile_queue = iv;
    else if (key == "tile64") c.o.tile64 = iv;
    else return false;
  }
  if (!have_alpha) c.alpha = c.epi == 1 ? 1.0 : -1.0;
  if (!have_beta) c.beta = c.epi == 1 ? 0.0 : 1.0;
  return true;
}

static inline std::vector<std::string> gemm_case_split(char* line) {
  std::vector<std::string> words;
  for (char* w = strtok(line, " \n"); w; w = strtok(nullptr, " \n")) words.push_back(w);
  return words;
}

// rows of at least 2056 doubles; align = 1: odd lda
struct GemmCaseLd { long lda, ldb, ldc; };
static inline GemmCaseLd gemm_case_ld(const GemmCase& c) {
  GemmCaseLd l;
  l.lda = c.k > 2048 ? c.k + 8 : 2056;
  l.ldb = l.lda;
  l.ldc = c.n > 2048 ? c.n + 8 : 2056;
  if (c.align == 1) l.lda += 1;
  return l;
}
static inline bool gemm_case_has_c(const GemmCase& c) { return !(c.epi == 1 && c.beta == 0.0); }
static inline int gemm_case_stat_P(const GemmCase& c) { return c.stat_P >= 0 ? c.stat_P : (c.batch > 0 ? c.batch : 1); }

// The operands of the call: the dumper fabricates them, the runner allocates them.  A is the pointer the call gets (align = 2: 8 bytes
// past a 16-byte boundary); C is ignored where the case has none; the batch shares A.
struct GemmCaseMem {
  const double* A = nullptr; const double* B = nullptr; double* C = nullptr;
  double* part = nullptr; double* stat_sumsq = nullptr; double* stat_mv = nullptr; const double* stat_V = nullptr;
  int* sig_ptr = nullptr; const int* wait_ptr = nullptr; int* wait_info = nullptr;
};
static inline GemmArgs gemm_case_args(const GemmCase& c, const GemmCaseMem& mem) {
  const GemmCaseLd l = gemm_case_ld(c);
  GemmArgs g = gemm_base(c.m, c.n, c.k, c.alpha, mem.A, l.lda, mem.B, l.ldb, c.beta, gemm_case_has_c(c) ? mem.C : nullptr, l.ldc, c.batch,
                         0, c.batch > 1 ? (long)c.n * l.ldb : 0, c.batch > 1 ? (long)c.m * l.ldc : 0);
  const GemmArgs& o = c.o;
  g.c_lower = o.c_lower; g.b_tri = o.b_tri; g.a_tri = o.a_tri; g.b_tri_off = o.b_tri_off; g.k_off_step = o.k_off_step;
  g.stagger_first = o.stagger_first; g.no_small = o.no_small; g.small_loop = o.small_loop; g.max_wgs = o.max_wgs;
  g.tile_queue = o.tile_queue; g.tile64 = o.tile64;
  g.epi = c.epi;
  if (c.epi == 1) {   // one partial per 64 output columns: [2 * cdiv(n, 128)][m] per batch entry; no C2 columns
    g.sq_cols = c.n; g.part = mem.part; g.part_ld = c.m; g.stridePart = 2L * gemm_cdiv(c.n, 128) * c.m;
    g.C2 = mem.part; g.ldc2 = 0; g.strideC2 = 0; g.c2_cols = 0;
  }
  if (c.stats) {
    g.stat_sumsq = mem.stat_sumsq; g.stat_mv = mem.stat_mv; g.stat_V = mem.stat_V;
    g.stat_P = gemm_case_stat_P(c);
  }
  if (c.sig) { g.sig_ptr = mem.sig_ptr; g.sig_val = kGemmCaseSigVal; }
  if (c.wait) { g.wait_ptr = mem.wait_ptr; g.wait_val = kGemmCaseWaitVal; g.wait_info = mem.wait_info; }
  return g;
}

static inline const char* gemm_kernel_name(GemmKernel k) {
  switch (k) {
    case GemmKernel::none: return "none";
    case GemmKernel::small: return "small";
    case GemmKernel::pre64: return "pre64";
    case GemmKernel::generic: return "generic";
    case GemmKernel::fast: return "fast";
    default: return "unsupported";
  }
}

// the plan as `key value` lines (the caller closes the record with an `end` line)
static inline void gemm_plan_print(FILE* f, const GemmPlan& p, int m, int n) {
  const GemmTileShape t = gemm_tile_shape(p.tile);
  fprintf(f, "kernel %s\n", gemm_kernel_name(p.kernel));
  if (p.kernel == GemmKernel::generic) fprintf(f, "tile %d,%d,%d,%d\n", t.bm, t.bn, t.wgm, t.wgn);
#define I(x) fprintf(f, #x " %ld\n", (long)p.x)
  I(epi); I(pair); I(queue); I(sp); I(kind); I(gx); I(gy); I(total); I(compact); I(ldk); I(grid_x); I(grid_y); I(grid_z); I(threads);
  I(lds_bytes); I(tile_snake); I(stagger_first); I(stagger_ticks); I(pair_k_align); I(tail_first1); I(tail_tiles); I(tail_grid_x);
  I(queue_wgs); I(queue_fetches);
#undef I
  fprintf(f, "lower_tiles_128 %d\n", gemm_lower_tiles(gemm_cdiv(n, 128), gemm_cdiv(m, 128)));
}
