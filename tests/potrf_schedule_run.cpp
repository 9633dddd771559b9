// Runs the REAL enqueue code of the factorisation and of the fused drivers on the CPU against a recorder and prints what was
// enqueued, one JSON object per line: tests/test_potrf_schedule.py builds this with plain g++ (tests/hip_record first on the include
// path, once as the product build and once with -DGPK_EXPERIMENTAL) and checks the happens-before relation of the log.
//
// gpflow_amd/csrc/potrf.hip and drivers.hip are compiled unmodified (they hold no device code).  Everything they call and do not
// define is defined here:
//   * the HIP calls of tests/hip_record/hip/hip_runtime.h as recorders -- streams and events are numbered objects, hipMalloc hands
//     out fake addresses, the timing calls of the init-time self-check return constants;
//   * every gpk_launch_* / gpk_* launcher as a stub that logs its stream, a name and the memory its kernel reads and writes.  The
//     access list of a stub RESTATES its kernel; the kernel restated is named next to it (file:line at the time of writing).  A write
//     set may be a superset of what the kernel touches, a read set is never a subset.  Where a kernel reads AND writes the same
//     memory, the list is in the kernel's order: a read listed before the write is not served by it (the ticket of varexp_tail), a
//     read listed behind it is (that kernel's block partials) -- assertion 9 of tests/test_potrf_schedule.py relies on this.
//   * the two GEMM predicates, which are the library's own one-liners over make_gemm_plan (gemm_plan.h, plain C++).
// Operands are fake addresses chosen here, so the alignment and parity that gpk_potrf_core reads from pointer bits are inputs.
//
//   potrf_schedule_run ENTRY key=value ...
//     ENTRY   potrf | potrf_inv | trsm0 | trsm1 | gpr_lml | svgp | svgp_lik | svgp_sep
//     n       columns of the factor (M of the drivers)            extra   extra rows (potrf, potrf_inv), right-hand-side rows (trsm)
//     rows    minibatch rows (drivers)                            P       latents / columns of Y
//     batch   problems (potrf, trsm)                              layout  a (16-byte aligned, even strides) | p8 (8-byte-only aligned
//     whiten, q_diag  form of svgp / svgp_lik                             A) | odd (odd lda and batch stride)
//     conc    answer of gpk_probe_concurrent_kernels (0: flags_usable = 0)
//     reps    how many times the call is issued back to back on the same caller stream and workspace
// The A/B build reads its GPK_* tunables from the environment as the library does.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#ifndef POTRF_SRC
#define POTRF_SRC "../gpflow_amd/csrc/potrf.hip"
#endif
#ifndef DRIVERS_SRC
#define DRIVERS_SRC "../gpflow_amd/csrc/drivers.hip"
#endif

// ---- the recorder ---------------------------------------------------------------------------------------------------------------
struct RecStream { int id; };
struct RecEvent { int id; };
namespace rec {
int g_streams = 0, g_events = 0, g_concurrent = 1;
uintptr_t g_next_region = 1;
RecStream g_caller{0};   // the caller's stream: the device's default stream in the hardware-queue model of the checker

void line(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vprintf(fmt, ap);
  va_end(ap);
  putchar('\n');
}
void* region(const char* name, size_t bytes, size_t misalign = 0) {
  const uintptr_t base = (g_next_region++ << 40) + misalign;
  line("{\"k\":\"buf\",\"name\":\"%s\",\"base\":%llu,\"bytes\":%llu}", name, (unsigned long long)base, (unsigned long long)bytes);
  return (void*)base;
}
hipError_t new_stream(hipStream_t* s, const char* kind) {
  *s = new RecStream{++g_streams};
  line("{\"k\":\"stream\",\"s\":%d,\"kind\":\"%s\"}", (*s)->id, kind);
  return hipSuccess;
}
int sid(hipStream_t s) { return s ? s->id : 0; }

// one memory access of a launch: `rows` rows of `cols` elements of `elem` bytes, `ld` elements apart, `batch` of them `stride`
// elements apart.  Logged in BYTES.
struct Acc { char rw; const void* base; long rows, cols, ld; int batch; long stride; int elem; };
struct Launch {
  hipStream_t s;
  std::string name, desc;
  std::vector<Acc> acc;
  const void* sig_ptr = nullptr; int sig_val = 0; bool sig_on_entry = false;
  const void* wait_ptr = nullptr; int wait_val = 0;
  bool wait_dropped = false;     // a wait was asked of a kernel that does not honour it
  long wgs = 0, lds = 0;         // workgroups of the launch and LDS bytes of each (0: not restated)
  const char* info = "none";     // the status word: "reset" (leaf of column 0), "rmw" (later leaves), "may" (may store INT_MAX)
  const void* info_ptr = nullptr;

  Launch(hipStream_t s_, const char* name_) : s(s_), name(name_) {}
  Launch& d(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    desc = buf;
    return *this;
  }
  Launch& mat(char rw, const void* base, long rows, long cols, long ld, int batch = 1, long stride = 0, int elem = 8) {
    if (base && rows > 0 && cols > 0) acc.push_back(Acc{rw, base, rows, cols, ld, batch > 0 ? batch : 1, stride, elem});
    return *this;
  }
  Launch& R(const void* base, long rows, long cols, long ld, int batch = 1, long stride = 0) { return mat('R', base, rows, cols, ld, batch, stride); }
  Launch& W(const void* base, long rows, long cols, long ld, int batch = 1, long stride = 0) { return mat('W', base, rows, cols, ld, batch, stride); }
  Launch& vecR(const void* base, long n) { return mat('R', base, 1, n, n); }
  Launch& vecW(const void* base, long n) { return mat('W', base, 1, n, n); }
  Launch& status(const char* kind, const void* ptr) {
    if (ptr) { info = kind; info_ptr = ptr; }
    return *this;
  }
  int emit() {
    printf("{\"k\":\"launch\",\"s\":%d,\"name\":\"%s\",\"desc\":\"%s\",\"info\":\"%s\",\"info_ptr\":%llu", sid(s), name.c_str(), desc.c_str(), info,
           (unsigned long long)(uintptr_t)info_ptr);
    if (sig_ptr) printf(",\"sig\":[%llu,%d],\"sig_on_entry\":%d", (unsigned long long)(uintptr_t)sig_ptr, sig_val, sig_on_entry ? 1 : 0);
    if (wait_ptr) printf(",\"wait\":[%llu,%d]", (unsigned long long)(uintptr_t)wait_ptr, wait_val);
    if (wait_dropped) printf(",\"wait_dropped\":1");
    if (wgs) printf(",\"wgs\":%ld,\"lds\":%ld", wgs, lds);
    printf(",\"acc\":[");
    for (size_t i = 0; i < acc.size(); ++i) {
      const Acc& a = acc[i];
      printf("%s[\"%c\",%llu,%ld,%ld,%ld,%d,%ld]", i ? "," : "", a.rw, (unsigned long long)(uintptr_t)a.base, a.rows, a.cols * a.elem,
             a.ld * a.elem, a.batch, a.stride * a.elem);
    }
    printf("]}\n");
    return 0;
  }
};
}  // namespace rec
using rec::Launch;

hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int) { prop->multiProcessorCount = 256; return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) { *least = 0; *greatest = -1; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return rec::new_stream(s, "plain"); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return rec::new_stream(s, "priority"); }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t* s, uint32_t, const uint32_t*) { return rec::new_stream(s, "masked"); }
hipError_t hipStreamDestroy(hipStream_t s) { rec::line("{\"k\":\"stream_destroy\",\"s\":%d}", rec::sid(s)); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = new RecEvent{++rec::g_events}; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { rec::line("{\"k\":\"record\",\"s\":%d,\"ev\":%d}", rec::sid(s), e->id); return hipSuccess; }
// (the host waits: everything enqueued so far has completed)
hipError_t hipEventSynchronize(hipEvent_t) { rec::line("{\"k\":\"host_sync\"}"); return hipSuccess; }
// (the init-time self-check: 0.24 ms over 2 x 24 hand-offs = 5 us, a layout that passes)
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.24f; return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  rec::line("{\"k\":\"wait_event\",\"s\":%d,\"ev\":%d}", rec::sid(s), e->id);
  return hipSuccess;
}
hipError_t hipStreamWaitValue32(hipStream_t s, void* ptr, uint32_t value, unsigned, uint32_t) {
  rec::line("{\"k\":\"wait_value\",\"s\":%d,\"wait\":[%llu,%d]}", rec::sid(s), (unsigned long long)(uintptr_t)ptr, (int)value);
  return hipSuccess;
}
hipError_t hipStreamWriteValue32(hipStream_t s, void* ptr, uint32_t value, unsigned) {
  rec::line("{\"k\":\"write_value\",\"s\":%d,\"sig\":[%llu,%d]}", rec::sid(s), (unsigned long long)(uintptr_t)ptr, (int)value);
  return hipSuccess;
}
hipError_t hipMalloc(void** ptr, size_t bytes) { *ptr = rec::region("hipMalloc", bytes); return hipSuccess; }
hipError_t hipMemset(void*, int, size_t) { return hipSuccess; }   // (host-synchronous, init time only)
hipError_t hipMemsetAsync(void* ptr, int, size_t bytes, hipStream_t s) {
  return (hipError_t)Launch(s, "memset").mat('W', ptr, 1, (long)bytes, (long)bytes, 1, 0, 1).emit();
}

// ---- the code under test ----------------------------------------------------------------------------------------------------------
#include POTRF_SRC
#include DRIVERS_SRC

// ---- launch stubs: each restates the kernel named beside it ---------------------------------------------------------------------
// gemm.hip:1233 gpk_launch_gemm -> launch_plan; kernels gemm_nt_kernel :106, gemm_nt_pre64 :376, gemm_nt_fast :822, gemm_nt_small :939.
// Reads A [m, k], B [n, k] and, if beta != 0, C; writes C [m, n] (epi 0; c_lower declared as the whole rectangle), the projection
// partials part [2 * ceil(n / 128), m] per batch entry and C2 [m, c2_cols] (epi 1), stat_sumsq [m] and stat_mv [m, stat_P].
// Every kernel stores sig_val to sig_ptr on entry (:113, :380, :824, :964); only gemm_nt_small waits for wait_ptr (:966) and may then
// store INT_MAX to wait_info.
// One record stands for what launch_plan (gemm.hip:1060) issues: a capped fast launch with a tail split is followed by a second, generic
// launch for the tail tiles ON THE SAME STREAM with the same arguments (same sig_ptr and value), and the tile-queue form also reads and
// advances a device counter slot that only launches of that form, stream-ordered, touch -- neither adds an edge or a shared rectangle.
// wgs / lds: the plan's grid and LDS request (what a waiting kernel holds while it waits).
static const char* gemm_kernel_name(GemmKernel k) {
  switch (k) {
    case GemmKernel::small: return "gemm.small";
    case GemmKernel::pre64: return "gemm.pre64";
    case GemmKernel::generic: return "gemm.generic";
    case GemmKernel::fast: return "gemm.fast";
    default: return "gemm.none";
  }
}
int gpk_launch_gemm(hipStream_t s, const GemmArgs& a) {
  const GemmPlan p = make_gemm_plan(a);
  if (p.kernel == GemmKernel::none) return 0;
  if (p.kernel == GemmKernel::unsupported) return GPK_E_UNSUPPORTED;
  Launch l(s, gemm_kernel_name(p.kernel));
  l.d("m=%d n=%d k=%d batch=%d c_lower=%d b_tri=%d epi=%d", a.m, a.n, a.k, a.batch, a.c_lower, a.b_tri, a.epi);
  l.R(a.A, a.m, a.k, a.lda, a.batch, a.strideA).R(a.B, a.n, a.k, a.ldb, a.batch, a.strideB);
  if (a.beta != 0.0) l.R(a.C, a.m, a.n, a.ldc, a.batch, a.strideC);
  if (a.epi == 0) l.W(a.C, a.m, a.n, a.ldc, a.batch, a.strideC);
  else {
    l.W(a.part, 2 * gemm_cdiv(a.n, 128), a.m, a.part_ld, a.batch, a.stridePart);
    if (a.c2_cols > 0) l.W(a.C2, a.m, a.c2_cols, a.ldc2, a.batch, a.strideC2);
  }
  if (a.stat_sumsq) l.vecW(a.stat_sumsq, a.m).vecW(a.stat_mv, (long)a.m * a.stat_P).vecR(a.stat_V, (long)a.k * a.stat_P);
  l.wgs = (long)p.grid_x * p.grid_y * p.grid_z; l.lds = (long)p.lds_bytes;
  if (a.sig_ptr) { l.sig_ptr = a.sig_ptr; l.sig_val = a.sig_val; l.sig_on_entry = true; }
  if (a.wait_ptr) {
    if (p.kernel == GemmKernel::small) { l.wait_ptr = a.wait_ptr; l.wait_val = a.wait_val; l.status("may", a.wait_info); }
    else l.wait_dropped = true;
  }
  return l.emit();
}
bool gpk_gemm_takes_latency_kernel(const GemmArgs& a) { return make_gemm_plan(a).kernel == GemmKernel::small; }   // gemm.hip:1115, verbatim
bool gpk_gemm_fuses_row_stats(const GemmArgs& a) {                                                                // gemm.hip:1116, verbatim
  const GemmPlan p = make_gemm_plan(a);
  return p.kernel == GemmKernel::fast && p.sp;
}
int gpk_gemm_tiles_n(int n) { return gpk_cdiv(n, 128); }   // gemm.hip:1114, verbatim
// group_solve.hip:364: group_solve_choice(1, 1, 0, true).pipelined, which is GPK_TUNE(GROUP_SOLVE_V2, 1) for a partial solve (:355)
bool gpk_group_solve_takes_parts() { return GPK_TUNE(GROUP_SOLVE_V2, 1) != 0; }

// leaf.hip:85 gpk_launch_leaf: leaf2_kernel :35 (leaf2_device.h) factors the nb x nb block in place and writes its inverse [NB, NB];
// the status word is reset by the leaf of column 0 and read-modified by the others (leaf2_device.h:647-657).  already_factored:
// leaf_kernel :27 reads the block and writes the inverse only.
int gpk_launch_leaf(hipStream_t s, double* A, long lda, long strideA, int nb, double* invd, long strideInv, int* info, int col0, int batch,
                    int already_factored) {
  if (nb <= 0 || nb > GPK_NB) return GPK_E_ARG;
  Launch l(s, already_factored ? "leaf.inverse" : "leaf");
  l.d("col0=%d nb=%d batch=%d", col0, nb, batch);
  l.R(A, nb, nb, lda, batch, strideA).W(invd, GPK_NB, GPK_NB, GPK_NB, batch, strideInv);
  if (!already_factored) {
    l.W(A, nb, nb, lda, batch, strideA);
    l.status(col0 == 0 ? "reset" : "rmw", info);
  }
  return l.emit();
}

// group_solve.hip:366 gpk_launch_group_solve: group_solve_kernel :30 / group_solve2_kernel :157.  Blocks [j0, j1) of the group are
// solved with their inverses X_j and every later block of the group gets their update: reads E[:, 0 : nb NB] (a superset for a partial
// solve), L[j0 NB : nb NB, j0 NB : j1 NB] -- for the whole group the block rows of its lower triangle -- and X[j0 : j1]; writes
// Eo[:, j0 NB : nb NB] (:338: a partial launch hands the updated, unsolved blocks back).
int gpk_launch_group_solve(hipStream_t s, const double* E, long lde, double* Eo, long ldeo, int rows, const double* Lgg, long ldl, const double* X,
                           int nb, int batch, long strideE, long strideEo, long strideL, long strideX, int max_wgs, int j0, int j1) {
  (void)max_wgs;
  if (rows <= 0) return 0;
  if (j1 < 0) j1 = nb;
  if (j0 < 0 || j0 >= j1 || j1 > nb) return GPK_E_ARG;
  const bool partial = j0 > 0 || j1 < nb;
  if (partial && (E != Eo || lde != ldeo || strideE != strideEo || !gpk_group_solve_takes_parts())) return GPK_E_UNSUPPORTED;
  if (batch < 1) batch = 1;
  if (!E || !Eo || !Lgg || !X || nb < 1 || nb > 4) return GPK_E_ARG;
  if ((ldl & 1) || (reinterpret_cast<uintptr_t>(Lgg) & 15) || (reinterpret_cast<uintptr_t>(X) & 15)) return GPK_E_UNSUPPORTED;
  if (batch > 1 && ((strideL & 1) || (strideX & 1))) return GPK_E_UNSUPPORTED;
  const long NBl = GPK_NB;
  Launch l(s, partial ? "group_solve.part" : "group_solve");
  l.d("rows=%d nb=%d j0=%d j1=%d batch=%d", rows, nb, j0, j1, batch);
  l.R(E, rows, nb * NBl, lde, batch, strideE);
  if (partial) l.R(Lgg + j0 * NBl * ldl + j0 * NBl, (nb - j0) * NBl, (j1 - j0) * NBl, ldl, batch, strideL);
  else
    for (int i = 0; i < nb; ++i) l.R(Lgg + i * NBl * ldl, NBl, (i + 1) * NBl, ldl, batch, strideL);
  l.R(X + j0 * NBl * NBl, (j1 - j0) * NBl, NBl, NBl, batch, strideX);
  l.W(Eo + j0 * NBl, rows, (nb - j0) * NBl, ldeo, batch, strideEo);
  return l.emit();
}

// rowops.hip:159 set_identity_kernel :139 (writes the n x n block), :167 zero_upper_kernel :7 (writes above the diagonal: declared as
// the whole square)
int gpk_launch_set_identity(hipStream_t s, double* A, int n, long lda, int batch, long strideA) {
  if (n <= 0) return 0;
  return Launch(s, "set_identity").d("n=%d", n).W(A, n, n, lda, batch, strideA).emit();
}
int gpk_launch_zero_upper(hipStream_t s, double* A, int n, long lda, int batch, long strideA) {
  if (n <= 1) return 0;
  return Launch(s, "zero_upper").d("n=%d", n).W(A, n, n, lda, batch, strideA).emit();
}

// sync.hip:37 wait_flag_kernel :21 (one-wave gate; INT_MAX to info when its bound expires), :42 set_flag_kernel :33 (the store is the
// kernel: it carries everything queued before it on its stream), :7 noop_kernel
int gpk_launch_wait_flag(hipStream_t s, const int* ptr, int val, int* info) {
  Launch l(s, "wait_flag");
  l.wait_ptr = ptr; l.wait_val = val;
  return l.status("may", info).emit();
}
int gpk_launch_set_flag(hipStream_t s, int* ptr, int val) {
  Launch l(s, "set_flag");
  l.sig_ptr = ptr; l.sig_val = val;
  return l.emit();
}
int gpk_launch_noop(hipStream_t s) { return Launch(s, "noop").emit(); }
// sync.hip:61: answers what the command line says (conc=0 is how the runner reaches flags_usable = 0)
int gpk_probe_concurrent_kernels(hipStream_t, hipStream_t, int*, int* concurrent) { *concurrent = rec::g_concurrent; return 0; }

// rbf.hip:240 gpk_kernel_matrix, rbf_kernel :76: reads X1 [n1, d] (and X2 [n2, d]), writes K [n1, n2] (lower_only: declared whole)
extern "C" int gpk_kernel_matrix(void* stream, int, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d,
                                 const double* ls_host, int, double, double, int lower_only, double* K, long ldk) {
  if (!ls_host || n1 < 0 || (X2 && n2 < 0) || d <= 0 || d > GPK_MAX_D) return GPK_E_ARG;
  if (n1 == 0 || (X2 && n2 == 0)) return 0;
  if (!X1 || !K) return GPK_E_ARG;
  Launch l((hipStream_t)stream, X2 ? "kernel_matrix.cross" : "kernel_matrix.sym");
  l.d("n1=%d n2=%d lower_only=%d", n1, X2 ? n2 : n1, lower_only).R(X1, n1, d, ldx1);
  if (X2) l.R(X2, n2, d, ldx2);
  return l.W(K, n1, X2 ? n2 : n1, ldk).emit();
}
// rowops.hip:152 diag_add_kernel :148: A[i, i] += v[i] (declared as the whole square)
extern "C" int gpk_diag_add(void* stream, double* A, int n, long lda, const double* v) {
  if (!A || !v || n < 0 || lda < n) return GPK_E_ARG;
  if (n == 0) return 0;
  return Launch((hipStream_t)stream, "diag_add").R(A, n, n, lda).W(A, n, n, lda).vecR(v, n).emit();
}
// rowops.hip:177 transpose_kernel :15: out [cols, rows] = in [rows, cols]^T per batch entry
extern "C" int gpk_transpose(void* stream, const double* in, int rows, int cols, long ldin, double* out, long ldout, int mode, int batch,
                             long stride_in, long stride_out) {
  if (rows < 0 || cols < 0) return GPK_E_ARG;
  if (rows == 0 || cols == 0) return 0;
  if (!in || !out) return GPK_E_ARG;
  return Launch((hipStream_t)stream, "transpose").d("rows=%d cols=%d mode=%d batch=%d", rows, cols, mode, batch)
      .R(in, rows, cols, ldin, batch, stride_in).W(out, cols, rows, ldout, batch, stride_out).emit();
}
// rowops.hip:237 transpose_shift_kernel :40
int gpk_launch_transpose_shift(hipStream_t s, const double* in, int rows, int cols, long ldin, double* out, long ldout, double) {
  if (rows == 0 || cols == 0) return 0;
  return Launch(s, "transpose_shift").R(in, rows, cols, ldin).W(out, cols, rows, ldout).emit();
}
// rowops.hip:192 row_stats_kernel :60 (one launch per four latents): reads At [rows, m], V and W [m, P]; writes sumsq [rows] (read
// first if beta != 0), mv [rows, P], wsq [P, rows]
extern "C" int gpk_row_stats(void* stream, const double* At, int rows, int m, long ldat, const double* V, const double* W, int P, double,
                             double beta, double* sumsq, double* mv, double* wsq) {
  if (rows < 0 || m < 0) return GPK_E_ARG;
  if (rows == 0) return 0;
  if (!At) return GPK_E_ARG;
  const int np = (V || W) ? P : 0;
  Launch l((hipStream_t)stream, "row_stats");
  l.d("rows=%d m=%d P=%d", rows, m, np).R(At, rows, m, ldat).vecR(V, (long)m * np).vecR(W, (long)m * np);
  if (beta != 0.0) l.vecR(sumsq, rows);
  l.vecW(sumsq, rows);
  if (V) l.vecW(mv, (long)rows * np);
  if (W) l.vecW(wsq, (long)rows * np);
  return l.emit();
}
extern "C" int gpk_row_sumsq(void* stream, const double* A, int rows, int cols, long lda, double alpha, double beta, double* out) {   // rowops.hip:231
  return gpk_row_stats(stream, A, rows, cols, lda, nullptr, nullptr, 0, alpha, beta, out, nullptr, nullptr);
}
// rowops.hip:210 row_stats_sep_kernel :102
int gpk_launch_row_stats_sep(hipStream_t s, const double* At, long strideAt, int rows, int m, long ldat, const double* V, int P, double* sumsq,
                             double* mv) {
  if (!At || !V || !sumsq || !mv || rows < 0 || m < 0 || P <= 0) return GPK_E_ARG;
  if (rows == 0) return 0;
  return Launch(s, "row_stats_sep").R(At, rows, m, ldat, P, strideAt).vecR(V, (long)m * P).vecW(sumsq, (long)P * rows).vecW(mv, (long)rows * P).emit();
}

// reduce.hip:160 sum_parts_kernel :25: ssq[p, b] = sum over the nt slots part[p][t][b]
int gpk_launch_sum_parts(hipStream_t s, const double* part, int nt, int rows, long stridePart, int P, double* ssq) {
  if (rows == 0 || P == 0) return 0;
  return Launch(s, "sum_parts").R(part, nt, rows, rows, P, stridePart).vecW(ssq, (long)P * rows).emit();
}
// reduce.hip:193 final_sum_kernel :12: out[0] from part[t][0 : count[t]]
int gpk_launch_final(hipStream_t s, int nterms, const double* const* part, const int* count, const double*, double, double* out) {
  Launch l(s, "final");
  for (int t = 0; t < nterms; ++t) l.vecR(part[t], count[t]);
  return l.vecW(out, 1).emit();
}
int gpk_launch_final_one(hipStream_t s, const double* part, int count, double scale, double add, double* out) {   // reduce.hip:204
  return gpk_launch_final(s, 1, &part, &count, &scale, add, out);
}
static int blocks_for(long elems) {   // (reduce_device.h nblocks_for: at most GPK_REDUCE_MAXPART partials; the count only sizes `part`)
  const long nb = (elems + 255) / 256;
  return (int)(nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb));
}
// reduce.hip:209 sumsq_kernel :141
int gpk_launch_sumsq_stage1(hipStream_t s, const double* A, int rows, int cols, long lda, int, double* part, int* count) {
  int nb = rows < GPK_REDUCE_MAXPART ? rows : GPK_REDUCE_MAXPART;
  if (nb < 1) nb = 1;
  *count = nb;
  return Launch(s, "sumsq_stage1").R(A, rows, cols, lda).vecW(part, nb).emit();
}
// reduce.hip:218 kl_white_kernel :88: also zeroes *zero_word (:92), the ticket of the shard's one-launch tail
int gpk_launch_kl_white_stage1(hipStream_t s, const double* q_mu, const double* q_sqrt, int m, int P, int q_diag, double* part, int* count,
                               int* zero_word) {
  const long elems = q_diag ? (long)m * P : (long)P * m * m;
  *count = blocks_for(elems);
  return Launch(s, "kl_white_stage1").vecR(q_mu, (long)m * P).vecR(q_sqrt, elems).vecW(part, *count).mat('W', zero_word, 1, 1, 1, 1, 0, 4).emit();
}
// reduce.hip:281 kl_unwhite_diag_kernel :257
int gpk_launch_kl_unwhite_diag_stage1(hipStream_t s, const double* LinvT, long ldl, int m, const double* W, int P, double* part, int* count) {
  *count = m < GPK_REDUCE_MAXPART ? m : GPK_REDUCE_MAXPART;
  return Launch(s, "kl_unwhite_diag_stage1").R(LinvT, m, m, ldl).vecR(W, (long)m * P).vecW(part, *count).emit();
}
// reduce.hip:290 sum_log_diag_sq_kernel :131, :246 sum_log_diag_kernel :119 (the diagonal: declared as the whole square)
int gpk_launch_sum_log_diag_sq(hipStream_t s, const double* L, int n, long ldl, int batch, long strideL, double* out) {
  if (!L || !out || n <= 0) return GPK_E_ARG;
  return Launch(s, "sum_log_diag_sq").R(L, n, n, ldl, batch, strideL).vecW(out, batch > 0 ? batch : 1).emit();
}
extern "C" int gpk_sum_log_diag(void* stream, const double* L, int n, long ldl, int batch, long strideL, double* out) {
  if (!L || !out || n <= 0) return GPK_E_ARG;
  return Launch((hipStream_t)stream, "sum_log_diag").R(L, n, n, ldl, batch, strideL).vecW(out, batch > 0 ? batch : 1).emit();
}

// varexp.hip:317 (verbatim), :324 varexp_kernel<false> :34, :333 varexp_kernel<true> (sums the slots, one partial per block, the last
// block by the ticket sums them into out[0]), :398 the quadrature stage (:152, :241)
LatentMoments gpk_latent_moments(const double* Y, long ldy, const double* fmean, int rows, int P, const double* s0, int s0_per_latent,
                                 const double* ssq, const double* knn_host, int knn_per_latent, double mean_const, double* fvar_out) {
  LatentMoments m{Y, ldy, fmean, rows, P, s0, s0_per_latent, ssq, {}, knn_per_latent, mean_const, fvar_out};
  for (int i = 0; i < (knn_per_latent ? P : 1); ++i) m.knn[i] = knn_host[i];
  return m;
}
static Launch& moments(Launch& l, const LatentMoments& m, bool with_ssq) {
  l.R(m.Y, m.rows, m.P, m.ldy).vecR(m.fmean, (long)m.rows * m.P).vecR(m.s0, (long)m.rows * (m.s0_per_latent ? m.P : 1));
  if (with_ssq) l.vecR(m.ssq, (long)m.rows * m.P);
  return l.vecW(m.fvar_out, (long)m.rows * m.P);
}
int gpk_launch_varexp_stage1(hipStream_t s, const LatentMoments& m, double, const double* noise_rows, double* part, int* count) {
  *count = blocks_for((long)m.rows * m.P);
  Launch l(s, "varexp_stage1");
  return moments(l, m, true).vecR(noise_rows, m.rows).vecW(part, *count).emit();
}
int gpk_launch_varexp_tail(hipStream_t s, const LatentMoments& m, const double* slot, int nt, long strideSlot, double, const double* noise_rows,
                           double* part, int* ticket, double* out) {
  if (!slot || !part || !ticket || !out || nt < 0) return GPK_E_ARG;
  Launch l(s, "varexp_tail");
  moments(l, m, false).R(slot, nt, m.rows, m.rows, m.P, strideSlot).vecR(noise_rows, m.rows).vecW(part, blocks_for((long)m.rows * m.P));
  return l.vecR(part, blocks_for((long)m.rows * m.P)).mat('R', ticket, 1, 1, 1, 1, 0, 4).mat('W', ticket, 1, 1, 1, 1, 0, 4).vecW(out, 1).emit();
}
int gpk_likelihood_check(int, const double*, int) { return 0; }
int gpk_launch_likelihood_varexp_stage1(hipStream_t s, int, const double*, const LatentMoments& m, double* rows_out, double* dmu_out,
                                        double* dvar_out, double* part, double* part1, int* count) {
  *count = blocks_for((long)m.rows * m.P);
  Launch l(s, "likelihood_varexp_stage1");
  moments(l, m, true).vecW(rows_out, m.rows).vecW(dmu_out, (long)m.rows * m.P).vecW(dvar_out, (long)m.rows * m.P);
  return l.vecW(part, *count).vecW(part1, *count).emit();
}

// ---- the command line -------------------------------------------------------------------------------------------------------------
namespace {
struct Opts {
  std::string entry, layout = "a";
  int n = 0, extra = 0, rows = 0, P = 1, batch = 1, whiten = 1, q_diag = 0, reps = 2, zero_upper = 1, d = 8;
};
struct Named { const void* p; size_t bytes; };
std::vector<Named> g_bufs;   // what the caller's own launches around each call touch
double* buf(const char* name, size_t elems, size_t misalign = 0) {
  double* p = (double*)rec::region(name, elems * sizeof(double) + misalign, misalign);
  g_bufs.push_back(Named{p, elems * sizeof(double)});
  return p;
}
// the caller's own work on its stream in front of the first call and behind every call: it touches every operand
void caller_touches(const char* name) {
  Launch l(&rec::g_caller, name);
  for (const Named& b : g_bufs) l.mat('W', b.p, 1, (long)b.bytes, (long)b.bytes, 1, 0, 1);
  l.emit();
}
long even_up(long x) { return (x + 7) / 8 * 8; }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  Opts o;
  o.entry = argv[1];
  for (int i = 2; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) return 2;
    const std::string key(argv[i], eq - argv[i]);
    const int v = atoi(eq + 1);
    if (key == "layout") o.layout = eq + 1;
    else if (key == "n") o.n = v;
    else if (key == "extra") o.extra = v;
    else if (key == "rows") o.rows = v;
    else if (key == "P") o.P = v;
    else if (key == "batch") o.batch = v;
    else if (key == "whiten") o.whiten = v;
    else if (key == "q_diag") o.q_diag = v;
    else if (key == "reps") o.reps = v;
    else if (key == "zero_upper") o.zero_upper = v;
    else if (key == "conc") rec::g_concurrent = v;
    else return 2;
  }
  const bool odd = o.layout == "odd", p8 = o.layout == "p8";
  if (!odd && !p8 && o.layout != "a") return 2;
  hipStream_t S = &rec::g_caller;
  rec::line("{\"k\":\"stream\",\"s\":0,\"kind\":\"caller\"}");
  rec::line("{\"k\":\"device\",\"cus\":256,\"lds\":163840}");   // what hipGetDeviceProperties answers above; LDS of a compute unit
  const int n = o.n, P = o.P, d = o.d;
  int* info = (int*)buf("info", 8);
  static const double ls[64 * 16] = {1.0};
  static const double var[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
  static const int fam[16] = {0};
  static const double likp[16] = {1.0};
  std::function<int()> call;
  if (o.entry == "potrf" || o.entry == "potrf_inv") {
    const bool inv = o.entry == "potrf_inv";
    const long rows_all = (long)n + o.extra + (inv ? n : 0);
    const long lda = odd ? (n | 1) : even_up(n);
    long stride = rows_all * lda;
    if (odd && !(stride & 1)) ++stride;
    const int batch = inv ? 1 : o.batch;
    double* A = buf("A", (size_t)stride * batch, p8 ? 8 : 0);
    double* invd = buf("invd", gpk_invd_elems(n, batch));
    if (inv) call = [=] { return gpk_potrf_inv(S, A, n, o.extra, lda, invd, o.zero_upper, info); };
    else call = [=] { return gpk_potrf(S, A, n, o.extra, lda, batch, stride, invd, o.zero_upper, info); };
  } else if (o.entry == "trsm0" || o.entry == "trsm1") {
    const long ldl = odd ? (n | 1) : even_up(n);
    long strideL = (long)n * ldl, strideB = (long)o.extra * ldl;
    if (odd) { strideL |= 1; strideB |= 1; }
    const double* L = buf("L", (size_t)strideL * o.batch, p8 ? 8 : 0);
    const double* invd = buf("invd", gpk_invd_elems(n, o.batch));
    double* B = buf("B", (size_t)strideB * o.batch, p8 ? 8 : 0);
    const int trans = o.entry == "trsm1";
    call = [=] { return gpk_trsm(S, trans, L, ldl, invd, n, B, o.extra, ldl, o.batch, strideL, strideB); };
  } else if (o.entry == "gpr_lml") {
    const double* X = buf("X", (size_t)n * d);
    const double* Y = buf("Y", (size_t)n * P);
    double* out = buf("out", 2);
    const size_t wsb = gpk_gpr_lml_workspace_bytes(n, d, P);
    void* ws = buf("ws", wsb / 8);
    call = [=] { return gpk_gpr_lml(S, 0, X, n, d, d, Y, P, P, ls, 0, 1.0, 0.1, nullptr, 0.0, out, info, ws, wsb); };
  } else if (o.entry == "svgp" || o.entry == "svgp_lik" || o.entry == "svgp_sep") {
    const bool sep = o.entry == "svgp_sep";
    const double* Z = buf("Z", (size_t)n * d * (sep ? P : 1));
    const double* Xb = buf("Xb", (size_t)o.rows * d + 1);
    const double* Yb = buf("Yb", (size_t)o.rows * P + 1);
    const double* q_mu = buf("q_mu", (size_t)n * P);
    const double* q_sqrt = buf("q_sqrt", o.q_diag ? (size_t)n * P : (size_t)P * n * n);
    double* out = buf("out", 2);
    if (sep) {
      const size_t wsb = gpk_svgp_elbo_sep_workspace_bytes(n, o.rows, d, P);
      void* ws = buf("ws", wsb / 8);
      call = [=] {
        return gpk_svgp_elbo_shard_sep(S, fam, Z, n, d, (long)n * d, Xb, Yb, o.rows, d, P, d, P, ls, 0, var, 0.1, nullptr, 1e-6, 0.0, q_mu, q_sqrt,
                                       out, info, ws, wsb);
      };
    } else {
      const size_t wsb = gpk_svgp_elbo_workspace_bytes(n, o.rows, d, P, o.q_diag, o.whiten);
      void* ws = buf("ws", wsb / 8);
      if (o.entry == "svgp")
        call = [=] {
          return gpk_svgp_elbo_shard(S, 0, Z, n, d, Xb, Yb, o.rows, d, P, d, P, ls, 0, 1.0, 0.1, nullptr, 1e-6, 0.0, q_mu, q_sqrt, o.q_diag,
                                     o.whiten, out, info, ws, wsb);
        };
      else
        call = [=] {
          return gpk_svgp_elbo_shard_lik(S, 0, Z, n, d, Xb, Yb, o.rows, d, P, d, P, ls, 0, 1.0, 1, likp, 1e-6, 0.0, q_mu, q_sqrt, o.q_diag,
                                         o.whiten, out, info, ws, wsb);
        };
    }
  } else return 2;
  caller_touches("caller_before");
  for (int r = 0; r < o.reps; ++r) {
    rec::line("{\"k\":\"call\",\"i\":%d}", r);
    const int rc = call();
    rec::line("{\"k\":\"call_end\",\"i\":%d,\"rc\":%d}", r, rc);
    if (rc) return 3;
    caller_touches("caller_next");
  }
  return 0;
}
