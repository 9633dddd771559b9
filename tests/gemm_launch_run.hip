// Runs GEMM calls through the library's INTERNAL launcher, gpk_launch_gemm, on the device: the GemmArgs fields that only the
// factorisation and the fused drivers set (max_wgs, tile_queue, tile64, small_loop, no_small, sig_ptr / wait_ptr, stat_*) are out of
// reach of the exported gpk_gemm_nt / gpk_project, so this program links the library's object files and calls the launcher itself
// (Makefile target build/gemm_launch_run; no export is added to libgpk.so).  tests/test_gpu_gemm_launch.py writes the operands, starts
// ONE process for its whole case list and checks what comes back.
//   gemm_launch_run @FILE      one case per line of FILE, the key=value words of tests/gemm_case_words.h, each with dir=PATH
// Per case, in PATH:  A.bin [m][k], B.bin [batch][n][k], C0.bin [batch][m][n] (cases with a C), V.bin [k][stat_P] (stats=1): raw
// little-endian fp64.  The operands are placed in device buffers with the leading dimensions of the plan dumper, every padding element
// NaN.  The call runs twice on fresh copies of its outputs (r = 1, 2) on a non-default stream; written back:
//   C_run<r>.bin [batch][m][n]   or, epi = 1,   part_run<r>.bin [batch][2 cdiv(n, 128)][m]   and, stats=1, sumsq_run<r>.bin [m], mv_run<r>.bin [m][stat_P].
// Printed per case: the plan (the dumper's format), then
//   sig_word W        the sig=1 word after run 1 (it held 0; the kernel stores 7)
//   wait_info W       the wait=1 status word after run 1 (0: the bounded wait did not expire).  The awaited word ALREADY holds the
//                     awaited value when the kernel starts: this program never launches a wait that is not satisfied.
//   pad_intact 0/1    the padding of C is still NaN, bit for bit, after both runs
//   inputs_intact 0/1 the device buffers of A, B and V, padding included, are bitwise what was uploaded
//   launch_ms T       run 1, launch to end of synchronisation
// and `end`; after the last case a record `total_ms T`.  The first HIP error or failed launch ends the program with a non-zero exit:
// nothing is started after it.
#include <chrono>
#include <cmath>
#include <cstdint>
#include "../gpflow_amd/csrc/gpk_internal.h"
#include "gemm_case_words.h"

#define RUN_HIP(call)                                                                                       \
  do {                                                                                                      \
    const hipError_t e__ = (call);                                                                          \
    if (e__ != hipSuccess) {                                                                                \
      fprintf(stderr, "gemm_launch_run: case %d: %s -> %s\n", g_case, #call, hipGetErrorString(e__));       \
      exit(1);                                                                                              \
    }                                                                                                       \
  } while (0)

static int g_case = -1;

static void die(const char* what, const std::string& arg) {
  fprintf(stderr, "gemm_launch_run: case %d: %s %s\n", g_case, what, arg.c_str());
  exit(2);
}

static std::vector<double> read_doubles(const std::string& path, size_t count) {
  std::vector<double> v(count);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) die("cannot open", path);
  const size_t got = count ? fread(v.data(), sizeof(double), count, f) : 0;
  const bool more = fgetc(f) != EOF;
  fclose(f);
  if (got != count || more) die("wrong size:", path);
  return v;
}

static void write_doubles(const std::string& path, const double* p, size_t count) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) die("cannot create", path);
  const size_t put = count ? fwrite(p, sizeof(double), count, f) : 0;
  if (fclose(f) != 0 || put != count) die("short write:", path);
}

// a host image and its device copy
struct Buf {
  std::vector<double> host;
  double* dev = nullptr;
  void alloc() {
    if (host.empty()) return;
    RUN_HIP(hipMalloc((void**)&dev, host.size() * sizeof(double)));
  }
  void upload() {
    if (dev) RUN_HIP(hipMemcpy(dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  std::vector<double> download() const {
    std::vector<double> out(host.size());
    if (dev) RUN_HIP(hipMemcpy(out.data(), dev, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    return out;
  }
  bool device_unchanged() const {
    const std::vector<double> now = download();
    return now.empty() || memcmp(now.data(), host.data(), now.size() * sizeof(double)) == 0;
  }
  void release() {
    if (dev) RUN_HIP(hipFree(dev));
    dev = nullptr;
  }
};

// [count][rows][cols] packed -> rows of ld doubles starting `off` doubles in, everything else NaN
static std::vector<double> padded(const std::vector<double>& packed, size_t count, size_t rows, size_t cols, size_t ld, size_t off = 0) {
  std::vector<double> out(count * rows * ld + off, std::nan(""));
  for (size_t r = 0; r < count * rows; ++r) memcpy(&out[off + r * ld], &packed[r * cols], cols * sizeof(double));
  return out;
}
static std::vector<double> packed(const std::vector<double>& img, size_t count, size_t rows, size_t cols, size_t ld) {
  std::vector<double> out(count * rows * cols);
  for (size_t r = 0; r < count * rows; ++r) memcpy(&out[r * cols], &img[r * ld], cols * sizeof(double));
  return out;
}
static bool padding_is(const std::vector<double>& img, const std::vector<double>& want, size_t count, size_t rows, size_t cols, size_t ld) {
  for (size_t r = 0; r < count * rows; ++r)
    if (memcmp(&img[r * ld + cols], &want[r * ld + cols], (ld - cols) * sizeof(double)) != 0) return false;
  return true;
}

static void run_case(hipStream_t stream, const GemmCase& c) {
  const GemmCaseLd l = gemm_case_ld(c);
  const size_t m = c.m, n = c.n, k = c.k, nb = c.batch > 0 ? c.batch : 1;
  const size_t P = c.stats ? gemm_case_stat_P(c) : 0, nt = 2 * (size_t)gemm_cdiv(c.n, 128);
  const bool has_c = gemm_case_has_c(c);
  if (c.dir.empty() || c.m <= 0 || c.n <= 0 || c.k <= 0) die("bad case", c.dir);
  const size_t a_off = c.align == 2 ? 1 : 0;   // (hipMalloc returns 256-byte aligned blocks)
  Buf A, B, C, V, part, sumsq, mv;
  A.host = padded(read_doubles(c.dir + "/A.bin", m * k), 1, m, k, l.lda, a_off);
  B.host = padded(read_doubles(c.dir + "/B.bin", nb * n * k), nb, n, k, l.ldb);
  if (has_c) C.host = padded(read_doubles(c.dir + "/C0.bin", nb * m * n), nb, m, n, l.ldc);
  if (c.epi == 1) part.host.assign(nb * nt * m, std::nan(""));
  if (c.stats) {
    V.host = read_doubles(c.dir + "/V.bin", k * P);
    sumsq.host.assign(m, std::nan(""));
    mv.host.assign(m * P, std::nan(""));
  }
  for (Buf* b : {&A, &B, &C, &V, &part, &sumsq, &mv}) b->alloc();
  for (Buf* b : {&A, &B, &V}) b->upload();
  int* words = nullptr;   // [0] the sig word, [1] the awaited word, [2] wait_info
  RUN_HIP(hipMalloc((void**)&words, 3 * sizeof(int)));

  GemmCaseMem mem;
  mem.A = A.dev + a_off; mem.B = B.dev; mem.C = C.dev; mem.part = part.dev;
  mem.stat_sumsq = sumsq.dev; mem.stat_mv = mv.dev; mem.stat_V = V.dev;
  mem.sig_ptr = words; mem.wait_ptr = words + 1; mem.wait_info = words + 2;
  const GemmArgs g = gemm_case_args(c, mem);
  const GemmPlan plan = make_gemm_plan(g);
  printf("case %d\n", g_case);
  gemm_plan_print(stdout, plan, c.m, c.n);
  if (plan.kernel == GemmKernel::none || plan.kernel == GemmKernel::unsupported) die("nothing to launch in", c.dir);

  bool pad_intact = true;
  int sig_word = 0, wait_info = 0;
  double launch_ms = 0.0;
  for (int r = 1; r <= 2; ++r) {
    for (Buf* b : {&C, &part, &sumsq, &mv}) b->upload();   // fresh outputs: C0, and NaN where the call must write
    const int init[3] = {0, kGemmCaseWaitVal, 0};          // the awaited word holds the awaited value BEFORE the launch
    RUN_HIP(hipMemcpy(words, init, sizeof init, hipMemcpyHostToDevice));
    RUN_HIP(hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = gpk_launch_gemm(stream, g);
    if (rc != 0) {
      fprintf(stderr, "gemm_launch_run: case %d: gpk_launch_gemm -> %d\n", g_case, rc);
      exit(1);
    }
    RUN_HIP(hipStreamSynchronize(stream));
    RUN_HIP(hipGetLastError());
    if (r == 1) launch_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const std::string tag = "_run" + std::to_string(r) + ".bin";
    if (has_c) {
      const std::vector<double> got = C.download();
      pad_intact = pad_intact && padding_is(got, C.host, nb, m, n, l.ldc);
      const std::vector<double> out = packed(got, nb, m, n, l.ldc);
      write_doubles(c.dir + "/C" + tag, out.data(), out.size());
    }
    if (c.epi == 1) {
      const std::vector<double> got = part.download();
      write_doubles(c.dir + "/part" + tag, got.data(), got.size());
    }
    if (c.stats) {
      const std::vector<double> s = sumsq.download(), v = mv.download();
      write_doubles(c.dir + "/sumsq" + tag, s.data(), s.size());
      write_doubles(c.dir + "/mv" + tag, v.data(), v.size());
    }
    if (r == 1) {
      int now[3];
      RUN_HIP(hipMemcpy(now, words, sizeof now, hipMemcpyDeviceToHost));
      sig_word = now[0]; wait_info = now[2];
    }
  }
  const bool inputs_intact = A.device_unchanged() && B.device_unchanged() && V.device_unchanged();
  printf("sig_word %d\nwait_info %d\npad_intact %d\ninputs_intact %d\nlaunch_ms %.3f\nend\n", sig_word, wait_info, pad_intact ? 1 : 0,
         inputs_intact ? 1 : 0, launch_ms);
  fflush(stdout);
  for (Buf* b : {&A, &B, &C, &V, &part, &sumsq, &mv}) b->release();
  RUN_HIP(hipFree(words));
}

int main(int argc, char** argv) {
  if (argc != 2 || argv[1][0] != '@') {
    fprintf(stderr, "usage: gemm_launch_run @FILE\n");
    return 2;
  }
  FILE* f = fopen(argv[1] + 1, "r");
  if (!f) die("cannot open", argv[1] + 1);
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t stream;
  RUN_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  char line[4096];
  while (fgets(line, sizeof line, f)) {
    ++g_case;
    GemmCase c;
    if (!gemm_case_parse(gemm_case_split(line), c)) die("bad words in line of", argv[1] + 1);
    run_case(stream, c);
  }
  fclose(f);
  RUN_HIP(hipStreamDestroy(stream));
  printf("total_ms %.1f\nend\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}
