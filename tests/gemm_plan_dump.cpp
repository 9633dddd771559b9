// Prints the launch plan of GEMM calls: tests/test_gemm_plan.py builds this with plain g++ (no ROCm include path -- which is the check
// that gemm_plan.h needs no HIP header) and reads the lines back.
//   gemm_plan_dump key=value ...     one call
//   gemm_plan_dump @FILE             one call per line of FILE (the same key=value words)
// The words, the leading dimensions and the plan format are those of tests/gemm_case_words.h, shared with the device runner
// (tests/gemm_launch_run.hip).  Pointers are fabricated: no memory is touched.  Each plan is printed as `key value` lines and a closing
// `end` line.
#include "gemm_case_words.h"

static int dump(const std::vector<std::string>& words) {
  GemmCase c;
  if (!gemm_case_parse(words, c)) return 2;
  // fabricated operands: 4 KiB-aligned addresses far apart
  const auto at = [](int i) { return (uintptr_t)i << 32; };
  GemmCaseMem mem;
  mem.A = reinterpret_cast<const double*>(at(1) + (c.align == 2 ? 8 : 0));
  mem.B = reinterpret_cast<const double*>(at(2));
  mem.C = reinterpret_cast<double*>(at(3));
  mem.part = reinterpret_cast<double*>(at(4));
  mem.stat_sumsq = reinterpret_cast<double*>(at(5));
  mem.stat_mv = reinterpret_cast<double*>(at(6));
  mem.stat_V = reinterpret_cast<const double*>(at(7));
  mem.sig_ptr = reinterpret_cast<int*>(at(8));
  mem.wait_ptr = reinterpret_cast<const int*>(at(9));
  mem.wait_info = reinterpret_cast<int*>(at(10));
  gemm_plan_print(stdout, make_gemm_plan(gemm_case_args(c, mem)), c.m, c.n);
  printf("end\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && argv[1][0] == '@') {
    FILE* f = fopen(argv[1] + 1, "r");
    if (!f) return 2;
    char line[4096];
    while (fgets(line, sizeof line, f)) {
      const int rc = dump(gemm_case_split(line));
      if (rc) return rc;
    }
    fclose(f);
    return 0;
  }
  return dump(std::vector<std::string>(argv + 1, argv + argc));
}
