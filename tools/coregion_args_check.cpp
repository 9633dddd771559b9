// Stand-alone host program: every argument refusal of the gpk_coregion_* entry points (include/gpk.h, "Coregion kernel"), called with
// host buffers and NULLs.  No call here reaches a launch, so it needs no device; it is meant to be built with the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         gpflow_amd/csrc/coregion/coregion.hip tools/coregion_args_check.cpp -o /tmp/coregion_args_check && /tmp/coregion_args_check
//
// Exit status 0 and "ok" when every answer is the documented one and no buffer was written.
#include <cstdio>
#include <vector>
#include "../include/gpk.h"

static int failures = 0;
#define EXPECT(call, want)                                                          \
  do {                                                                              \
    const int got__ = (call);                                                       \
    if (got__ != (want)) {                                                          \
      std::printf("%s:%d: %s -> %d, expected %d\n", __FILE__, __LINE__, #call, got__, (want)); \
      ++failures;                                                                   \
    }                                                                               \
  } while (0)

int main() {
  std::vector<double> buf(64 * 64, -555.0);
  double* p = buf.data();
  const int E = GPK_E_ARG;
  // output covariance: P, R out of range, short leading dimensions, NULL operands
  for (int P : {0, -1, 65}) EXPECT(gpk_coregion_output_covariance(nullptr, p, 2, p, P, 2, p, 65), E);
  for (int R : {0, -3, 65}) EXPECT(gpk_coregion_output_covariance(nullptr, p, 65, p, 3, R, p, 3), E);
  EXPECT(gpk_coregion_output_covariance(nullptr, p, 1, p, 3, 2, p, 3), E);
  EXPECT(gpk_coregion_output_covariance(nullptr, p, 2, p, 3, 2, p, 2), E);
  EXPECT(gpk_coregion_output_covariance(nullptr, nullptr, 2, p, 3, 2, p, 3), E);
  EXPECT(gpk_coregion_output_covariance(nullptr, p, 2, nullptr, 3, 2, p, 3), E);
  EXPECT(gpk_coregion_output_covariance(nullptr, p, 2, p, 3, 2, nullptr, 3), E);
  // builder
  for (int P : {0, -1, 65}) EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 1, p, 5, 1, p, 65, P, 0.0, 0, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, -1, 1, p, 5, 1, p, 3, 3, 0.0, 0, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 1, p, -1, 1, p, 3, 3, 0.0, 0, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 0, p, 5, 1, p, 3, 3, 0.0, 0, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 1, p, 5, 0, p, 3, 3, 0.0, 0, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 1, p, 5, 1, p, 2, 3, 0.0, 0, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 1, p, 7, 1, p, 3, 3, 0.0, 0, p, 6), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 1, nullptr, 0, 0, p, 3, 3, 0.0, 0, p, 4), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, nullptr, 5, 1, p, 5, 1, p, 3, 3, 0.0, 0, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 1, p, 5, 1, nullptr, 3, 3, 0.0, 0, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, p, 5, 1, p, 5, 1, p, 3, 3, 0.0, 0, nullptr, 5), E);
  EXPECT(gpk_coregion_kernel_matrix(nullptr, nullptr, 0, 1, p, 5, 1, nullptr, 3, 3, 0.0, 0, nullptr, 5), 0);   // nothing to do
  // combine
  for (int op : {0, 3, -1}) EXPECT(gpk_coregion_kernel_matrix_combine(nullptr, op, p, 5, 1, p, 5, 1, p, 3, 3, 0.0, p, 5, p, 5), E);
  for (int P : {0, 65}) EXPECT(gpk_coregion_kernel_matrix_combine(nullptr, 1, p, 5, 1, p, 5, 1, p, 65, P, 0.0, p, 5, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix_combine(nullptr, 1, p, 5, 1, p, 7, 1, p, 3, 3, 0.0, p, 6, p, 7), E);
  EXPECT(gpk_coregion_kernel_matrix_combine(nullptr, 2, p, 5, 1, p, 7, 1, p, 3, 3, 0.0, p, 7, p, 6), E);
  EXPECT(gpk_coregion_kernel_matrix_combine(nullptr, 1, p, 5, 1, p, 5, 1, p, 3, 3, 0.0, nullptr, 5, p, 5), E);
  EXPECT(gpk_coregion_kernel_matrix_combine(nullptr, 1, p, 5, 1, p, 5, 1, p, 3, 3, 0.0, p, 5, nullptr, 5), E);
  EXPECT(gpk_coregion_kernel_matrix_combine(nullptr, 1, p, 5, 1, p, 0, 1, p, 3, 3, 0.0, nullptr, 1, nullptr, 1), 0);
  // row diagonal
  for (int op : {-1, 3}) EXPECT(gpk_coregion_kernel_diag(nullptr, op, p, 5, 1, p, 3, 3, p, p), E);
  EXPECT(gpk_coregion_kernel_diag(nullptr, 0, p, -1, 1, p, 3, 3, p, p), E);
  EXPECT(gpk_coregion_kernel_diag(nullptr, 0, p, 5, 0, p, 3, 3, p, p), E);
  EXPECT(gpk_coregion_kernel_diag(nullptr, 0, p, 5, 1, p, 2, 3, p, p), E);
  EXPECT(gpk_coregion_kernel_diag(nullptr, 1, p, 5, 1, p, 3, 3, nullptr, p), E);
  EXPECT(gpk_coregion_kernel_diag(nullptr, 0, p, 5, 1, p, 3, 3, nullptr, nullptr), E);
  EXPECT(gpk_coregion_kernel_diag(nullptr, 0, nullptr, 0, 1, nullptr, 3, 3, nullptr, nullptr), 0);
  // one-hot rows
  for (int P : {0, 65}) EXPECT(gpk_coregion_onehot_rows(nullptr, p, 5, 1, P, p, 5), E);
  EXPECT(gpk_coregion_onehot_rows(nullptr, p, -1, 1, 3, p, 5), E);
  EXPECT(gpk_coregion_onehot_rows(nullptr, p, 5, 0, 3, p, 5), E);
  EXPECT(gpk_coregion_onehot_rows(nullptr, p, 5, 1, 3, p, 4), E);
  EXPECT(gpk_coregion_onehot_rows(nullptr, nullptr, 5, 1, 3, p, 5), E);
  EXPECT(gpk_coregion_onehot_rows(nullptr, p, 5, 1, 3, nullptr, 5), E);
  EXPECT(gpk_coregion_onehot_rows(nullptr, nullptr, 0, 1, 3, nullptr, 1), 0);
  // adjoint tail
  for (int P : {0, 65}) EXPECT(gpk_coregion_adjoint_tail(nullptr, p, 65, p, 2, P, 2, p, 2, p), E);
  for (int R : {0, 65}) EXPECT(gpk_coregion_adjoint_tail(nullptr, p, 3, p, 65, 3, R, p, 65, p), E);
  EXPECT(gpk_coregion_adjoint_tail(nullptr, p, 2, p, 2, 3, 2, p, 2, p), E);
  EXPECT(gpk_coregion_adjoint_tail(nullptr, p, 3, p, 1, 3, 2, p, 2, p), E);
  EXPECT(gpk_coregion_adjoint_tail(nullptr, p, 3, p, 2, 3, 2, p, 1, p), E);
  EXPECT(gpk_coregion_adjoint_tail(nullptr, nullptr, 3, p, 2, 3, 2, p, 2, p), E);
  EXPECT(gpk_coregion_adjoint_tail(nullptr, p, 3, nullptr, 2, 3, 2, p, 2, p), E);
  EXPECT(gpk_coregion_adjoint_tail(nullptr, p, 3, p, 2, 3, 2, nullptr, 2, p), E);
  EXPECT(gpk_coregion_adjoint_tail(nullptr, p, 3, p, 2, 3, 2, p, 2, nullptr), E);
  for (double v : buf)
    if (v != -555.0) {
      std::printf("a refused call wrote\n");
      ++failures;
      break;
    }
  std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
