// The label rule of the kernels that read a column of task / output labels (coregion/coregion.hip, switched/switched_varexp.hip).
#pragma once

namespace {
// the label of a row, or -1 for an invalid one.  The DOUBLE is tested (both comparisons are false for a NaN); only a value inside
// (-1, P) is converted, and the conversion truncates toward zero.
__device__ __forceinline__ int label_of(double x, int P) { return (x > -1.0 && x < (double)P) ? (int)x : -1; }
}  // namespace
