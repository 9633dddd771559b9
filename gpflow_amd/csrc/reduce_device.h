// Fixed-order wave and block sums and the block count of a stage-1 reduction, shared by reduce.hip, rowops.hip and varexp.hip.
#pragma once
#include "gpk_internal.h"

namespace {
constexpr int RB = 256;       // threads per reduction block

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}
// valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int i = 0; i < nw; ++i) r += sh[i];
  }
  return r;
}

int nblocks_for(long elems) {
  long b = (elems + RB * 4 - 1) / (RB * 4);
  if (b < 1) b = 1;
  if (b > GPK_REDUCE_MAXPART) b = GPK_REDUCE_MAXPART;
  return (int)b;
}
}  // namespace
