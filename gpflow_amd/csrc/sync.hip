// Stream hand-offs and the host mailbox: the chain's flag kernels, the init-time concurrency probe, the empty kernel, publish_host.
#include "gpk_internal.h"

namespace {
__global__ void noop_kernel() {}
}  // namespace
int gpk_launch_noop(hipStream_t s) {
  hipLaunchKernelGGL(noop_kernel, dim3(1), dim3(64), 0, s);
  GPK_LAUNCH_CHECK();
  return 0;
}

// ---- gate / signal kernels of the chain flags (potrf.hip, round 6) ---------------------------------------------------------
// hipStreamWaitValue32 / hipStreamWriteValue32 run as the runtime's own one-workgroup kernels behind queue packets: 5 - 7 us
// each between two kernels of a stream (rocprofv3: __amd_rocclr_streamOpsWait / Write).  A kernel of ours that follows another
// on its stream starts 0.3 us later.  So a stream that has to wait for a flag word enqueues this gate -- one wave, no LDS, one
// lane polling with s_sleep, bounded like the in-kernel waits of the GEMM kernels (0.5 s, then the status word becomes
// INT_MAX) -- and a stream that has to publish one enqueues the one-thread store.  The end-of-kernel release of whatever ran
// before the store / the acquire at the start of whatever follows the gate order the data as the packets did.
namespace {
__global__ void wait_flag_kernel(const int* __restrict__ ptr, int val, int* __restrict__ info) {
  if (threadIdx.x == 0) {
    const long long t0 = wall_clock64();   // 100 MHz
    while ((int)(__hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - val) < 0) {
      if (wall_clock64() - t0 >= 50000000LL) {
        if (info) atomicMax(info, 0x7fffffff);
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
  }
}
__global__ void set_flag_kernel(int* __restrict__ ptr, int val) {
  __hip_atomic_store(ptr, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // namespace
int gpk_launch_wait_flag(hipStream_t s, const int* ptr, int val, int* info) {
  hipLaunchKernelGGL(wait_flag_kernel, dim3(1), dim3(64), 0, s, ptr, val, info);
  GPK_LAUNCH_CHECK();
  return 0;
}
int gpk_launch_set_flag(hipStream_t s, int* ptr, int val) {
  hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1), 0, s, ptr, val);
  GPK_LAUNCH_CHECK();
  return 0;
}

// ---- can two kernels of this process run at the same time? -----------------------------------------------------------------
// The chain flags of potrf.hip let a kernel wait in-kernel for a word that a kernel (or stream write) on ANOTHER stream sets.
// Under a tool that serialises kernel execution (rocprofv3 --pmc, AMD_SERIALIZE_KERNEL) the producer would never start while the
// consumer spins: a deadlock inside the runtime's own stream-wait kernel, which has no timeout.  So the first factorisation of a
// device asks: a kernel that waits at most 2 ms for a word, and one on a second stream that sets it.
__global__ void probe_wait_kernel(const int* flag, int* result) {
  const long long t0 = wall_clock64();   // 100 MHz
  int seen = 0;
  while (!(seen = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) && wall_clock64() - t0 < 200000LL)
    __builtin_amdgcn_s_sleep(8);
  *result = seen ? 1 : 0;
}
__global__ void probe_set_kernel(int* flag) { __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
int gpk_probe_concurrent_kernels(hipStream_t a, hipStream_t b, int* scratch /* 2 device ints */, int* concurrent) {
  GPK_HIP(hipMemsetAsync(scratch, 0, 2 * sizeof(int), a));
  GPK_HIP(hipStreamSynchronize(a));
  hipLaunchKernelGGL(probe_wait_kernel, dim3(1), dim3(1), 0, a, scratch, scratch + 1);
  GPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(probe_set_kernel, dim3(1), dim3(1), 0, b, scratch);
  GPK_LAUNCH_CHECK();
  GPK_HIP(hipStreamSynchronize(a));
  GPK_HIP(hipStreamSynchronize(b));
  int h[2] = {0, 0};
  GPK_HIP(hipMemcpy(h, scratch, sizeof(h), hipMemcpyDeviceToHost));
  *concurrent = h[1];
  GPK_HIP(hipMemset(scratch, 0, 2 * sizeof(int)));
  return 0;
}

// ---- result mailbox: device scalars -> mapped host memory, sequence word last (gpk.h) --------------------------------
namespace {
__global__ void publish_host_kernel(const double* __restrict__ src, int n, const int* __restrict__ info, double* vals, int* tail,
                                    int seq) {
  if (threadIdx.x == 0) {
    for (int i = 0; i < n; ++i) __hip_atomic_store(vals + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(tail, info ? info[0] : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(tail + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);  // after everything above
  }
}
}  // namespace

extern "C" int gpk_publish_host(void* stream, const double* src, int n, const int* info, void* host_dst, int seq) {
  if (!src || !host_dst || n <= 0 || n > 16) return GPK_E_ARG;
  double* vals = (double*)host_dst;
  hipLaunchKernelGGL(publish_host_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, src, n, info, vals, (int*)(vals + n), seq);
  GPK_LAUNCH_CHECK();
  return 0;
}
