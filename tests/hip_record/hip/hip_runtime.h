// Recording stand-in for <hip/hip_runtime.h>: exactly the HIP types and calls that gpflow_amd/csrc/potrf.hip, drivers.hip and their
// headers use, declared only.  tests/potrf_schedule_run.cpp defines them as recorders and compiles the two files as plain C++ with
// this directory first on the include path (tests/test_potrf_schedule.py).  A HIP name that those files start to use and that is
// missing here is a compile error of that test: add it here and record it in the runner.
#pragma once
#include <stddef.h>
#include <stdint.h>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
struct RecStream;
struct RecEvent;
typedef RecStream* hipStream_t;
typedef RecEvent* hipEvent_t;
struct hipDeviceProp_t { int multiProcessorCount; };
constexpr unsigned hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipEventDisableSystemFence = 0x20000000;
constexpr unsigned hipStreamWaitValueGte = 0;

hipError_t hipGetLastError();
hipError_t hipGetDevice(int* dev);
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int dev);
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest);
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags);
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority);
hipError_t hipExtStreamCreateWithCUMask(hipStream_t* s, uint32_t words, const uint32_t* mask);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipEventCreate(hipEvent_t* e);
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s);
hipError_t hipEventSynchronize(hipEvent_t e);
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b);
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags);
hipError_t hipStreamWaitValue32(hipStream_t s, void* ptr, uint32_t value, unsigned flags, uint32_t mask);
hipError_t hipStreamWriteValue32(hipStream_t s, void* ptr, uint32_t value, unsigned flags);
hipError_t hipMalloc(void** ptr, size_t bytes);
hipError_t hipMemset(void* ptr, int value, size_t bytes);
hipError_t hipMemsetAsync(void* ptr, int value, size_t bytes, hipStream_t s);
