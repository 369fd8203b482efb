// wave_util.h — the wave-level device helpers the kernel files share (gfx950, wave64).  Device-only: include it from .hip
// files, after kernels.h.  One definition of each; a kernel file adds none of its own under another name.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace gsx {

typedef double v4d __attribute__((ext_vector_type(4)));   // an accumulator of v_mfma_f64_16x16x4

// sum over the wave, total in lane 0 (fixed order => deterministic)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__device__ __forceinline__ i64 readlane_i64(i64 v, int src_lane) {  // src_lane must be wave-uniform
  int lo = (int)(v & 0xFFFFFFFFll), hi = (int)(v >> 32);
  lo = __builtin_amdgcn_readlane(lo, src_lane);
  hi = __builtin_amdgcn_readlane(hi, src_lane);
  return ((i64)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ double readlane_f64(double v, int src_lane) {  // src_lane wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}
// lane's value of v for every lane (lane may differ from lane to lane, unlike readlane_i64's)
__device__ __forceinline__ i64 shfl_i64(i64 v, int lane) {
  return ((i64)__shfl((int)(v >> 32), lane) << 32) | (unsigned)__shfl((int)(v & 0xffffffff), lane);
}
__device__ __forceinline__ double shfl_f64(double v, int lane) {
  return __longlong_as_double(shfl_i64(__double_as_longlong(v), lane));
}

// 1 / sqrt(d) to full precision from the hardware seed (one cubic correction step)
__device__ __forceinline__ double rsqrt_refined(double d) {
  const double y0 = __builtin_amdgcn_rsq(d);
  const double e = fma(-d * y0, y0, 1.0);
  return fma(y0 * e, fma(e, 0.375, 0.5), y0);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding GLOBAL access
// (s_waitcnt vmcnt(0)) — which would put the latency of in-flight prefetches and of
// just-issued stores on the critical path of the latency-bound kernels that use it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The same for code in which ONE wave owns its LDS: the traffic of its lanes is ordered once the counter has drained
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// e = q d + r for a SMALL quotient (q < 1024, e < 2^23): an integer division by a run-time divisor costs ~40
// instructions on gfx950, and these index splits sit in the inner loops of issue-bound kernels.  rd = 1.0f / d.
__device__ __forceinline__ void divmod_small(int e, int d, float rd, int& q, int& r) {
  q = (int)(((float)e + 0.5f) * rd);
  r = e - q * d;
}

// a front that could not be factored: counted, and the lowest one named
__device__ inline void report_failure(DevStatus* status, int front) {
  atomicAdd(&status->n_fail, 1);
  atomicMin(&status->first_front, front);
}

}  // namespace gsx
