// Integer wavefront primitives of the run-length, evaluation and comparison kernels: 64-bit shuffles, order-free reductions (exact on
// integers) and the inclusive scan over the lanes.  All are unrolled butterflies of 32-bit shuffles; the float reductions are in common.h.
// yolo_kernels.hip, box_kernels.hip and roi_kernels.hip keep their own: theirs sit inside tuned loops (DPP forms, lane-63 results).
#pragma once
#include "common.h"

namespace mi355 {

__device__ __forceinline__ long long shfl_i64(long long v, int src) {
  const int lo = __shfl((int)v, src, WAVE), hi = __shfl((int)(v >> 32), src, WAVE);
  return ((long long)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ long long shfl_up_i64(long long v, int delta) {
  const int lo = __shfl_up((int)v, delta, WAVE), hi = __shfl_up((int)(v >> 32), delta, WAVE);
  return ((long long)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ long long shfl_xor_i64(long long v, int mask) {
  const int lo = __shfl_xor((int)v, mask, WAVE), hi = __shfl_xor((int)(v >> 32), mask, WAVE);
  return ((long long)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor_i64(v, o);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, WAVE));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, WAVE));
  return v;
}
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (unsigned)__shfl_xor((int)v, o, WAVE);
  return v;
}

// lane l gets v(0) + .. + v(l); T = int or long long (HIP shuffles a 64-bit value as its two halves, like shfl_up_i64)
template <class T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const T t = __shfl_up(v, o, WAVE);
    if (lane >= o) v += t;
  }
  return v;
}

}  // namespace mi355
