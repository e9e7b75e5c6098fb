// Bitonic network on 64-bit keys in LDS, largest first, by the THREADS threads of one workgroup (top-k tails of roi_kernels.hip, the
// small-input branch of nms_sort_kernel in box_kernels.hip).  npad is a power of two; the caller synchronises after filling keys[0, npad),
// and the sort ends with a barrier.
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

template <int THREADS>
__device__ __forceinline__ void bitonic_sort_desc(unsigned long long* keys, int npad) {
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < npad; i += THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keys[i], c = keys[ixj];
          if (((i & k) == 0) ? a < c : a > c) {
            keys[i] = c;
            keys[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
}

}  // namespace mi355
