// Per-item counts -> exclusive offsets: the one block-wide scan of the run-length family (rle_kernels.hip, rle_string_kernels.hip,
// poly_kernels.hip).  off[i] = load(0) + .. + load(i - 1) for i in [0, n), off[n] = the total; with a Flag, num_flagged[0] = the number of
// i with flag(i).
//
// One block of THREADS; a thread owns SCAN_ITEMS consecutive items of each round of THREADS * SCAN_ITEMS: it sums them, the wavefront scans
// the sums, the waves' totals go through LDS, and the round's total is carried into the next.  Two barriers per round.  The block has
// SCAN_THREADS threads, or SCAN_THREADS_SMALL where those take all n items in one round (a few hundred masks of one image: 16 waves
// measured 1 us slower there than the 4 of the kernels this one replaced; profiles/r27_rle_protocol.md).
// `load` may read `off` itself (in place): a thread reads all its items of a round before it writes any of them, and no other thread
// touches them.  Integers only, fixed order: the same bits every run.
#pragma once
#include "wave_ops.h"

#include <type_traits>

namespace mi355 {

constexpr int SCAN_THREADS = 1024, SCAN_THREADS_SMALL = 256, SCAN_ITEMS = 8;

struct ScanInPlace {                                     // the counts are in `off` already
  const long long* off;
  __device__ __forceinline__ long long operator()(long long i) const { return off[i]; }
};
struct ScanNoFlag {
  __device__ __forceinline__ bool operator()(long long) const { return false; }
};

template <int THREADS, class Load, class Flag>
__global__ __launch_bounds__(THREADS) void offsets_scan_kernel(long long n, Load load, long long* off, Flag flag, long long* num_flagged) {
  constexpr int NW = THREADS / WAVE;
  constexpr bool FLAGS = !std::is_same<Flag, ScanNoFlag>::value;
  __shared__ long long s_wave[NW];
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t >> 6;
  long long carry = 0, flagged = 0;
  for (long long r0 = 0; r0 < n; r0 += (long long)THREADS * SCAN_ITEMS) {
    const long long i0 = r0 + (long long)t * SCAN_ITEMS;
    long long v[SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      v[j] = i0 + j < n ? load(i0 + j) : 0;
      if (FLAGS && i0 + j < n && flag(i0 + j)) ++flagged;
      mine += v[j];
    }
    const long long incl = wave_scan_incl(mine, lane);
    if (lane == WAVE - 1) s_wave[wv] = incl;
    __syncthreads();
    long long before = carry, all = 0;
    for (int j = 0; j < NW; ++j) {
      if (j < wv) before += s_wave[j];
      all += s_wave[j];
    }
    long long at = before + incl - mine;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      if (i0 + j < n) off[i0 + j] = at;
      at += v[j];
    }
    carry += all;
    __syncthreads();
  }
  if (FLAGS) {
    flagged = wave_sum_i64(flagged);
    if (lane == 0) s_wave[wv] = flagged;                  // free again: the last round ended with a barrier
    __syncthreads();
    if (t == 0) {
      long long b = 0;
      for (int j = 0; j < NW; ++j) b += s_wave[j];
      num_flagged[0] = b;
    }
  }
  if (t == 0) off[n] = carry;
}

template <class Load, class Flag = ScanNoFlag>
inline void launch_offsets_scan(long long n, Load load, long long* off, void* stream, Flag flag = Flag(), long long* num_flagged = nullptr) {
  if (n <= (long long)SCAN_THREADS_SMALL * SCAN_ITEMS)
    hipLaunchKernelGGL((offsets_scan_kernel<SCAN_THREADS_SMALL, Load, Flag>), dim3(1), dim3(SCAN_THREADS_SMALL), 0, S(stream), n, load, off, flag,
                       num_flagged);
  else
    hipLaunchKernelGGL((offsets_scan_kernel<SCAN_THREADS, Load, Flag>), dim3(1), dim3(SCAN_THREADS), 0, S(stream), n, load, off, flag, num_flagged);
}

}  // namespace mi355
