// The two pieces of the Fast R-CNN box-head loss that frcnn_kernels.hip and longtail_kernels.hip share: the smooth-L1 box half of one row
// (one wave per row) and the fixed-order sum of the per-row losses (one workgroup of 256).  Include after common.h.
#pragma once

namespace mi355 {

// roi_heads.py:84-93: smooth-L1 (beta 1) over the 4 deltas of the labelled class of a positive row, zeros elsewhere; -> this row's share of
// sum / N, the same value in every lane.  `y` is only ever compared, never used as an index: any value outside [1, k) gives a zero row.
__device__ __forceinline__ float frcnn_box_row(const float* __restrict__ breg, const float* __restrict__ tgt, float* __restrict__ gbox, int row,
                                               int k, int y, int lane, float inv_n) {
  float lb = 0.0f;
  const float* br = breg + (size_t)row * 4 * k;
  float* gb = gbox ? gbox + (size_t)row * 4 * k : nullptr;
  for (int c = lane; c < 4 * k; c += 64) {
    float g = 0.0f;
    if (y > 0 && (c >> 2) == y) {
      const float d = br[c] - tgt[(size_t)row * 4 + (c & 3)];
      const float a = fabsf(d);
      lb += a < 1.0f ? 0.5f * d * d : a - 0.5f;
      g = (a < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f)) * inv_n;
    }
    if (gb) gb[c] = g;
  }
  return wave_sum(lb) * inv_n;
}

// sums of row_cls[0:n] and row_box[0:n] by one workgroup of 256 threads: strided partial sums, then an LDS tree - the same order on every
// run.  The results are valid in thread 0.
__device__ __forceinline__ void frcnn_sum_rows(const float* __restrict__ row_cls, const float* __restrict__ row_box, int n, float& cls, float& box) {
  __shared__ float s1[256], s2[256];
  float a = 0.0f, b = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) {
    a += row_cls[i];
    b += row_box[i];
  }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      s1[threadIdx.x] += s1[threadIdx.x + o];
      s2[threadIdx.x] += s2[threadIdx.x + o];
    }
    __syncthreads();
  }
  cls = s1[0];
  box = s2[0];
}

}  // namespace mi355
