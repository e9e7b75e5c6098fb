// BatchNorm + LeakyReLU backward, per element: the scalar forms behind bn_dy8 / bn_dz8 (elem_kernels.hip) and the EPI_BNRED epilogue of
// the data-gradient kernels (igemm_common.h), which sums dy and dy * xhat over the tile it writes.
#pragma once
#include <hip/hip_runtime.h>

// dy = g * lrelu'(y),  y = z * scale + shift
__device__ __forceinline__ float bn_dy(float g, float z, float scale, float shift, float slope) {
  const float y = z * scale + shift;
  return y > 0.f ? g : g * slope;
}
__device__ __forceinline__ float bn_xhat(float z, float mu, float is) { return (z - mu) * is; }
