// The RoIAlign rules of torchvision.ops.roi_align / MultiScaleRoIAlign, stated once for every kernel that pools (roi_kernels.hip: the NCHW,
// the per-sample channels-last and the separable form; mask_kernels.hip: the mask targets): the level mapper, the level table, the
// RoI-to-bins geometry, the sample positions and the border rule with its bilinear weights.  Device helpers only; the files that include
// this are compiled with -ffp-contract=off, and every helper keeps torchvision's float32 operation order.
#pragma once
#include "common.h"

namespace mi355 {

// LevelMapper of MultiScaleRoIAlign: k = floor(4 + log2(sqrt(area)/224) + 1e-6) clamped to the pyramid
__device__ __forceinline__ int map_level(const float4 r, int k_min, int k_max) {
  const float s = sqrtf((r.z - r.x) * (r.w - r.y));
  int k = (int)floorf(4.0f + log2f(s / 224.0f) + 1e-6f);
  k = min(max(k, k_min), k_max);
  return k - k_min;
}

// Up to four pyramid levels: T = float (NCHW planes, ld unused) or bf16_t (NHWC with pixel pitch ld); grad = the fp32 feature gradients.
template <class T>
struct RoiLevels {
  const T* feat[4];
  float* grad[4];
  int h[4], w[4], ld[4];
  float scale[4];
  struct Level {
    const T* feat;
    float* grad;
    int h, w, ld;
    float scale;
  };
  // (all four entries are read before the selects, from scalar registers: a level loop, unrolled only late, left the table in scratch, and
  // reads under the conditions became one read per lane at an address chosen by lv)
  template <class V>
  static __device__ __forceinline__ V sel(int lv, const V (&a)[4]) {
    const V a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    return lv == 3 ? a3 : (lv == 2 ? a2 : (lv == 1 ? a1 : a0));
  }
  __device__ __forceinline__ Level pick(int lv) const { return Level{sel(lv, feat), sel(lv, grad), sel(lv, h), sel(lv, w), sel(lv, ld), sel(lv, scale)}; }
};

// RoI -> bins: box * scale - offset (0.5 when aligned; else the sides are clamped to >= 1), bin size, sampling grid (`sampling` or
// ceil(side / bins)) and the divisor max(gh * gw, 1).  The mask targets call it with scale 1, not aligned: box * 1.0f - 0.0f is the box
// itself for every finite coordinate (and for +-0 and infinities), so nothing is rounded there.
struct RoiBins {
  float x1, y1, bh, bw, cnt;
  int gh, gw;
};
__device__ __forceinline__ RoiBins roi_bins(const float4 box, float scale, bool aligned, int ph, int pw, int sampling) {
  const float off = aligned ? 0.5f : 0.0f;
  const float x1 = box.x * scale - off, y1 = box.y * scale - off, x2 = box.z * scale - off, y2 = box.w * scale - off;
  float rw = x2 - x1, rh = y2 - y1;
  if (!aligned) {
    rw = fmaxf(rw, 1.0f);
    rh = fmaxf(rh, 1.0f);
  }
  RoiBins b;
  b.x1 = x1;
  b.y1 = y1;
  b.bh = rh / (float)ph;
  b.bw = rw / (float)pw;
  b.gh = sampling > 0 ? sampling : (int)ceilf(rh / (float)ph);
  b.gw = sampling > 0 ? sampling : (int)ceilf(rw / (float)pw);
  b.cnt = fmaxf((float)(b.gh * b.gw), 1.0f);
  return b;
}

// coordinate of sample i (of `grid`) of bin `bin` along one axis
__device__ __forceinline__ float bin_sample(float start, int bin, float bin_size, int i, int grid) {
  return start + bin * bin_size + ((float)i + 0.5f) * bin_size / (float)grid;
}

// The border rule along one axis: a sample outside [-1, size] is dropped (ok = false), one below 0 is moved to 0, one in the last pixel or
// beyond collapses onto it (hi = lo = size - 1, weight 1 | 0); wl weights pixel lo, wh pixel hi.
__device__ __forceinline__ void axis_sample(float s, int size, bool& ok, int& lo, int& hi, float& wl, float& wh) {
  ok = !(s < -1.0f || s > (float)size);
  if (s <= 0.f) s = 0.f;
  lo = (int)s;
  if (lo >= size - 1) {
    hi = lo = size - 1;
    s = (float)lo;
  } else hi = lo + 1;
  wh = s - lo;
  wl = 1.f - wh;
}

// The four corners of a 2-D sample; false when it is dropped.  The weights stay FACTORS: a forward multiplies (hy * hx) * f, a backward
// (g * hy) * hx, and both orders are part of the results.
struct RoiCorners {
  int yl, yh, xl, xh;
  float hy, ly, hx, lx;
};
__device__ __forceinline__ bool roi_corners(float y, float x, int H, int W, RoiCorners& q) {
  bool oky, okx;
  axis_sample(y, H, oky, q.yl, q.yh, q.hy, q.ly);
  axis_sample(x, W, okx, q.xl, q.xh, q.hx, q.lx);
  return oky && okx;
}

}  // namespace mi355
