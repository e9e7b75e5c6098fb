// paste_masks_in_image (tvision/roi_heads.py:403-537) for ONE output pixel: expand_masks (zero padding, scale (M + 2 pad) / M), expand_boxes,
// the .to(int64) truncation, torch's bilinear upsample (align_corners = False) of the padded mask to the box and the clipped paste.
// Shared by paste_masks_kernel (mask_kernels.hip), which writes the value, and by the run-length kernels (rle_kernels.hip), which only
// compare it with a threshold.  Both files are compiled with -ffp-contract=off, so the two see the same float32 bits.
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

// expand_masks: float(M + 2*pad) / M, applied to float32 boxes
__host__ __device__ __forceinline__ float paste_scale(int M, int pad) { return (float)((double)(M + 2 * pad) / (double)M); }

// linear weights of torch's upsample (align_corners = False, no scale given): src = max(scale*(dst+0.5)-0.5, 0), index floor clamped to
// in-1, lambda clamped to [0,1], the second tap one further unless at the border
__device__ __forceinline__ void lin_tap(int dst, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = min((int)floorf(src), in - 1);
  float lam = src - (float)i0;
  lam = fminf(fmaxf(lam, 0.f), 1.f);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = lam;
  l0 = 1.f - lam;
}

// the integer box of one detection: [b0, b0 + bw) x [b1, b1 + bh) is where the resized mask lands, [x0, x1) x [y0, y1) its part inside the
// H x W image (empty when x1 <= x0 or y1 <= y0)
struct PasteBox {
  long long b0, b1, bw, bh, x0, x1, y0, y1;
  __device__ __forceinline__ bool has(int x, int y) const { return x >= x0 && x < x1 && y >= y0 && y < y1; }
};

// expand_boxes, then .to(int64) (truncation)
__device__ __forceinline__ PasteBox paste_box(const float* __restrict__ bx, float scale, int H, int W) {
  float w_half = (bx[2] - bx[0]) * 0.5f, h_half = (bx[3] - bx[1]) * 0.5f;
  const float x_c = (bx[2] + bx[0]) * 0.5f, y_c = (bx[3] + bx[1]) * 0.5f;
  w_half *= scale;
  h_half *= scale;
  PasteBox B;
  B.b0 = (long long)(x_c - w_half);
  const long long b2 = (long long)(x_c + w_half);
  B.b1 = (long long)(y_c - h_half);
  const long long b3 = (long long)(y_c + h_half);
  B.bw = max(b2 - B.b0 + 1, 1ll);
  B.bh = max(b3 - B.b1 + 1, 1ll);
  B.x0 = max(B.b0, 0ll);
  B.x1 = min(b2 + 1, (long long)W);
  B.y0 = max(B.b1, 0ll);
  B.y1 = min(b3 + 1, (long long)H);
  return B;
}

// the value paste_masks_in_image leaves at pixel (x, y) of the detection whose M x M probabilities are m and whose box is B: 0 outside B
__device__ __forceinline__ float paste_value(const float* __restrict__ m, int M, int pad, const PasteBox& B, int x, int y) {
  if (!B.has(x, y)) return 0.f;
  const int Mp = M + 2 * pad;
  const int iy = (int)(y - B.b1), ix = (int)(x - B.b0);
  int ya, yb, xa, xb;
  float wy0, wy1, wx0, wx1;
  lin_tap(iy, Mp, (float)Mp / (float)B.bh, ya, yb, wy0, wy1);
  lin_tap(ix, Mp, (float)Mp / (float)B.bw, xa, xb, wx0, wx1);
  auto at = [&](int yy, int xx) -> float {          // the zero-padded (M + 2 pad)^2 mask of expand_masks
    yy -= pad;
    xx -= pad;
    return (yy >= 0 && yy < M && xx >= 0 && xx < M) ? m[yy * M + xx] : 0.f;
  };
  const float t0 = at(ya, xa) * wx0 + at(ya, xb) * wx1;
  const float t1 = at(yb, xa) * wx0 + at(yb, xb) * wx1;
  return t0 * wy0 + t1 * wy1;
}

}  // namespace mi355
