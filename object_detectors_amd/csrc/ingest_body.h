// The uint8 ingest, stated once: bilinear taps, the four-tap blend and the tile loop of mi355det_ingest_u8 (transform_kernels.hip) and
// mi355det_ingest_aug_u8 (augment_kernels.hip).  The two differ only in how a tap is fetched, which a Rule says:
//   Rule::Image                 the table entry (offset, out_h, out_w, first_tile and whatever the rule needs)
//   Rule(packed, im)            built once per thread and tile
//   h(), w()                    the size of the image the resize sees
//   row(i), col(i)              a handle for row / column i of that image, i in [0, h) / [0, w)
//   byte(row, col, c)           channel c of the pixel there
#pragma once
#include "common.h"

namespace mi355 {

// One axis of ATen's upsample_bilinear2d (area_pixel_compute_source_index, align_corners = false):
//   src = max(scale * (dst + 0.5) - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1
struct Taps {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Taps bilinear_taps(float scale, int dst, int in) {
  const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
  Taps t;
  t.i0 = (int)s;
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = s - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}
// The four-tap blend, for the float route (resize_bilinear_kernel) and the uint8 routes alike:
//   val = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)
__device__ __forceinline__ float bilinear_blend(float v00, float v01, float v10, float v11, const Taps& ty, const Taps& tx) {
  return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

constexpr int TILE_H = MI355DET_INGEST_TILE_H, TILE_W = MI355DET_INGEST_TILE_W;
static_assert(TILE_H * (TILE_W / 4) == 256, "one thread per four pixels of a tile");

// A batch of uint8 HWC images of any sizes, packed back to back, in one launch (tables: include/mi355det.h).  A block walks tiles of
// TILE_H x TILE_W output pixels; a thread owns four neighbouring pixels of one row for all three channels, so each of its sixteen taps is
// three neighbouring bytes and each plane's store is 16 bytes per lane (VEC: pw % 4 == 0 and out 16-byte aligned; else dwords).
// The normalised value of a byte, ((float)b / 255.0f - mean) / std, has 256 values per channel: a block computes them once into LDS with
// the two correctly rounded divisions of the float route and looks the taps up, instead of 24 divisions per pixel.  The bytes are plain
// byte-indexed loads without an alignment assumption (rows are 3w bytes); the taps of neighbouring pixels share cache lines.
template <bool VEC, class Rule>
__device__ __forceinline__ void ingest_tiles(const uint8_t* __restrict__ packed, const typename Rule::Image* __restrict__ table, int n, int tiles_x,
                                             int total_tiles, const float* __restrict__ mean, const float* __restrict__ stdv,
                                             float* __restrict__ out, int ph, int pw) {
  __shared__ float lut[3][256];
  for (int e = threadIdx.x; e < 3 * 256; e += 256) lut[e >> 8][e & 255] = ((float)(e & 255) / 255.0f - mean[e >> 8]) / stdv[e >> 8];
  __syncthreads();
  const int lx = (threadIdx.x % (TILE_W / 4)) * 4, ly = threadIdx.x / (TILE_W / 4);
  const long long plane = (long long)ph * pw;
  for (int tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    int lo = 0, hi = n - 1;                                  // block-uniform: the last image whose first tile is <= tile
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (table[mid].first_tile <= tile) lo = mid; else hi = mid - 1;
    }
    const typename Rule::Image im = table[lo];
    const int t = tile - im.first_tile;
    const int y = (t / tiles_x) * TILE_H + ly, x = (t % tiles_x) * TILE_W + lx;
    if (y >= ph || x >= pw) continue;
    float v[3][4] = {};
    if (y < im.out_h && x < im.out_w) {
      const Rule rule(packed, im);
      const float rh = (float)rule.h() / (float)im.out_h, rw = (float)rule.w() / (float)im.out_w;
      const Taps ty = bilinear_taps(rh, y, rule.h());
      const auto r0 = rule.row(ty.i0), r1 = rule.row(ty.i1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x + j >= im.out_w) continue;
        const Taps tx = bilinear_taps(rw, x + j, rule.w());
        const auto c0 = rule.col(tx.i0), c1 = rule.col(tx.i1);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          v[c][j] = bilinear_blend(lut[c][rule.byte(r0, c0, c)], lut[c][rule.byte(r0, c1, c)], lut[c][rule.byte(r1, c0, c)],
                                   lut[c][rule.byte(r1, c1, c)], ty, tx);
      }
    }
    float* o = out + ((long long)lo * 3 * ph + y) * pw + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (VEC) {
        *(float4*)(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < pw) o[c * plane + j] = v[c][j];
      }
    }
  }
}

}  // namespace mi355
