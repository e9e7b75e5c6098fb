// YOLO ingest: the input side of the YOLO step (yolo/dsets/transformations.py:10-53, ResizeToTensor) for a whole batch of decoded uint8
// images: cv2.resize(img, (S, S), INTER_CUBIC), / 255, normalise -> fp32 [n, 3, S, S] in one launch; the boxes to relative xcycwh and the
// relative areas in one more.  The rule (OpenCV's 8-bit fixed-point bicubic, restated) is written out in include/mi355det.h.
//
// The image kernel does integer arithmetic only.  The per-axis (s, w0..w3) come from the host, built there in the rule's float32 order, and
// the 768 normalised values of a byte come from the host too, so no float operation on the device has to round as numpy or torch do.
// Like ingest_u8_kernel (transform_kernels.hip) a block walks tiles of TILE_H x TILE_W output pixels and a thread owns four neighbouring
// pixels of one row for all three channels: each plane's store is 16 bytes per lane (VEC: S % 4 == 0 and out 16-byte aligned; else dwords),
// and the look-up table sits in LDS.  The 48 byte taps of a pixel come from the tile's source footprint staged in LDS where it fits (below);
// read tap by tap from global memory a wave's byte load touches four source rows and costs a cache-line access for each, which left the
// kernel at 22% of a device copy's store rate.
#include "common.h"

using namespace mi355;

namespace {

constexpr int TILE_H = MI355DET_YOLO_TILE_H, TILE_W = MI355DET_YOLO_TILE_W;
static_assert(TILE_H * (TILE_W / 4) == 256, "one thread per four pixels of a tile");
static_assert(sizeof(mi355det_cubic_tap) == 12 && sizeof(mi355det_yolo_image) == 32, "layouts of include/mi355det.h");

// Source indices s-1 .. s+2 clamped to [0, size-1].  s is clamped first so that no table content can overflow the sum.
__device__ __forceinline__ void tap_indices(int s, int size, int idx[4]) {
  s = min(max(s, -4), size + 4);
#pragma unroll
  for (int k = 0; k < 4; ++k) idx[k] = min(max(s - 1 + k, 0), size - 1);
}

// One pixel, three channels: r[ky] points at byte 0 of source row ky (global memory, or its staged copy), cols[kx] are byte offsets in it.
template <typename Row>
__device__ __forceinline__ void cubic_pixel(const Row (&r)[4], const int (&cols)[4], int pix, const mi355det_cubic_tap& tx, const mi355det_cubic_tap& ty,
                                            const float* lut, float (&v)[3][4], int j) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int co = pix == 3 ? c : 0;
    int acc = 0;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      int hsum = 0;
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) hsum += (int)tx.w[kx] * (int)r[ky][cols[kx] + co];
      acc += (int)ty.w[ky] * hsum;
    }
    const int byte = min(max((acc + (1 << 21)) >> 22, 0), 255);      // >> of a negative int is arithmetic here
    v[c][j] = lut[c * 256 + byte];
  }
}

// A tile's source footprint (rows r_lo .. r_hi, source columns c_lo .. c_hi) is staged in LDS when it fits STAGE_BYTES: the block copies it
// with coalesced byte loads, once, and the 48 taps of every pixel are LDS reads.  A footprint that does not fit (a strong reduction: 16 x 64
// output pixels of a 4:1 reduction span 67 x 259 source pixels) is read tap by tap from global memory, as ingest_u8_kernel does.
constexpr int STAGE_BYTES = 24 * 1024;

template <bool VEC>
__global__ __launch_bounds__(256) void yolo_ingest_u8_kernel(const uint8_t* __restrict__ packed, const mi355det_yolo_image* __restrict__ table,
                                                             const mi355det_cubic_tap* __restrict__ taps, const float* __restrict__ lut_g,
                                                             float* __restrict__ out, int size, int tiles_x, int tiles_per_image, int total_tiles) {
  __shared__ float lut[3 * 256];
  __shared__ uint8_t stage[STAGE_BYTES];
  for (int e = threadIdx.x; e < 3 * 256; e += 256) lut[e] = lut_g[e];
  __syncthreads();
  const int lx = (threadIdx.x % (TILE_W / 4)) * 4, ly = threadIdx.x / (TILE_W / 4);
  const long long plane = (long long)size * size;
  for (int tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    const int img = tile / tiles_per_image, t = tile - img * tiles_per_image;       // every image has the same S x S tiles
    const int y0 = (t / tiles_x) * TILE_H, x0 = (t % tiles_x) * TILE_W;
    const int y = y0 + ly, x = x0 + lx;
    const bool active = y < size && x < size;
    const mi355det_yolo_image im = table[img];
    const int pix = im.channels == 3 ? 3 : 1;                  // bytes per source pixel; a grey image serves its one byte to all channels
    const uint8_t* base = packed + im.offset;

    // block-uniform: the footprint of the tile from the taps of its first and last row and column (s does not decrease along an axis)
    int fr[4], lr[4], fc[4], lc[4];
    tap_indices(taps[(long long)im.ytab + y0].s, im.h, fr);
    tap_indices(taps[(long long)im.ytab + min(y0 + TILE_H, size) - 1].s, im.h, lr);
    tap_indices(taps[(long long)im.xtab + x0].s, im.w, fc);
    tap_indices(taps[(long long)im.xtab + min(x0 + TILE_W, size) - 1].s, im.w, lc);
    const int r_lo = min(fr[0], lr[0]), r_hi = max(fr[3], lr[3]);
    const int a_lo = min(fc[0], lc[0]), a_hi = max(fc[3], lc[3]);
    const int c_lo = im.flip ? im.w - 1 - a_hi : a_lo, c_hi = im.flip ? im.w - 1 - a_lo : a_hi;      // in source columns
    const int nrows = r_hi - r_lo + 1, seg = (c_hi - c_lo + 1) * pix, pitch = (seg + 3) & ~3;
    const bool staged = (long long)nrows * pitch <= STAGE_BYTES;
    if (staged) {
      __syncthreads();                                           // the previous tile's readers are done
      const uint8_t* first = base + ((long long)r_lo * im.w + c_lo) * pix;
      for (int i = threadIdx.x; i < nrows * seg; i += 256) {
        const int rr = i / seg, b = i - rr * seg;
        stage[rr * pitch + b] = first[(long long)rr * im.w * pix + b];
      }
      __syncthreads();
    }
    if (!active) continue;                                       // `staged` is block-uniform: no barrier is skipped by a part of the block

    const mi355det_cubic_tap ty = taps[(long long)im.ytab + y];
    int rows[4];
    tap_indices(ty.s, im.h, rows);
    float v[3][4] = {};
    if (staged) {
      const uint8_t* r[4];                                       // staged rows; indices clamped into the footprint, a no-op for a monotonic table
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = stage + (min(max(rows[k], r_lo), r_hi) - r_lo) * pitch;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!VEC && x + j >= size) continue;
        const mi355det_cubic_tap tx = taps[(long long)im.xtab + x + j];
        int cols[4];
        tap_indices(tx.s, im.w, cols);
#pragma unroll
        for (int k = 0; k < 4; ++k) cols[k] = (min(max(im.flip ? im.w - 1 - cols[k] : cols[k], c_lo), c_hi) - c_lo) * pix;
        cubic_pixel(r, cols, pix, tx, ty, lut, v, j);
      }
    } else {
      const uint8_t* r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = base + (long long)rows[k] * im.w * pix;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!VEC && x + j >= size) continue;
        const mi355det_cubic_tap tx = taps[(long long)im.xtab + x + j];
        int cols[4];
        tap_indices(tx.s, im.w, cols);
#pragma unroll
        for (int k = 0; k < 4; ++k) cols[k] = (im.flip ? im.w - 1 - cols[k] : cols[k]) * pix;
        cubic_pixel(r, cols, pix, tx, ty, lut, v, j);
      }
    }
    float* o = out + ((long long)img * 3 * size + y) * size + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (VEC) {
        *(float4*)(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < size) o[c * plane + j] = v[c][j];
      }
    }
  }
}

// One thread per box of the whole batch, float64 throughout (transformations.py:44-49, helper.convert2_rel_xcycwh); the file is compiled
// with -ffp-contract=off, so every quotient and sum is rounded once, as torch's CPU operations round them.
__global__ __launch_bounds__(256) void yolo_targets_kernel(const double* __restrict__ boxes, const double* __restrict__ area, long long g,
                                                           const long long* __restrict__ box_offsets,
                                                           const mi355det_yolo_image* __restrict__ table, int n, float* __restrict__ bbox,
                                                           double* __restrict__ rel_area) {
  const long long b = blockIdx.x * 256ll + threadIdx.x;
  if (b >= g) return;
  int lo = 0, hi = n - 1;                                    // the last image whose first row is <= b (an image without boxes owns no row)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (box_offsets[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const mi355det_yolo_image im = table[lo];
  const double w = (double)im.w, h = (double)im.h;
  double xmin = boxes[4 * b];
  const double ymin = boxes[4 * b + 1], bw = boxes[4 * b + 2], bh = boxes[4 * b + 3];
  if (im.flip) xmin = w - (xmin + bw);
  const double rx = xmin / w, ry = ymin / h, rw = bw / w, rh = bh / h;
  bbox[4 * b] = (float)(rx + rw / 2.0);
  bbox[4 * b + 1] = (float)(ry + rh / 2.0);
  bbox[4 * b + 2] = (float)rw;
  bbox[4 * b + 3] = (float)rh;
  rel_area[b] = area[b] / (double)((long long)im.h * im.w);
}

}  // namespace

extern "C" {

int mi355det_yolo_ingest_u8(const uint8_t* packed, int64_t packed_bytes, const mi355det_yolo_image* table, const mi355det_yolo_image* table_dev,
                            int32_t n, const mi355det_cubic_tap* taps_dev, int64_t n_taps, const float* lut, float* out, int32_t size,
                            void* stream) {
  if (n <= 0) return fail(MI355DET_EINVAL, "%s: need n > 0", "yolo_ingest_u8");
  if (!packed || !table || !table_dev || !taps_dev || !lut || !out) return fail(MI355DET_EINVAL, "%s: null pointer", "yolo_ingest_u8");
  if (size <= 0) return fail(MI355DET_EINVAL, "%s: need size > 0", "yolo_ingest_u8");
  const long long tiles_x = (size + TILE_W - 1) / TILE_W, tiles = tiles_x * ((size + TILE_H - 1) / TILE_H);
  if (tiles * n > INT32_MAX) return fail(MI355DET_EINVAL, "%s: too many tiles for one launch", "yolo_ingest_u8");
  for (int i = 0; i < n; ++i) {
    const mi355det_yolo_image& im = table[i];
    if (im.h <= 0 || im.w <= 0) return fail(MI355DET_EINVAL, "%s: image %lld: sizes must be > 0", "yolo_ingest_u8", i);
    if (im.channels != 1 && im.channels != 3) return fail(MI355DET_EINVAL, "%s: image %lld: channels must be 1 or 3", "yolo_ingest_u8", i);
    if (im.offset < 0 || im.offset > packed_bytes || (long long)im.h * im.w * im.channels > packed_bytes - im.offset)
      return fail(MI355DET_EINVAL, "%s: image %lld lies outside the %lld packed bytes", "yolo_ingest_u8", i, packed_bytes);
    if (im.xtab < 0 || im.ytab < 0 || (long long)im.xtab + size > n_taps || (long long)im.ytab + size > n_taps)
      return fail(MI355DET_EINVAL, "%s: image %lld: a tap table lies outside the %lld entries", "yolo_ingest_u8", i, n_taps);
  }
  const int total = (int)(tiles * n), grid = min(total, 2048);
  if (size % 4 == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(yolo_ingest_u8_kernel<true>, dim3(grid), dim3(256), 0, S(stream), packed, table_dev, taps_dev, lut, out, size, (int)tiles_x,
                       (int)tiles, total);
  else
    hipLaunchKernelGGL(yolo_ingest_u8_kernel<false>, dim3(grid), dim3(256), 0, S(stream), packed, table_dev, taps_dev, lut, out, size, (int)tiles_x,
                       (int)tiles, total);
  return check_launch("yolo_ingest_u8");
}

int mi355det_yolo_targets(const double* boxes, const double* area, int64_t g, const int64_t* box_offsets, const mi355det_yolo_image* table_dev,
                          int32_t n, float* bbox, double* rel_area, void* stream) {
  if (n <= 0 || g < 0) return fail(MI355DET_EINVAL, "%s: need n > 0 and g >= 0", "yolo_targets");
  if (!box_offsets || !table_dev) return fail(MI355DET_EINVAL, "%s: null table", "yolo_targets");
  if (g == 0) return MI355DET_OK;
  if (!boxes || !area || !bbox || !rel_area) return fail(MI355DET_EINVAL, "%s: null boxes", "yolo_targets");
  hipLaunchKernelGGL(yolo_targets_kernel, dim3((int)((g + 255) / 256)), dim3(256), 0, S(stream), boxes, area, (long long)g,
                     (const long long*)box_offsets, table_dev, n, bbox, rel_area);
  return check_launch("yolo_targets");
}

}  // extern "C"
