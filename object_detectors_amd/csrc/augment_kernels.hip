// The SSD augmentations of the uint8 ingest (detection/transforms.py:54-239 on PIL images, decided on the host by tvision/transforms.py):
//   mi355det_photometric_u8   RandomPhotometricDistort on the packed bytes, in place: Pillow's 8-bit rules, restated in include/mi355det.h
//   mi355det_ingest_aug_u8    RandomZoomOut, RandomIoUCrop and RandomHorizontalFlip folded into the ingest: the tile loop of ingest_body.h
//                             with a fetch rule that maps a tap of the window to a source pixel or to the fill colour, so the canvas of
//                             the zoom-out is never written anywhere
// Everything that decides a byte is integer or correctly rounded IEEE arithmetic in the order Pillow's C has it (-ffp-contract=off).
#include "common.h"
#include "ingest_body.h"

using namespace mi355;

namespace {

constexpr int MAX_OPS = MI355DET_PHOTO_MAX_OPS, BLOCK_PIXELS = MI355DET_PHOTO_BLOCK_PIXELS;

// Image.blend(degenerate, image, f) for one byte: float32 d + f * (v - d), clipped to [0, 255], truncated.
__device__ __forceinline__ int blend_byte(int d, int v, float f) {
  const float t = (float)d + f * (float)(v - d);
  return (int)fminf(fmaxf(t, 0.0f), 255.0f);
}
// convert("L") of one RGB pixel
__device__ __forceinline__ int luma(int r, int g, int b) { return (int)((19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16); }

// adjust_hue: RGB -> HSV bytes, H + shift modulo 256, HSV -> RGB bytes.
__device__ __forceinline__ void hue_pixel(int& r, int& g, int& b, int shift) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int H = 0, S = 0;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx) h = bc - gc;
    else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;                 // in [5/6, 11/6): fmod(x, 1.0) is x or the exact x - 1
    h = (float)(x >= 1.0 ? x - 1.0 : x);
    H = min(max((int)((double)h * 255.0), 0), 255);
    S = min(max((int)((double)s * 255.0), 0), 255);
  }
  H = (H + shift) & 255;
  if (S == 0) {
    r = g = b = mx;
    return;
  }
  const double V = (double)mx, hh = (double)H * 6.0 / 255.0, fl = floor(hh), f = hh - fl, s = (double)S / 255.0;
  const int p = (int)floor(V * (1.0 - s) + 0.5), q = (int)floor(V * (1.0 - s * f) + 0.5), t = (int)floor(V * (1.0 - s * (1.0 - f)) + 0.5);
  switch ((int)fl % 6) {
    case 0: r = mx; g = t; b = p; break;
    case 1: r = q; g = mx; b = p; break;
    case 2: r = p; g = mx; b = t; break;
    case 3: r = p; g = q; b = mx; break;
    case 4: r = t; g = p; b = mx; break;
    default: r = mx; g = p; b = q; break;
  }
}

// The block's image: the last entry whose first block is <= the block (block-uniform; images without ops have no entry).
__device__ __forceinline__ int photo_entry(const mi355det_photo_image* __restrict__ table, int m) {
  int lo = 0, hi = m - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Ops [0, upto) of an entry on one pixel.  Brightness and contrast read the block's 256-entry tables, saturation and hue compute.
__device__ __forceinline__ void apply_ops(int& r, int& g, int& b, const mi355det_photo_image& im, int upto, const uint8_t (*lut)[256]) {
  for (int k = 0; k < upto; ++k) {
    const int op = im.op[k];
    if (op == MI355DET_PHOTO_BRIGHTNESS || op == MI355DET_PHOTO_CONTRAST) {
      r = lut[k][r];
      g = lut[k][g];
      b = lut[k][b];
    } else if (op == MI355DET_PHOTO_SATURATION) {
      const int d = luma(r, g, b);
      r = blend_byte(d, r, im.factor[k]);
      g = blend_byte(d, g, im.factor[k]);
      b = blend_byte(d, b, im.factor[k]);
    } else {
      hue_pixel(r, g, b, (int)im.factor[k]);
    }
  }
}

__device__ __forceinline__ int contrast_index(const mi355det_photo_image& im) {
  for (int k = 0; k < im.n_ops; ++k)
    if (im.op[k] == MI355DET_PHOTO_CONTRAST) return k;
  return -1;
}

// The integer sum of L over every image that has a contrast op, of the image as it is after the ops in front of the contrast.  Nothing
// is written to the pixels: the ops are recomputed by the applying launch.  One 64-bit atomic add per block; integers, so any order.
__global__ __launch_bounds__(256) void photo_sum_kernel(const uint8_t* __restrict__ packed, const mi355det_photo_image* __restrict__ table, int m,
                                                        unsigned long long* __restrict__ sums) {
  __shared__ uint8_t lut[MAX_OPS][256];
  __shared__ unsigned part[4];
  const int e = photo_entry(table, m);
  const mi355det_photo_image& im = table[e];                // read where it lies: a copy indexed by k would live in scratch
  const int kc = contrast_index(im);
  if (kc < 0) return;                                       // block-uniform
  for (int k = 0; k < kc; ++k)
    if (im.op[k] == MI355DET_PHOTO_BRIGHTNESS) lut[k][threadIdx.x] = (uint8_t)blend_byte(0, threadIdx.x, im.factor[k]);
  __syncthreads();
  const long long first = ((long long)blockIdx.x - im.first_block) * BLOCK_PIXELS;
  const long long last = min(first + BLOCK_PIXELS, (long long)im.pixels);
  const uint8_t* src = packed + im.offset;
  unsigned acc = 0;                                         // at most 16 pixels of at most 255 per thread
  for (long long p = first + threadIdx.x; p < last; p += 256) {
    int r = src[3 * p], g = src[3 * p + 1], b = src[3 * p + 2];
    apply_ops(r, g, b, im, kc, lut);
    acc += (unsigned)luma(r, g, b);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&sums[e], (unsigned long long)part[0] + part[1] + part[2] + part[3]);
}

// All ops of every entry and its channel permutation, bytes in and bytes out of the packed buffer, one pixel per thread and step.  The
// contrast's degenerate is int(sum / count + 0.5) in float64, formed here from the sum of the launch before.
__global__ __launch_bounds__(256) void photo_apply_kernel(uint8_t* __restrict__ packed, const mi355det_photo_image* __restrict__ table, int m,
                                                          const unsigned long long* __restrict__ sums) {
  __shared__ uint8_t lut[MAX_OPS][256];
  const int e = photo_entry(table, m);
  const mi355det_photo_image& im = table[e];                // read where it lies: a copy indexed by k would live in scratch
  for (int k = 0; k < im.n_ops; ++k) {
    if (im.op[k] == MI355DET_PHOTO_BRIGHTNESS) lut[k][threadIdx.x] = (uint8_t)blend_byte(0, threadIdx.x, im.factor[k]);
    if (im.op[k] == MI355DET_PHOTO_CONTRAST) {
      const int d = (int)((double)sums[e] / (double)im.pixels + 0.5);
      lut[k][threadIdx.x] = (uint8_t)blend_byte(d, threadIdx.x, im.factor[k]);
    }
  }
  __syncthreads();
  const long long first = ((long long)blockIdx.x - im.first_block) * BLOCK_PIXELS;
  const long long last = min(first + BLOCK_PIXELS, (long long)im.pixels);
  uint8_t* px = packed + im.offset;
  for (long long p = first + threadIdx.x; p < last; p += 256) {
    int r = px[3 * p], g = px[3 * p + 1], b = px[3 * p + 2];
    apply_ops(r, g, b, im, im.n_ops, lut);
#pragma unroll
    for (int c = 0; c < 3; ++c) px[3 * p + c] = (uint8_t)(im.perm[c] == 0 ? r : im.perm[c] == 1 ? g : b);     // channel c takes channel perm[c]
  }
}

// The fetch rule of the augmented ingest.  The resize sees the window [crop_h, crop_w] of a canvas on which the source image is pasted at
// (paste_top, paste_left); a tap of the window, mirrored where the image is flipped, is a source pixel or the fill colour.
struct WindowTap {
  using Image = mi355det_ingest_aug_image;
  const uint8_t* base;
  const Image& im;
  __device__ __forceinline__ WindowTap(const uint8_t* packed, const Image& image) : base(packed + image.offset), im(image) {}
  __device__ __forceinline__ int h() const { return im.crop_h; }
  __device__ __forceinline__ int w() const { return im.crop_w; }
  __device__ __forceinline__ const uint8_t* row(int i) const {           // null: a row of the fill
    const int sy = im.crop_top + min(max(i, 0), im.crop_h - 1) - im.paste_top;
    return sy >= 0 && sy < im.h ? base + (long long)sy * im.w * 3 : nullptr;
  }
  __device__ __forceinline__ int col(int i) const {                      // negative: a column of the fill
    const int xw = min(max(i, 0), im.crop_w - 1);
    const int sx = im.crop_left + (im.flip ? im.crop_w - 1 - xw : xw) - im.paste_left;
    return sx >= 0 && sx < im.w ? 3 * sx : -1;
  }
  __device__ __forceinline__ uint8_t byte(const uint8_t* r, int c0, int c) const { return r != nullptr && c0 >= 0 ? r[c0 + c] : (uint8_t)(im.fill_rgb >> (8 * c)); }
};

template <bool VEC>
__global__ __launch_bounds__(256) void ingest_aug_u8_kernel(const uint8_t* __restrict__ packed, const mi355det_ingest_aug_image* __restrict__ table,
                                                            int n, int tiles_x, int total_tiles, const float* __restrict__ mean,
                                                            const float* __restrict__ stdv, float* __restrict__ out, int ph, int pw) {
  ingest_tiles<VEC, WindowTap>(packed, table, n, tiles_x, total_tiles, mean, stdv, out, ph, pw);
}

}  // namespace

extern "C" {

int32_t mi355det_photo_blocks(int64_t pixels) {
  if (pixels <= 0) return 0;
  const long long b = (pixels + BLOCK_PIXELS - 1) / BLOCK_PIXELS;
  return b > INT32_MAX ? 0 : (int32_t)b;
}

int mi355det_photometric_u8(uint8_t* packed, int64_t packed_bytes, const mi355det_photo_image* table, const mi355det_photo_image* table_dev,
                            int32_t m, uint64_t* sums, void* stream) {
  if (m <= 0) return fail(MI355DET_EINVAL, "%s: need m > 0", "photometric_u8");
  if (!packed || !table || !table_dev || !sums) return fail(MI355DET_EINVAL, "%s: null pointer", "photometric_u8");
  long long blocks = 0;
  bool any_contrast = false;
  for (int i = 0; i < m; ++i) {
    const mi355det_photo_image& im = table[i];
    if (im.pixels <= 0 || im.offset < 0 || im.offset > packed_bytes || im.pixels > (packed_bytes - im.offset) / 3)
      return fail(MI355DET_EINVAL, "%s: image %lld lies outside the %lld packed bytes", "photometric_u8", i, packed_bytes);
    if (im.n_ops < 0 || im.n_ops > MAX_OPS) return fail(MI355DET_EINVAL, "%s: image %lld: n_ops outside [0, %lld]", "photometric_u8", i, MAX_OPS);
    int contrasts = 0;
    for (int k = 0; k < im.n_ops; ++k) {
      if (im.op[k] < MI355DET_PHOTO_BRIGHTNESS || im.op[k] > MI355DET_PHOTO_HUE)
        return fail(MI355DET_EINVAL, "%s: image %lld: op code %lld out of range", "photometric_u8", i, im.op[k]);
      if (im.op[k] == MI355DET_PHOTO_HUE) {
        if (!(im.factor[k] >= 0.0f && im.factor[k] <= 255.0f) || im.factor[k] != (float)(int)im.factor[k])
          return fail(MI355DET_EINVAL, "%s: image %lld: a hue op carries its shift, a whole number in [0, 255]", "photometric_u8", i);
      } else if (!(im.factor[k] >= 0.0f && im.factor[k] <= 3.0e38f)) {
        return fail(MI355DET_EINVAL, "%s: image %lld: factor of op %lld is negative or not finite", "photometric_u8", i, k);
      }
      contrasts += im.op[k] == MI355DET_PHOTO_CONTRAST;
    }
    if (contrasts > 1) return fail(MI355DET_EINVAL, "%s: image %lld: more than one contrast op", "photometric_u8", i);
    any_contrast |= contrasts == 1;
    int seen = 0;
    for (int c = 0; c < 3; ++c)
      if (im.perm[c] >= 0 && im.perm[c] <= 2) seen |= 1 << im.perm[c];
    if (seen != 7)
      return fail(MI355DET_EINVAL, "%s: image %lld: perm is not a permutation of 0, 1, 2", "photometric_u8", i);
    if (im.first_block != blocks) return fail(MI355DET_EINVAL, "%s: image %lld: first_block is not %lld", "photometric_u8", i, blocks);
    blocks += mi355det_photo_blocks(im.pixels);
    if (mi355det_photo_blocks(im.pixels) == 0 || blocks > INT32_MAX)
      return fail(MI355DET_EINVAL, "%s: image %lld: too many blocks for one launch", "photometric_u8", i);
  }
  if (any_contrast) {
    if (hipMemsetAsync(sums, 0, sizeof(uint64_t) * m, S(stream)) != hipSuccess) return check_launch("photometric_u8 (clear)");
    hipLaunchKernelGGL(photo_sum_kernel, dim3((int)blocks), dim3(256), 0, S(stream), packed, table_dev, m, (unsigned long long*)sums);
    if (const int e = check_launch("photometric_u8 (sum)")) return e;
  }
  hipLaunchKernelGGL(photo_apply_kernel, dim3((int)blocks), dim3(256), 0, S(stream), packed, table_dev, m, (const unsigned long long*)sums);
  return check_launch("photometric_u8");
}

int mi355det_ingest_aug_u8(const uint8_t* packed, int64_t packed_bytes, const mi355det_ingest_aug_image* table,
                           const mi355det_ingest_aug_image* table_dev, int32_t n, const float* mean, const float* stdv, float* out, int32_t pad_h,
                           int32_t pad_w, void* stream) {
  if (n <= 0) return fail(MI355DET_EINVAL, "%s: need n > 0", "ingest_aug_u8");
  if (!packed || !table || !table_dev || !mean || !stdv || !out) return fail(MI355DET_EINVAL, "%s: null pointer", "ingest_aug_u8");
  const long long tiles = mi355det_ingest_tiles(pad_h, pad_w);
  if (tiles <= 0 || tiles * n > INT32_MAX) return fail(MI355DET_EINVAL, "%s: bad pad, or too many tiles for one launch", "ingest_aug_u8");
  for (int i = 0; i < n; ++i) {
    const mi355det_ingest_aug_image& im = table[i];
    if (im.h <= 0 || im.w <= 0 || im.out_h <= 0 || im.out_w <= 0) return fail(MI355DET_EINVAL, "%s: image %lld: sizes must be > 0", "ingest_aug_u8", i);
    if (pad_h < im.out_h || pad_w < im.out_w) return fail(MI355DET_EINVAL, "%s: image %lld: pad < out", "ingest_aug_u8", i);
    if (im.offset < 0 || im.offset > packed_bytes || (long long)im.h * im.w * 3 > packed_bytes - im.offset)
      return fail(MI355DET_EINVAL, "%s: image %lld lies outside the %lld packed bytes", "ingest_aug_u8", i, packed_bytes);
    if (im.paste_top < 0 || im.paste_left < 0 || (long long)im.paste_top + im.h > im.canvas_h || (long long)im.paste_left + im.w > im.canvas_w)
      return fail(MI355DET_EINVAL, "%s: image %lld: the pasted image lies outside its canvas", "ingest_aug_u8", i);
    if (im.crop_h <= 0 || im.crop_w <= 0) return fail(MI355DET_EINVAL, "%s: image %lld: a window with a zero side", "ingest_aug_u8", i);
    if (im.crop_top < 0 || im.crop_left < 0 || (long long)im.crop_top + im.crop_h > im.canvas_h || (long long)im.crop_left + im.crop_w > im.canvas_w)
      return fail(MI355DET_EINVAL, "%s: image %lld: the crop lies outside its canvas", "ingest_aug_u8", i);
    if (im.first_tile != i * tiles) return fail(MI355DET_EINVAL, "%s: image %lld: first_tile is not i * %lld", "ingest_aug_u8", i, tiles);
  }
  const int total = (int)(tiles * n), grid = min(total, 2048), tiles_x = (pad_w + TILE_W - 1) / TILE_W;
  if (pad_w % 4 == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(ingest_aug_u8_kernel<true>, dim3(grid), dim3(256), 0, S(stream), packed, table_dev, n, tiles_x, total, mean, stdv, out, pad_h, pad_w);
  else
    hipLaunchKernelGGL(ingest_aug_u8_kernel<false>, dim3(grid), dim3(256), 0, S(stream), packed, table_dev, n, tiles_x, total, mean, stdv, out, pad_h, pad_w);
  return check_launch("ingest_aug_u8");
}

}  // extern "C"
