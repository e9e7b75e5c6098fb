// Keypoint branch of Keypoint R-CNN (tvision/roi_heads.py:186-379,891-932, the keypoint parts of tvision/transform.py:169-172,244-275 and
// detection/transforms.py:10-19).  The head and the transposed convolution run on the MFMA convolution kernels (tvision/keypoint_rcnn.py);
// this file holds what is around them:
//
//   flip_resize_keypoints  _flip_coco_person_keypoints where the image is flipped, then resize_keypoints, all keypoints of a batch at once.
//   keypoint_targets       keypoints_to_heatmap for every positive RoI of the batch: heatmap index, valid flag, and the number of valid
//                          (RoI, keypoint) pairs, which stays on the device.
//   keypoint_heatmaps      the predictor's bilinear x2 (align_corners False): sub-pixel 28 x 28 logits -> fp32 [rows, K, 56, 56].
//   keypoint_loss          keypointrcnn_loss fused with that x2: cross entropy over the 3136 logits of every valid pair (mean over the
//                          pairs), its gradient gathered back to the 28 x 28 sub-pixel layout in bf16, the bias gradient of the
//                          transposed convolution.  Fixed summation order, no float atomics: the same bits from run to run.
//   heatmaps_to_keypoints  bicubic upsample of every map to its RoI's size + arg-max, without storing the upsampled map and without a host
//                          read (the reference loops over RoIs on the host).
//
// Sub-pixel layout (keypoint branch): ConvTranspose2d(512, K, 4, 2, 1) runs as a 3x3 convolution to 4 * KP channels, channel
// (2a + b) * KP + k of low-resolution pixel (i, j) = keypoint k at pixel (2i + a, 2j + b) of the 28 x 28 map; KP >= K pads the channels.
//
// Compiled with -ffp-contract=off (build.py): targets, decode and the keypoint resize follow torch's float32 operation order.
#include "common.h"

using namespace mi355;

namespace {

constexpr int LOW = 28, HI = 56, LOW2 = LOW * LOW, HI2 = HI * HI;

__constant__ int c_flip_inds[17] = {0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15};

// One thread per keypoint of the batch.  Flipped image (K == 17: the entry refuses any other K beside a flip): out[g][k] = in[g][flip_inds[k]] with x = width - x,
// and the whole triple zeroed where v == 0; then x *= out_w / w, y *= out_h / h with float32 ratios.
__global__ __launch_bounds__(256) void flip_resize_keypoints_kernel(const float* __restrict__ kp, float* __restrict__ out, long long g, int K,
                                                                    const long long* __restrict__ offsets,
                                                                    const mi355det_ingest_image* __restrict__ table, int n) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t >= g * K) return;
  const long long row = t / K;
  const int k = (int)(t - row * K);
  int lo = 0, hi = n - 1;                                    // the last image whose first row is <= row
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= row) lo = mid; else hi = mid - 1;
  }
  const mi355det_ingest_image im = table[lo];
  const float ratio_h = (float)im.out_h / (float)im.h, ratio_w = (float)im.out_w / (float)im.w;
  const float* s = kp + 3 * (row * K + (im.flip ? c_flip_inds[k] : k));
  float x = s[0], y = s[1], v = s[2];
  if (im.flip) {
    x = (float)im.w - x;
    if (v == 0.f) x = y = v = 0.f;
  }
  float* o = out + 3 * t;
  o[0] = x * ratio_w;
  o[1] = y * ratio_h;
  o[2] = v;
}

// floor().long() of a float32 that may be far outside the heatmap: only [0, size) matters, anything else is "outside"
__device__ __forceinline__ long long floor_to_long(float v) {
  if (!(v >= -4.0e18f && v <= 4.0e18f)) return -1;           // NaN / inf / beyond int64: outside whatever the cast would give
  return (long long)floorf(v);
}

// keypoints_to_heatmap, one thread per (RoI, keypoint).  rois [rows, 5] = (image, x1, y1, x2, y2); the keypoints of all images lie back to
// back in kp [G, K, 3], image b owning rows [kp_offsets[b], kp_offsets[b + 1]).
__global__ __launch_bounds__(256) void keypoint_targets_kernel(const float* __restrict__ kp, const long long* __restrict__ kp_offsets, int n_images,
                                                               const float* __restrict__ rois, const long long* __restrict__ gt_index, int rows,
                                                               int valid_rows, int K, int size, int* __restrict__ target,
                                                               int* __restrict__ valid, int* __restrict__ count) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  int ok = 0, idx = 0;
  if (t < rows * K) {
    const int r = t / K, k = t - r * K;
    const float* roi = rois + 5 * (size_t)r;
    const int b = (int)roi[0];
    if (r < valid_rows && b >= 0 && b < n_images) {
      const long long gi = kp_offsets[b] + gt_index[r];
      if (gt_index[r] >= 0 && gi < kp_offsets[b + 1]) {
        const float* p = kp + 3 * ((size_t)gi * K + k);
        const float x1 = roi[1], y1 = roi[2], x2 = roi[3], y2 = roi[4];
        const float scale_x = (float)size / (x2 - x1), scale_y = (float)size / (y2 - y1);
        const float x = p[0], y = p[1];
        long long xi = floor_to_long((x - x1) * scale_x), yi = floor_to_long((y - y1) * scale_y);
        if (x == x2) xi = size - 1;
        if (y == y2) yi = size - 1;
        ok = xi >= 0 && yi >= 0 && xi < size && yi < size && p[2] > 0.f;
        idx = ok ? (int)(yi * size + xi) : 0;
      }
    }
    target[t] = idx;
    valid[t] = ok;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));       // integer: the order does not matter
}

// the 28 x 28 logits of (row r, keypoint k) out of the sub-pixel convolution output z [rows, 14, 14, ld]
__device__ __forceinline__ void stage_low(const float* __restrict__ z, int ld, int KP, int r, int k, float* low) {
  for (int e = threadIdx.x; e < LOW2; e += 256) {
    const int y = e / LOW, x = e - y * LOW;
    low[e] = z[((size_t)r * 196 + (y >> 1) * 14 + (x >> 1)) * ld + ((y & 1) * 2 + (x & 1)) * KP + k];
  }
}

// F.interpolate(scale_factor=2, mode='bilinear', align_corners=False): source = max((d + 0.5) * 0.5 - 0.5, 0), i1 = min(i0 + 1, 27),
// weights 1 - t and t (0.75 / 0.25, and 1 / 0 on the first pixel); rows blended after columns, as torch's CPU kernel does
struct Lin {
  int i0, i1;
  float w0, w1;
};
__device__ __forceinline__ Lin lin_taps(int d) {
  const float s = fmaxf(((float)d + 0.5f) * 0.5f - 0.5f, 0.f);
  Lin t;
  t.i0 = (int)s;
  t.i1 = min(t.i0 + 1, LOW - 1);
  t.w1 = s - (float)t.i0;
  t.w0 = 1.f - t.w1;
  return t;
}
__device__ __forceinline__ float hi_value(const float* low, int Y, int X) {
  const Lin ty = lin_taps(Y), tx = lin_taps(X);
  const float r0 = low[ty.i0 * LOW + tx.i0] * tx.w0 + low[ty.i0 * LOW + tx.i1] * tx.w1;
  const float r1 = low[ty.i1 * LOW + tx.i0] * tx.w0 + low[ty.i1 * LOW + tx.i1] * tx.w1;
  return r0 * ty.w0 + r1 * ty.w1;
}

__global__ __launch_bounds__(256) void keypoint_heatmaps_kernel(const float* __restrict__ z, int ld, int KP, int K, float* __restrict__ out) {
  __shared__ float low[LOW2];
  const int r = blockIdx.x / K, k = blockIdx.x - r * K;
  stage_low(z, ld, KP, r, k, low);
  __syncthreads();
  float* o = out + (size_t)blockIdx.x * HI2;
  for (int e = threadIdx.x; e < HI2; e += 256) o[e] = hi_value(low, e / HI, e % HI);
}

// block-wide reductions in a fixed order: lanes by butterfly, then the four waves left to right
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// the high-resolution rows that read low-resolution row y, and their weights on it (the transpose of lin_taps): 2y - 1 (0.25), 2y (0.75; 1
// for y = 0), 2y + 1 (0.75; 1 for y = 27, whose second tap is clamped onto it), 2y + 2 (0.25)
__device__ __forceinline__ void contributors(int y, int (&Y)[4], float (&w)[4]) {
  Y[0] = 2 * y - 1; w[0] = y >= 1 ? 0.25f : 0.f;
  Y[1] = 2 * y;     w[1] = y >= 1 ? 0.75f : 1.f;
  Y[2] = 2 * y + 1; w[2] = y <= LOW - 2 ? 0.75f : 1.f;
  Y[3] = 2 * y + 2; w[3] = y <= LOW - 2 ? 0.25f : 0.f;
  Y[0] = max(Y[0], 0);
  Y[3] = min(Y[3], HI - 1);
}

// One workgroup per (row, keypoint): cross entropy of the 56 x 56 logits against target[row][k], and its gradient gathered to 28 x 28.
//   part[2 * (r * K + k)] = lse - logit[target] (0 where the pair is not valid), part[.. + 1] = sum of the pair's 28 x 28 gradient
//   dz [rows, 14, 14, ld] bf16, sub-pixel layout, channel k of each phase; the padded channels are zeroed by the entry
//   dlow (nullable) fp32 [rows, K, 28, 28]: the same gradient before its rounding to bf16
__global__ __launch_bounds__(256) void keypoint_loss_kernel(const float* __restrict__ z, int ld, int KP, int K, const int* __restrict__ target,
                                                            const int* __restrict__ valid, const int* __restrict__ count,
                                                            bf16_t* __restrict__ dz, float* __restrict__ dlow, float* __restrict__ part) {
  __shared__ float low[LOW2];
  __shared__ float hi[HI2];
  __shared__ float red[4];
  const int r = blockIdx.x / K, k = blockIdx.x - r * K;
  const bool live = valid[blockIdx.x] != 0;                  // uniform over the workgroup
  float loss = 0.f, inv_sum = 0.f, inv_n = 0.f;
  const int tgt = target[blockIdx.x];
  if (live) {
    stage_low(z, ld, KP, r, k, low);
    __syncthreads();
    float m = -INFINITY;
    for (int e = threadIdx.x; e < HI2; e += 256) {
      const float v = hi_value(low, e / HI, e % HI);
      hi[e] = v;
      m = fmaxf(m, v);
    }
    m = block_max(m, red);
    float s = 0.f;
    for (int e = threadIdx.x; e < HI2; e += 256) {
      const float ex = expf(hi[e] - m);
      s += ex;
      if (e == tgt) loss = hi[e];                            // the target's logit, held by one thread
      hi[e] = ex;
    }
    s = block_sum(s, red);
    const float at = block_sum(loss, red);
    loss = (m + logf(s)) - at;
    inv_sum = 1.f / s;
    inv_n = 1.f / (float)max(count[0], 1);
  }
  __syncthreads();
  float bsum = 0.f;
  for (int e = threadIdx.x; e < LOW2; e += 256) {
    const int y = e / LOW, x = e - y * LOW;
    float g = 0.f;
    if (live) {
      int Y[4], X[4];
      float wy[4], wx[4];
      contributors(y, Y, wy);
      contributors(x, X, wx);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        float row = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int idx = Y[a] * HI + X[b];
          row += wx[b] * ((hi[idx] * inv_sum - (idx == tgt ? 1.f : 0.f)) * inv_n);
        }
        g += wy[a] * row;
      }
    }
    bsum += g;
    if (dlow) dlow[(size_t)blockIdx.x * LOW2 + e] = g;
    dz[((size_t)r * 196 + (y >> 1) * 14 + (x >> 1)) * ld + ((y & 1) * 2 + (x & 1)) * KP + k] = f2bf(g);
  }
  bsum = block_sum(bsum, red);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = loss;
    part[2 * (size_t)blockIdx.x + 1] = bsum;
  }
}

// block k < K: the bias gradient of keypoint k, rows in order; block K: the loss, pairs in order by a fixed tree
__global__ __launch_bounds__(256) void keypoint_loss_finish_kernel(const float* __restrict__ part, int rows, int K, const int* __restrict__ count,
                                                                   float* __restrict__ loss, float* __restrict__ dbias) {
  __shared__ float red[4];
  const int k = blockIdx.x;
  float a = 0.f;
  if (k < K) {
    for (int r = threadIdx.x; r < rows; r += 256) a += part[2 * ((size_t)r * K + k) + 1];
    a = block_sum(a, red);
    if (threadIdx.x == 0) dbias[k] = a;
  } else {
    for (int e = threadIdx.x; e < rows * K; e += 256) a += part[2 * (size_t)e];
    a = block_sum(a, red);
    const int n = count[0];
    if (threadIdx.x == 0) loss[0] = n > 0 ? a / (float)n : 0.f;
  }
}

// torch's bicubic (A = -0.75) taps of one output coordinate: source = (d + 0.5) * (56 / size) - 0.5 in float32, not clamped; the four
// indices clamped into the map
struct Cubic {
  int i[4];
  float w[4];
};
__device__ __forceinline__ Cubic cubic_taps(int d, float scale) {
  const float A = -0.75f;
  const float real = scale * ((float)d + 0.5f) - 0.5f;
  const int i0 = min((int)floorf(real), HI - 1);
  const float t = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
  Cubic c;
  float x = t + 1.f;
  c.w[0] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
  c.w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  x = 1.f - t;
  c.w[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = x + 1.f;
  c.w[3] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
#pragma unroll
  for (int j = 0; j < 4; ++j) c.i[j] = max(min(i0 + j - 1, HI - 1), 0);
  return c;
}

// One workgroup per (RoI, keypoint): the map in LDS, lanes stride over the pixels of the upsampled map, (value, lowest index) reduced over
// the wavefront and then the workgroup.  The upsampled map is never stored.
__global__ __launch_bounds__(256) void heatmaps_to_keypoints_kernel(const float* __restrict__ maps, const float* __restrict__ rois, int roi_ld,
                                                                    int K, int max_side, float* __restrict__ xy, float* __restrict__ scores) {
  __shared__ float m[HI2];
  __shared__ unsigned long long best[4];
  const int r = blockIdx.x / K;
  const float* src = maps + (size_t)blockIdx.x * HI2;
  for (int e = threadIdx.x; e < HI2; e += 256) m[e] = src[e];
  __syncthreads();
  const float* roi = rois + (size_t)r * roi_ld + (roi_ld - 4);
  const float x1 = roi[0], y1 = roi[1];
  const float w = fmaxf(roi[2] - x1, 1.f), h = fmaxf(roi[3] - y1, 1.f);
  const int wc = min(max((int)ceilf(w), 1), max_side), hc = min(max((int)ceilf(h), 1), max_side);
  const float sx = (float)HI / (float)wc, sy = (float)HI / (float)hc;
  const unsigned total = (unsigned)wc * (unsigned)hc;
  unsigned long long key = 0;
  for (unsigned p = threadIdx.x; p < total; p += 256) {
    const unsigned oy = p / (unsigned)wc, ox = p - oy * (unsigned)wc;
    const Cubic cy = cubic_taps((int)oy, sy), cx = cubic_taps((int)ox, sx);
    float v = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float* row = m + cy.i[a] * HI;
      const float t = ((row[cx.i[0]] * cx.w[0] + row[cx.i[1]] * cx.w[1]) + row[cx.i[2]] * cx.w[2]) + row[cx.i[3]] * cx.w[3];
      v = a == 0 ? t * cy.w[0] : v + t * cy.w[a];
    }
    // larger value first, then the lower index: one unsigned maximum (p grows along the loop, so `>` keeps the first of equals)
    const unsigned long long cand = ((unsigned long long)f2ord(v) << 32) | (0xFFFFFFFFu - p);
    key = cand > key ? cand : key;
  }
  key = wave_max_u64(key);
  if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = best[0];
    for (int i = 1; i < 4; ++i) b = best[i] > b ? best[i] : b;
    const unsigned pos = 0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFu);
    const unsigned x_int = pos % (unsigned)wc, y_int = (pos - x_int) / (unsigned)wc;
    float* o = xy + 3 * (size_t)blockIdx.x;
    o[0] = ((float)x_int + 0.5f) * (w / (float)wc) + x1;
    o[1] = ((float)y_int + 0.5f) * (h / (float)hc) + y1;
    o[2] = 1.f;
    scores[blockIdx.x] = ord2f((unsigned)(b >> 32));
  }
}

}  // namespace

extern "C" {

int mi355det_flip_resize_keypoints(const float* keypoints, float* out, int64_t g, int32_t num_keypoints, const int64_t* kp_offsets,
                                   const mi355det_ingest_image* table, const mi355det_ingest_image* table_dev, int32_t n, void* stream) {
  if (n <= 0 || g < 0 || num_keypoints < 1) return fail(MI355DET_EINVAL, "%s: need n > 0, g >= 0 and num_keypoints > 0", "flip_resize_keypoints");
  if (!kp_offsets || !table || !table_dev) return fail(MI355DET_EINVAL, "%s: null table", "flip_resize_keypoints");
  for (int i = 0; i < n; ++i)          // the flip is the COCO person permutation of 17 indices (detection/transforms.py:10-19)
    if (table[i].flip && num_keypoints != 17)
      return fail(MI355DET_EINVAL, "%s: image %lld is flipped, which needs 17 keypoints (got %lld)", "flip_resize_keypoints", i, num_keypoints);
  if (g == 0) return MI355DET_OK;
  if (!keypoints || !out) return fail(MI355DET_EINVAL, "%s: null keypoints", "flip_resize_keypoints");
  const long long total = (long long)g * num_keypoints;
  if (total > 0x7FFFFFFFll * 64) return fail(MI355DET_EINVAL, "%s: too many keypoints for one launch", "flip_resize_keypoints");
  hipLaunchKernelGGL(flip_resize_keypoints_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(stream), keypoints, out, (long long)g,
                     num_keypoints, (const long long*)kp_offsets, table_dev, n);
  return check_launch("flip_resize_keypoints");
}

int mi355det_keypoint_targets(const float* keypoints, const int64_t* kp_offsets, int32_t n_images, const float* rois, const int64_t* gt_index,
                              int32_t rows, int32_t valid_rows, int32_t num_keypoints, int32_t heatmap_size, int32_t* target, int32_t* valid,
                              int32_t* count, void* stream) {
  if (n_images < 1 || rows < 0 || valid_rows < 0 || valid_rows > rows || num_keypoints < 1 || heatmap_size < 1 || heatmap_size > 4096 || !count)
    return fail(MI355DET_EINVAL, "%s: bad arguments", "keypoint_targets");
  if ((long long)rows * num_keypoints > 0x7FFFFFFFll) return fail(MI355DET_EINVAL, "%s: too many pairs for one launch", "keypoint_targets");
  if (hipMemsetAsync(count, 0, sizeof(int32_t), S(stream)) != hipSuccess) return fail(MI355DET_ELAUNCH, "%s: memset failed", "keypoint_targets");
  if (rows == 0) return MI355DET_OK;
  if (!kp_offsets || !rois || !gt_index || !target || !valid || (valid_rows > 0 && !keypoints))
    return fail(MI355DET_EINVAL, "%s: missing operand", "keypoint_targets");
  const int total = rows * num_keypoints;
  hipLaunchKernelGGL(keypoint_targets_kernel, dim3((total + 255) / 256), dim3(256), 0, S(stream), keypoints, (const long long*)kp_offsets, n_images,
                     rois, (const long long*)gt_index, rows, valid_rows, num_keypoints, heatmap_size, target, valid, count);
  return check_launch("keypoint_targets");
}

static int check_logits(const char* what, const void* z, int32_t ld, int32_t kp, int32_t rows, int32_t k) {
  if (rows < 0 || k < 1 || kp < k || ld < 4 * kp) return fail(MI355DET_EINVAL, "%s: bad arguments (need rows >= 0, 1 <= K <= KP, ld >= 4 KP)", what);
  if ((long long)rows * k > 0x7FFFFFFFll) return fail(MI355DET_EINVAL, "%s: too many (row, keypoint) pairs for one launch", what);
  if (rows > 0 && !z) return fail(MI355DET_EINVAL, "%s: null logits", what);
  return MI355DET_OK;
}

int mi355det_keypoint_heatmaps(const float* logits, int32_t logits_ld, int32_t padded_keypoints, int32_t rows, int32_t num_keypoints,
                               float* out, void* stream) {
  if (int e = check_logits("keypoint_heatmaps", logits, logits_ld, padded_keypoints, rows, num_keypoints)) return e;
  if (rows == 0) return MI355DET_OK;
  if (!out) return fail(MI355DET_EINVAL, "%s: null output", "keypoint_heatmaps");
  hipLaunchKernelGGL(keypoint_heatmaps_kernel, dim3(rows * num_keypoints), dim3(256), 0, S(stream), logits, logits_ld, padded_keypoints,
                     num_keypoints, out);
  return check_launch("keypoint_heatmaps");
}

size_t mi355det_keypoint_loss_workspace(int32_t rows, int32_t num_keypoints) {
  return rows > 0 && num_keypoints > 0 ? (size_t)rows * num_keypoints * 2 * sizeof(float) : 0;
}

int mi355det_keypoint_loss(const float* logits, int32_t logits_ld, int32_t padded_keypoints, int32_t rows, int32_t num_keypoints,
                           const int32_t* target, const int32_t* valid, const int32_t* count, float* loss, void* dlogits, float* dlogits_f32,
                           float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = check_logits("keypoint_loss", logits, logits_ld, padded_keypoints, rows, num_keypoints)) return e;
  if (!loss || !dbias || !count) return fail(MI355DET_EINVAL, "%s: null output", "keypoint_loss");
  if (rows > 0 && (!target || !valid || !dlogits)) return fail(MI355DET_EINVAL, "%s: missing operand", "keypoint_loss");
  if (workspace_bytes < mi355det_keypoint_loss_workspace(rows, num_keypoints) || (rows > 0 && !workspace))
    return fail(MI355DET_EWORKSPACE, "%s: workspace too small", "keypoint_loss");
  if (rows > 0) {
    // the padded channels of the gradient (and the pitch padding) carry zeros
    if (hipMemsetAsync(dlogits, 0, (size_t)rows * 196 * logits_ld * sizeof(bf16_t), S(stream)) != hipSuccess)
      return fail(MI355DET_ELAUNCH, "%s: memset failed", "keypoint_loss");
    hipLaunchKernelGGL(keypoint_loss_kernel, dim3(rows * num_keypoints), dim3(256), 0, S(stream), logits, logits_ld, padded_keypoints,
                       num_keypoints, target, valid, count, (bf16_t*)dlogits, dlogits_f32, (float*)workspace);
  }
  // rows == 0 or no valid pair: loss 0 and zero gradients (roi_heads.py:351-352: keypoint_logits.sum() * 0)
  hipLaunchKernelGGL(keypoint_loss_finish_kernel, dim3(num_keypoints + 1), dim3(256), 0, S(stream), (const float*)workspace, rows, num_keypoints,
                     count, loss, dbias);
  return check_launch("keypoint_loss");
}

int mi355det_heatmaps_to_keypoints(const float* maps, const float* rois, int32_t roi_ld, int32_t rows, int32_t num_keypoints, float* xy,
                                   float* scores, void* stream) {
  if (rows < 0 || num_keypoints < 1 || (roi_ld != 4 && roi_ld != 5)) return fail(MI355DET_EINVAL, "%s: bad arguments", "heatmaps_to_keypoints");
  if ((long long)rows * num_keypoints > 0x7FFFFFFFll) return fail(MI355DET_EINVAL, "%s: too many pairs for one launch", "heatmaps_to_keypoints");
  if (rows == 0) return MI355DET_OK;
  if (!maps || !rois || !xy || !scores) return fail(MI355DET_EINVAL, "%s: missing operand", "heatmaps_to_keypoints");
  hipLaunchKernelGGL(heatmaps_to_keypoints_kernel, dim3(rows * num_keypoints), dim3(256), 0, S(stream), maps, rois, roi_ld, num_keypoints,
                     MI355DET_KEYPOINT_MAX_SIDE, xy, scores);
  return check_launch("heatmaps_to_keypoints");
}

}  // extern "C"
