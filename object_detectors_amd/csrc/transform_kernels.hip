// Input-side transform of the detection step: GeneralizedRCNNTransform (torchvision_models/tvision/transform.py:88-226:
// normalize -> bilinear resize (align_corners=False) -> zero-pad into the batch tensor), resize_boxes (:279-293) and the YOLO multi-scale
// F.interpolate (yolo/procedures/train_one_epoch.py:64-69).  HBM-bound: every output element is written once, every input element read ~once
// (the four taps of neighbouring outputs hit the same lines).  The uint8 route (mi355det_ingest_u8, mi355det_flip_resize_boxes) does the
// same for a whole batch of decoded HWC images in one launch each, with the horizontal flip of detection/transforms.py:30-44 folded in.
#include "common.h"
#include "ingest_body.h"

using namespace mi355;

namespace {

// out[p][y][x] for planes p of one image (or of a same-size batch): bilinear sample of (in - mean[p % c]) / std[p % c], zero outside [oh, ow].
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ in, int planes, int c, int h, int w, const float* __restrict__ mean,
                                                              const float* __restrict__ stdv, float* __restrict__ out, int oh, int ow, int ph, int pw,
                                                              float rh, float rw) {
  const long long total = (long long)planes * ph * pw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % pw);
    const long long t = i / pw;
    const int y = (int)(t % ph), p = (int)(t / ph);
    float v = 0.0f;
    if (y < oh && x < ow) {
      const Taps ty = bilinear_taps(rh, y, h), tx = bilinear_taps(rw, x, w);
      const float* src = in + (size_t)p * h * w;
      float v00 = src[(size_t)ty.i0 * w + tx.i0], v01 = src[(size_t)ty.i0 * w + tx.i1], v10 = src[(size_t)ty.i1 * w + tx.i0],
            v11 = src[(size_t)ty.i1 * w + tx.i1];
      if (mean) {
        const float m = mean[p % c], s = stdv[p % c];
        v00 = (v00 - m) / s;
        v01 = (v01 - m) / s;
        v10 = (v10 - m) / s;
        v11 = (v11 - m) / s;
      }
      v = bilinear_blend(v00, v01, v10, v11, ty, tx);
    }
    out[i] = v;
  }
}

// The same for a batch of uint8 HWC images of any sizes, packed back to back, in one launch: the tile loop of ingest_body.h with the plain
// fetch rule.  A tap is a pixel of the image itself, column w - 1 - x where the image is flipped.
struct PlainTap {
  using Image = mi355det_ingest_image;
  const uint8_t* packed;
  const Image& im;
  __device__ __forceinline__ PlainTap(const uint8_t* packed_, const Image& image) : packed(packed_), im(image) {}
  __device__ __forceinline__ int h() const { return im.h; }
  __device__ __forceinline__ int w() const { return im.w; }
  __device__ __forceinline__ const uint8_t* row(int i) const { return packed + im.offset + (long long)i * im.w * 3; }
  __device__ __forceinline__ int col(int i) const { return 3 * (im.flip ? im.w - 1 - i : i); }
  __device__ __forceinline__ uint8_t byte(const uint8_t* r, int c0, int c) const { return r[c0 + c]; }
};

template <bool VEC>
__global__ __launch_bounds__(256) void ingest_u8_kernel(const uint8_t* __restrict__ packed, const mi355det_ingest_image* __restrict__ table, int n,
                                                        int tiles_x, int total_tiles, const float* __restrict__ mean,
                                                        const float* __restrict__ stdv, float* __restrict__ out, int ph, int pw) {
  ingest_tiles<VEC, PlainTap>(packed, table, n, tiles_x, total_tiles, mean, stdv, out, ph, pw);
}

__global__ void resize_boxes_kernel(const float* __restrict__ boxes, float* __restrict__ out, long long n, float ratio_h, float ratio_w) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 4) return;
  out[i] = boxes[i] * ((i & 1) ? ratio_h : ratio_w);       // (xmin, ymin, xmax, ymax): x by the width ratio, y by the height ratio
}

// One thread per box of the whole batch: RandomHorizontalFlip's `boxes[:, [0, 2]] = width - boxes[:, [2, 0]]` where the image is flipped,
// then resize_boxes_kernel's multiply with the float32 ratios out / in of the box's image.
__global__ __launch_bounds__(256) void flip_resize_boxes_kernel(const float* __restrict__ boxes, float* __restrict__ out, long long g,
                                                                const long long* __restrict__ box_offsets,
                                                                const mi355det_ingest_image* __restrict__ table, int n) {
  const long long b = blockIdx.x * 256ll + threadIdx.x;
  if (b >= g) return;
  int lo = 0, hi = n - 1;                                    // the last image whose first row is <= b (an image without boxes owns no row)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (box_offsets[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const mi355det_ingest_image im = table[lo];
  const float ratio_h = (float)im.out_h / (float)im.h, ratio_w = (float)im.out_w / (float)im.w;
  float x0 = boxes[4 * b], x2 = boxes[4 * b + 2];
  if (im.flip) {
    const float w = (float)im.w, f0 = w - x2, f2 = w - x0;
    x0 = f0;
    x2 = f2;
  }
  out[4 * b] = x0 * ratio_w;
  out[4 * b + 1] = boxes[4 * b + 1] * ratio_h;
  out[4 * b + 2] = x2 * ratio_w;
  out[4 * b + 3] = boxes[4 * b + 3] * ratio_h;
}

}  // namespace

extern "C" {

int mi355det_resize_bilinear(const float* in, int32_t planes, int32_t c, int32_t h, int32_t w, const float* mean, const float* stdv, float* out,
                             int32_t out_h, int32_t out_w, int32_t pad_h, int32_t pad_w, void* stream) {
  if (planes <= 0 || c <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0 || pad_h < out_h || pad_w < out_w)
    return fail(MI355DET_EINVAL, "%s: bad geometry (need planes, sizes > 0 and pad >= out)", "resize_bilinear");
  if ((mean == nullptr) != (stdv == nullptr)) return fail(MI355DET_EINVAL, "%s: mean and std come together", "resize_bilinear");
  const float rh = (float)h / (float)out_h, rw = (float)w / (float)out_w;      // recompute_scale_factor / size= : scale from the two sizes
  const long long total = (long long)planes * pad_h * pad_w;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((int)min((long long)8192, (total + 255) / 256)), dim3(256), 0, S(stream), in, planes, c, h, w, mean, stdv,
                     out, out_h, out_w, pad_h, pad_w, rh, rw);
  return check_launch("resize_bilinear");
}

int mi355det_resize_boxes(const float* boxes, float* out, int64_t n, int32_t orig_h, int32_t orig_w, int32_t new_h, int32_t new_w, void* stream) {
  if (n < 0 || orig_h <= 0 || orig_w <= 0) return fail(MI355DET_EINVAL, "%s: bad sizes", "resize_boxes");
  if (n == 0) return 0;
  const float rh = (float)new_h / (float)orig_h, rw = (float)new_w / (float)orig_w;
  hipLaunchKernelGGL(resize_boxes_kernel, dim3((int)((n * 4 + 255) / 256)), dim3(256), 0, S(stream), boxes, out, (long long)n, rh, rw);
  return check_launch("resize_boxes");
}

int32_t mi355det_ingest_tiles(int32_t pad_h, int32_t pad_w) {
  if (pad_h <= 0 || pad_w <= 0) return 0;
  const long long t = (long long)((pad_h + TILE_H - 1) / TILE_H) * ((pad_w + TILE_W - 1) / TILE_W);
  return t > INT32_MAX ? 0 : (int32_t)t;
}

int mi355det_ingest_u8(const uint8_t* packed, int64_t packed_bytes, const mi355det_ingest_image* table, const mi355det_ingest_image* table_dev,
                       int32_t n, const float* mean, const float* stdv, float* out, int32_t pad_h, int32_t pad_w, void* stream) {
  if (n <= 0) return fail(MI355DET_EINVAL, "%s: need n > 0", "ingest_u8");
  if (!packed || !table || !table_dev || !mean || !stdv || !out) return fail(MI355DET_EINVAL, "%s: null pointer", "ingest_u8");
  const long long tiles = mi355det_ingest_tiles(pad_h, pad_w);
  if (tiles <= 0 || tiles * n > INT32_MAX) return fail(MI355DET_EINVAL, "%s: bad pad, or too many tiles for one launch", "ingest_u8");
  for (int i = 0; i < n; ++i) {
    const mi355det_ingest_image& im = table[i];
    if (im.h <= 0 || im.w <= 0 || im.out_h <= 0 || im.out_w <= 0) return fail(MI355DET_EINVAL, "%s: image %lld: sizes must be > 0", "ingest_u8", i);
    if (pad_h < im.out_h || pad_w < im.out_w) return fail(MI355DET_EINVAL, "%s: image %lld: pad < out", "ingest_u8", i);
    if (im.offset < 0 || im.offset > packed_bytes || (long long)im.h * im.w * 3 > packed_bytes - im.offset)
      return fail(MI355DET_EINVAL, "%s: image %lld lies outside the %lld packed bytes", "ingest_u8", i, packed_bytes);
    if (im.first_tile != i * tiles) return fail(MI355DET_EINVAL, "%s: image %lld: first_tile is not i * %lld", "ingest_u8", i, tiles);
  }
  const int total = (int)(tiles * n), grid = min(total, 2048), tiles_x = (pad_w + TILE_W - 1) / TILE_W;
  if (pad_w % 4 == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(ingest_u8_kernel<true>, dim3(grid), dim3(256), 0, S(stream), packed, table_dev, n, tiles_x, total, mean, stdv, out, pad_h, pad_w);
  else
    hipLaunchKernelGGL(ingest_u8_kernel<false>, dim3(grid), dim3(256), 0, S(stream), packed, table_dev, n, tiles_x, total, mean, stdv, out, pad_h, pad_w);
  return check_launch("ingest_u8");
}

int mi355det_flip_resize_boxes(const float* boxes, float* out, int64_t g, const int64_t* box_offsets, const mi355det_ingest_image* table_dev,
                               int32_t n, void* stream) {
  if (n <= 0 || g < 0) return fail(MI355DET_EINVAL, "%s: need n > 0 and g >= 0", "flip_resize_boxes");
  if (!box_offsets || !table_dev) return fail(MI355DET_EINVAL, "%s: null table", "flip_resize_boxes");
  if (g == 0) return MI355DET_OK;
  if (!boxes || !out) return fail(MI355DET_EINVAL, "%s: null boxes", "flip_resize_boxes");
  hipLaunchKernelGGL(flip_resize_boxes_kernel, dim3((int)((g + 255) / 256)), dim3(256), 0, S(stream), boxes, out, (long long)g,
                     (const long long*)box_offsets, table_dev, n);
  return check_launch("flip_resize_boxes");
}

}  // extern "C"

// ---- output side: kept detections -> the numbers of the COCO result dicts -------------------------------------
// yolo/procedures/test_one_epoch.py:41-66: rows [k,6] = (x1,y1,x2,y2,score,label) in network pixels -> bbox (xmin, ymin, w, h) in the
// ORIGINAL image's pixels (x / inp_dim * W, y / inp_dim * H), area = w*h, category id (80 -> 91 COCO map, or label + 1).
// torchvision_models/detection/coco_eval.py:83-105,169-171: convert_to_xywh = the same with inp_dim = W = H = 1 and labels untouched.
namespace {

__constant__ int c_coco80to91[80] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 31, 32, 33, 34,
                                     35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63,
                                     64, 65, 67, 70, 72, 73, 74, 75, 76, 77, 78, 79, 80, 81, 82, 84, 85, 86, 87, 88, 89, 90};

__global__ void coco_rows_kernel(const float* __restrict__ boxes, int box_ld, const float* __restrict__ labels_f, const long long* __restrict__ labels_i,
                                 int lab_ld, long long k, float inp_dim, float img_h, float img_w, int scale, int label_mode, float* __restrict__ bbox,
                                 float* __restrict__ area, long long* __restrict__ cat) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const float* r = boxes + i * box_ld;
  float xmin = r[0], ymin = r[1], xmax = r[2], ymax = r[3];
  if (scale) {
    xmin = xmin / inp_dim * img_w;
    ymin = ymin / inp_dim * img_h;
    xmax = xmax / inp_dim * img_w;
    ymax = ymax / inp_dim * img_h;
  }
  const float w = xmax - xmin, h = ymax - ymin;
  bbox[i * 4 + 0] = xmin;
  bbox[i * 4 + 1] = ymin;
  bbox[i * 4 + 2] = w;
  bbox[i * 4 + 3] = h;
  if (area) area[i] = w * h;
  if (cat) {
    const long long l = labels_i ? labels_i[i * lab_ld] : (long long)labels_f[i * lab_ld];     // (atrbs[:,5]).long()
    cat[i] = label_mode == 1 ? (long long)c_coco80to91[l < 0 ? 0 : (l > 79 ? 79 : l)] : label_mode == 0 ? l + 1 : l;
  }
}

}  // namespace

extern "C" int mi355det_coco_rows(const float* boxes, int32_t box_ld, const float* labels_f32, const int64_t* labels_i64, int32_t label_ld, int64_t k,
                                  float inp_dim, float img_h, float img_w, int32_t scale, int32_t label_mode, float* bbox_xywh, float* area,
                                  int64_t* category_id, void* stream) {
  if (k < 0 || box_ld < 4 || (scale && !(inp_dim > 0.f))) return fail(MI355DET_EINVAL, "%s: bad arguments", "coco_rows");
  if (label_mode < 0 || label_mode > 2) return fail(MI355DET_EINVAL, "%s: label_mode 0 (+1), 1 (COCO 80->91) or 2 (as is)", "coco_rows");
  if (category_id && !labels_f32 && !labels_i64) return fail(MI355DET_EINVAL, "%s: category ids need labels", "coco_rows");
  if (k == 0) return 0;
  hipLaunchKernelGGL(coco_rows_kernel, dim3((int)((k + 255) / 256)), dim3(256), 0, S(stream), boxes, box_ld, labels_f32, (const long long*)labels_i64,
                     label_ld, (long long)k, inp_dim, img_h, img_w, scale, label_mode, bbox_xywh, area, (long long*)category_id);
  return check_launch("coco_rows");
}
