// Mask branch of Mask R-CNN (tvision/mask_rcnn.py:21-300, tvision/roi_heads.py:99-183,403-537,844-887, the masks parts of
// tvision/transform.py:26-62,228-247).  bf16 storage, fp32 arithmetic; the R-CNN path is bf16-only, so there are no fp16 twins.
//
//   mask_targets         project_masks_on_boxes: roi_align(gt_masks[:, None].float(), [matched_idx, box], (M, M), 1.0) with torchvision's
//                        defaults sampling_ratio = -1 (adaptive) and aligned = False, on the uint8 masks of every image in one launch.
//   mask_loss            mask_fcn_logits (1x1, 256 -> K) restricted to the label channel + binary_cross_entropy_with_logits(mean), fused,
//                        with every gradient the backward needs; mask_probs is its forward-only form (maskrcnn_inference).
//   mask_resize_nearest  F.interpolate(mask[:, None].float(), ..., mode='nearest')[:, 0].byte() with torch's source-index rule; with the
//                        flip flag, of masks.flip(-1) (detection/transforms.py:38-39) without the flipped copy.
//   paste_masks          paste_masks_in_image (expand_masks, expand_boxes, per-box bilinear resize, clipped paste), each output pixel once.
//
// The branch's pooling, MultiScaleRoIAlign(['0'..'3'], 14, 2) into the conv layout (mi355det_mask_roi_pool), is the per-sample channels-last
// kernel of roi_kernels.hip with a bf16 NHWC store.
//
// The ConvTranspose2d(256, 256, 2, stride=2) of the mask predictor has no kernel here: with kernel == stride its output pixel (2i+di, 2j+dj)
// depends on input pixel (i, j) only, so it IS the 1x1 convolution 256 -> 4*256 of the existing MFMA kernels (conv_fwd_ex / conv_dgrad_mask /
// conv_wgrad) with output channel q*256 + co, q = 2*di + dj.  Its output stays in that sub-pixel order [R, 14, 14, 4, 256]; mask_loss and
// mask_probs do the depth-to-space in their indexing (mask branch).
//
// Compiled with -ffp-contract=off (build.py): the targets (on the RoIAlign rules of roi_sample.h), the nearest index and the paste follow
// torch's CPU float32 operation order.
#include "common.h"
#include "mask_paste.h"
#include "roi_sample.h"

using namespace mi355;

namespace {

struct MaskImages {
  const uint8_t* masks[MI355DET_MASK_MAX_IMAGES];
  int h[MI355DET_MASK_MAX_IMAGES], w[MI355DET_MASK_MAX_IMAGES];
};

// torchvision roi_align (CPU kernel order) on one uint8 mask plane per RoI: spatial_scale 1, aligned = False, adaptive sampling.
__global__ __launch_bounds__(256) void mask_targets_kernel(MaskImages I, int n_images, const float* __restrict__ rois,
                                                           const int64_t* __restrict__ gt_index, int R, int M, float* __restrict__ out) {
  const long long total = (long long)R * M * M;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int px = (int)(i % M);
    const int py = (int)((i / M) % M);
    const int k = (int)(i / ((long long)M * M));
    const float* r = rois + 5 * (size_t)k;
    const int b = (int)r[0];
    if (b < 0 || b >= n_images) {
      out[i] = 0.f;
      continue;
    }
    const int H = I.h[b], W = I.w[b];
    const uint8_t* m = I.masks[b] + (size_t)gt_index[k] * H * W;
    const RoiBins B = roi_bins(make_float4(r[1], r[2], r[3], r[4]), 1.0f, false, M, M, 0);
    float acc = 0.f;
    for (int iy = 0; iy < B.gh; ++iy) {
      const float y = bin_sample(B.y1, py, B.bh, iy, B.gh);
      for (int ix = 0; ix < B.gw; ++ix) {
        const float x = bin_sample(B.x1, px, B.bw, ix, B.gw);
        RoiCorners q;
        if (!roi_corners(y, x, H, W, q)) continue;
        const float w1 = q.hy * q.hx, w2 = q.hy * q.lx, w3 = q.ly * q.hx, w4 = q.ly * q.lx;
        acc += w1 * (float)m[(size_t)q.yl * W + q.xl] + w2 * (float)m[(size_t)q.yl * W + q.xh] + w3 * (float)m[(size_t)q.yh * W + q.xl] +
               w4 * (float)m[(size_t)q.yh * W + q.xh];
      }
    }
    out[i] = acc / B.cnt;
  }
}

// Fused mask_fcn_logits (label channel only) + BCE-with-logits.  One workgroup (4 waves) per RoI; lane l owns channels 4l..4l+3 of the 256
// (one 8-byte load per logit and lane), each wave walks 196 of the 784 = 14*14*4 sub-pixels.  F = feat[(r*196 + i*14 + j)*ld + q*256 + c]
// is the deconvolution output (after its ReLU) in sub-pixel order; its pixel in the 28x28 mask is (2i + di, 2j + dj), q = 2*di + dj.
//   TRAIN:  loss partial, dF = dlogit * W[label] * (F > 0) (the gradient BEFORE the deconvolution's ReLU, bf16), per-RoI partials of
//           dW[label] (sum dlogit * F), db[label] (sum dlogit) and of the deconvolution bias (sum over the RoI's dF of its bf16 value).
//           Rows >= valid (bucket padding) get zero everywhere.
//   !TRAIN: probs[r][28*28] = sigmoid(logit) (maskrcnn_inference).
#define MASK_PART 516              // floats per RoI partial: dW[256] | dbias_deconv[256] | db | loss | pad
template <bool TRAIN>
__global__ __launch_bounds__(256) void mask_loss_kernel(const bf16_t* __restrict__ feat, int ld, const float* __restrict__ wl,
                                                        const float* __restrict__ bl, const int64_t* __restrict__ labels, int K, int valid,
                                                        const float* __restrict__ tgt, float inv_n, bf16_t* __restrict__ dfeat,
                                                        float* __restrict__ part, float* __restrict__ probs) {
  __shared__ float red[4][2 * 256 + 2];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = !TRAIN || r < valid;
  long long lab = labels[r];
  lab = lab < 0 ? 0 : (lab >= K ? K - 1 : lab);
  const float4 w = *(const float4*)(wl + lab * 256 + 4 * lane);
  const float b = bl[lab];
  float dw[4] = {0.f, 0.f, 0.f, 0.f}, dd[4] = {0.f, 0.f, 0.f, 0.f}, dbs = 0.f, ls = 0.f;
  for (int s = wave; s < 784; s += 4) {
    const int p = s >> 2, q = s & 3;                       // p = i*14 + j
    const size_t off = ((size_t)r * 196 + p) * ld + q * 256 + 4 * lane;
    const uint2 raw = *(const uint2*)(feat + off);
    const float f0 = __uint_as_float(raw.x << 16), f1 = __uint_as_float(raw.x & 0xffff0000u);
    const float f2 = __uint_as_float(raw.y << 16), f3 = __uint_as_float(raw.y & 0xffff0000u);
    float dot = f0 * w.x + f1 * w.y + f2 * w.z + f3 * w.w;
    dot = wave_sum(dot);
    const float x = dot + b;
    const int oy = 2 * (p / 14) + (q >> 1), ox = 2 * (p % 14) + (q & 1);
    const float sg = 1.f / (1.f + expf(-x));
    if (!TRAIN) {
      if (lane == 0) probs[(size_t)r * 784 + oy * 28 + ox] = sg;
      continue;
    }
    float g = 0.f;
    if (live) {
      const float t = tgt[(size_t)r * 784 + oy * 28 + ox];
      ls += fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
      g = (sg - t) * inv_n;
    }
    const bf16_t g0 = f2bf(f0 > 0.f ? g * w.x : 0.f), g1 = f2bf(f1 > 0.f ? g * w.y : 0.f);
    const bf16_t g2 = f2bf(f2 > 0.f ? g * w.z : 0.f), g3 = f2bf(f3 > 0.f ? g * w.w : 0.f);
    uint2 o;
    o.x = (unsigned)g0 | ((unsigned)g1 << 16);
    o.y = (unsigned)g2 | ((unsigned)g3 << 16);
    *(uint2*)(dfeat + off) = o;
    dw[0] += g * f0; dw[1] += g * f1; dw[2] += g * f2; dw[3] += g * f3;
    dd[0] += bf2f(g0); dd[1] += bf2f(g1); dd[2] += bf2f(g2); dd[3] += bf2f(g3);
    dbs += g;
  }
  if (!TRAIN) return;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    red[wave][4 * lane + u] = dw[u];
    red[wave][256 + 4 * lane + u] = dd[u];
  }
  if (lane == 0) {
    red[wave][512] = dbs;
    red[wave][513] = ls;
  }
  __syncthreads();
  float* pr = part + (size_t)r * MASK_PART;
  for (int e = threadIdx.x; e < 514; e += 256) pr[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

// Fixed-order reductions of the per-RoI partials: block k < K sums dW / db of the RoIs labelled k in RoI order (segmented sum, every
// class row written, zeros for absent classes); block K sums the deconvolution bias gradient; block K + 1 the loss.
__global__ __launch_bounds__(256) void mask_loss_finish_kernel(const float* __restrict__ part, const int64_t* __restrict__ labels, int valid,
                                                               int K, float inv_n, float* __restrict__ loss, float* __restrict__ dw,
                                                               float* __restrict__ db, float* __restrict__ dbias) {
  __shared__ float red[256];
  const int k = blockIdx.x, t = threadIdx.x;
  if (k < K) {
    float a = 0.f, c = 0.f;
    for (int r = 0; r < valid; ++r) {
      long long lab = labels[r];
      lab = lab < 0 ? 0 : (lab >= K ? K - 1 : lab);
      if (lab != k) continue;
      a += part[(size_t)r * MASK_PART + t];
      c += part[(size_t)r * MASK_PART + 512];
    }
    if (dw) dw[(size_t)k * 256 + t] = a;
    if (db && t == 0) db[k] = c;
  } else if (k == K) {
    float a = 0.f;
    for (int r = 0; r < valid; ++r) a += part[(size_t)r * MASK_PART + 256 + t];
    if (dbias) dbias[t] = a;
  } else {
    float a = 0.f;
    for (int r = t; r < valid; r += 256) a += part[(size_t)r * MASK_PART + 513];
    red[t] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) red[t] += red[t + s];
      __syncthreads();
    }
    if (t == 0) loss[0] = red[0] * inv_n;
  }
}

// torch nearest: identical sizes copy, doubling takes dst >> 1, else min(floor(dst * (float)in / out), in - 1) in float32
__device__ __forceinline__ int nearest_src(int dst, int in, int out) {
  if (out == in) return dst;
  if (out == 2 * in) return dst >> 1;
  const float scale = (float)in / (float)out;
  return min((int)floorf((float)dst * scale), in - 1);
}

// flip: the resize of masks.flip(-1) (RandomHorizontalFlip ahead of the transform), source column w - 1 - x
__global__ __launch_bounds__(256) void mask_resize_nearest_kernel(const uint8_t* __restrict__ in, int planes, int h, int w,
                                                                  uint8_t* __restrict__ out, int oh, int ow, int flip) {
  const long long total = (long long)planes * oh * ow;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % ow);
    const int y = (int)((i / ow) % oh);
    const long long p = i / ((long long)ow * oh);
    const int sx = nearest_src(x, w, ow);
    out[i] = in[(size_t)p * h * w + (size_t)nearest_src(y, h, oh) * w + (flip ? w - 1 - sx : sx)];
  }
}

// paste_masks_in_image for the D detections of one image: out [D, H, W], every pixel written once (the per-pixel rule: mask_paste.h).
__global__ __launch_bounds__(256) void paste_masks_kernel(const float* __restrict__ masks, const float* __restrict__ boxes, int D, int M, int pad,
                                                          int H, int W, float* __restrict__ out) {
  const long long total = (long long)D * H * W;
  const float scale = paste_scale(M, pad);
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const int d = (int)(i / ((long long)W * H));
    const PasteBox B = paste_box(boxes + 4 * (size_t)d, scale, H, W);
    out[i] = paste_value(masks + (size_t)d * M * M, M, pad, B, x, y);
  }
}

inline int grid_for(long long total) { return (int)min((long long)256 * 64, max((total + 255) / 256, 1ll)); }

}  // namespace

extern "C" {

int mi355det_mask_targets(const mi355det_mask_images* images, const float* rois, const int64_t* gt_index, int32_t num_rois, int32_t m,
                          float* out, void* stream) {
  if (!images || images->n_images < 1 || images->n_images > MI355DET_MASK_MAX_IMAGES || num_rois < 0 || m <= 0)
    return fail(MI355DET_EINVAL, "%s: bad arguments", "mask_targets");
  if (num_rois == 0) return MI355DET_OK;
  MaskImages I{};
  for (int b = 0; b < images->n_images; ++b) {
    if (images->h[b] <= 0 || images->w[b] <= 0) return fail(MI355DET_EINVAL, "%s: image %lld: bad mask size", "mask_targets", b);
    I.masks[b] = images->masks[b];
    I.h[b] = images->h[b];
    I.w[b] = images->w[b];
  }
  const long long total = (long long)num_rois * m * m;
  hipLaunchKernelGGL(mask_targets_kernel, dim3(grid_for(total)), dim3(256), 0, S(stream), I, images->n_images, rois, gt_index, num_rois, m, out);
  return check_launch("mask_targets");
}

size_t mi355det_mask_loss_workspace(int32_t rows) { return rows > 0 ? (size_t)rows * MASK_PART * sizeof(float) : 0; }

int mi355det_mask_loss(const void* feat, int32_t feat_ld, const float* w_logits, const float* b_logits, const int64_t* labels,
                       const float* targets, int32_t rows, int32_t valid, int32_t num_classes, float* loss, void* dfeat, float* dw,
                       float* db, float* dbias_deconv, void* workspace, size_t workspace_bytes, void* stream) {
  if (rows < 0 || valid < 0 || valid > rows || num_classes < 1 || feat_ld < 1024 || feat_ld % 4 || !loss)
    return fail(MI355DET_EINVAL, "%s: bad arguments", "mask_loss");
  if (rows > 0 && (!feat || !dfeat || !labels || !targets || !w_logits || !b_logits))
    return fail(MI355DET_EINVAL, "%s: missing operand", "mask_loss");
  if (workspace_bytes < mi355det_mask_loss_workspace(rows) || (rows > 0 && !workspace))
    return fail(MI355DET_EWORKSPACE, "%s: workspace too small", "mask_loss");
  const float inv_n = valid > 0 ? 1.0f / ((float)valid * 784.0f) : 0.f;
  if (rows > 0)
    hipLaunchKernelGGL(mask_loss_kernel<true>, dim3(rows), dim3(256), 0, S(stream), (const bf16_t*)feat, feat_ld, w_logits, b_logits, labels,
                       num_classes, valid, targets, inv_n, (bf16_t*)dfeat, (float*)workspace, nullptr);
  // valid == 0: the finish writes loss 0 and zero gradients (roi_heads.py:175-178: mask_logits.sum() * 0)
  hipLaunchKernelGGL(mask_loss_finish_kernel, dim3(num_classes + 2), dim3(256), 0, S(stream), (const float*)workspace, labels, valid, num_classes,
                     valid > 0 ? 1.0f / ((float)valid * 784.0f) : 0.f, loss, dw, db, dbias_deconv);
  return check_launch("mask_loss");
}

int mi355det_mask_probs(const void* feat, int32_t feat_ld, const float* w_logits, const float* b_logits, const int64_t* labels, int32_t rows,
                        int32_t num_classes, float* probs, void* stream) {
  if (rows < 0 || num_classes < 1 || feat_ld < 1024 || feat_ld % 4) return fail(MI355DET_EINVAL, "%s: bad arguments", "mask_probs");
  if (rows == 0) return MI355DET_OK;
  if (!feat || !w_logits || !b_logits || !labels || !probs) return fail(MI355DET_EINVAL, "%s: missing operand", "mask_probs");
  hipLaunchKernelGGL(mask_loss_kernel<false>, dim3(rows), dim3(256), 0, S(stream), (const bf16_t*)feat, feat_ld, w_logits, b_logits, labels,
                     num_classes, rows, nullptr, 0.f, nullptr, nullptr, probs);
  return check_launch("mask_probs");
}

int mi355det_mask_flip_resize_nearest(const uint8_t* in, int32_t planes, int32_t h, int32_t w, uint8_t* out, int32_t out_h, int32_t out_w,
                                      int32_t flip, void* stream) {
  if (planes < 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) return fail(MI355DET_EINVAL, "%s: bad arguments", "mask_resize_nearest");
  if (planes == 0) return MI355DET_OK;
  if (!in || !out) return fail(MI355DET_EINVAL, "%s: null masks", "mask_resize_nearest");
  const long long total = (long long)planes * out_h * out_w;
  hipLaunchKernelGGL(mask_resize_nearest_kernel, dim3(grid_for(total)), dim3(256), 0, S(stream), in, planes, h, w, out, out_h, out_w, flip);
  return check_launch("mask_resize_nearest");
}

int mi355det_mask_resize_nearest(const uint8_t* in, int32_t planes, int32_t h, int32_t w, uint8_t* out, int32_t out_h, int32_t out_w,
                                 void* stream) {
  return mi355det_mask_flip_resize_nearest(in, planes, h, w, out, out_h, out_w, 0, stream);
}

int mi355det_paste_masks(const float* masks, const float* boxes, int32_t num_masks, int32_t m, int32_t padding, int32_t im_h, int32_t im_w,
                         float* out, void* stream) {
  if (num_masks < 0 || m <= 0 || padding < 0 || im_h <= 0 || im_w <= 0) return fail(MI355DET_EINVAL, "%s: bad arguments", "paste_masks");
  if (num_masks == 0) return MI355DET_OK;
  const long long total = (long long)num_masks * im_h * im_w;
  hipLaunchKernelGGL(paste_masks_kernel, dim3(grid_for(total)), dim3(256), 0, S(stream), masks, boxes, num_masks, m, padding, im_h, im_w, out);
  return check_launch("paste_masks");
}

}  // extern "C"
