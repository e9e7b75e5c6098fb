// Model comparison on the device (include/mi355det.h, "Model comparison"): for two result sets, the best class-agnostic box overlap of every
// ground-truth instance and whether that detection carries the right label - the per-image body of the reference's
// notebooks/get_disagreement.py:62-100 (torchvision box_iou, then max over the detections) for all images and both models in one launch.
//
//   box_disagreement_kernel  block = (image, model), BD_WAVES wavefronts.  The wavefronts take the image's ground truths in turn; the 64 lanes
//                            stride over the image's detections, each keeping its own (value, index) under the arg-max order of torch.max
//                            (NaN beats every number; among equals, or among NaNs, the lowest index wins); a butterfly under the same order
//                            leaves the winner in every lane and lane 0 writes the ground truth's three outputs.
// float64 throughout, no atomics, one writer per output element, 64-bit offsets, no cap on either count of an image short of
// best_index being int32.
// Compiled with -ffp-contract=off: the sums, the products and the quotient have to be the correctly rounded float64 operations of the rule.
#include "wave_ops.h"

using namespace mi355;

namespace {

constexpr int BD_WAVES = 4;

struct Best {
  double v;
  long long i;        // index within the image's detections; -1: nothing seen yet (loses to everything)
};

// does b take over from a?  A total order: any two lanes agree on the winner, whichever way the butterfly pairs them.
__device__ __forceinline__ bool takes_over(const Best& a, const Best& b) {
  if (b.i < 0) return false;
  if (a.i < 0) return true;
  const bool an = a.v != a.v, bn = b.v != b.v;
  if (an || bn) return bn && (!an || b.i < a.i);
  return b.v > a.v || (b.v == a.v && b.i < a.i);
}

struct DtSide {
  const long long* off;      // [I + 1] on the device
  const double* box;         // [num, 4] as [x, y, w, h]
  const long long* label;    // [num]
  long long num;             // the host's copy of off[I]: an image whose range does not fit is treated as having no detections
};

struct DtSides {
  DtSide m[2];
};

// clamp(min = 0) as ATen computes it: a NaN stays a NaN
__device__ __forceinline__ double clamp0(double x) { return x < 0 ? 0.0 : x; }

__global__ __launch_bounds__(BD_WAVES* WAVE) void box_disagreement_kernel(const long long* __restrict__ gt_off, long long num_gt,
                                                                          const double* __restrict__ gt_box,
                                                                          const long long* __restrict__ gt_label, DtSides sides, double thr,
                                                                          double* __restrict__ best_iou, int* __restrict__ best_index,
                                                                          unsigned char* __restrict__ correct) {
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, model = blockIdx.y;
  const long long img = blockIdx.x;
  const long long g0 = gt_off[img], g1 = gt_off[img + 1];
  if (g0 < 0 || g1 < g0 || g1 > num_gt) return;                        // nothing of this image can be written safely
  const DtSide& side = sides.m[model];
  long long d0 = side.off[img], d1 = side.off[img + 1];
  if (d0 < 0 || d1 < d0 || d1 > side.num || d1 - d0 > INT32_MAX) d0 = d1 = 0;
  const long long D = d1 - d0;
  const size_t out = (size_t)model * (size_t)num_gt;
  if (D == 0) {                                                        // reads no box and no label
    for (long long g = g0 + threadIdx.x; g < g1; g += BD_WAVES * WAVE) {
      best_iou[out + g] = 0.0;
      best_index[out + g] = -1;
      correct[out + g] = 0;
    }
    return;
  }
  const double* db = side.box + 4 * d0;
  for (long long g = g0 + wave; g < g1; g += BD_WAVES) {
    const double gx = gt_box[4 * g], gy = gt_box[4 * g + 1];
    const double gx2 = gx + gt_box[4 * g + 2], gy2 = gy + gt_box[4 * g + 3];
    const double ga = (gx2 - gx) * (gy2 - gy);
    Best b{0.0, -1};
    for (long long d = lane; d < D; d += WAVE) {
      const double dx = db[4 * d], dy = db[4 * d + 1];
      const double dx2 = dx + db[4 * d + 2], dy2 = dy + db[4 * d + 3];
      const double da = (dx2 - dx) * (dy2 - dy);
      const double iw = clamp0(fmin(dx2, gx2) - fmax(dx, gx)), ih = clamp0(fmin(dy2, gy2) - fmax(dy, gy));
      const double inter = iw * ih;
      const Best c{inter / (da + ga - inter), d};
      if (takes_over(b, c)) b = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const Best c{__shfl_xor(b.v, o, WAVE), shfl_xor_i64(b.i, o)};
      if (takes_over(b, c)) b = c;
    }
    if (lane == 0) {                                                   // D >= 1: lane 0 saw detection 0, so b.i >= 0
      best_iou[out + g] = b.v;
      best_index[out + g] = (int)b.i;
      correct[out + g] = (b.v >= thr && gt_label[g] == side.label[d0 + b.i]) ? 1 : 0;
    }
  }
}

}  // namespace

extern "C" {

int mi355det_box_disagreement(int64_t num_images, const int64_t* gt_offsets, int64_t num_gt, const double* gt_box, const int64_t* gt_label,
                              const int64_t* dt_offsets_a, int64_t num_dt_a, const double* dt_box_a, const int64_t* dt_label_a,
                              const int64_t* dt_offsets_b, int64_t num_dt_b, const double* dt_box_b, const int64_t* dt_label_b,
                              double iou_threshold, double* best_iou, int32_t* best_index, uint8_t* correct, void* stream) {
  const char* what = "box_disagreement";
  if (num_images < 0 || num_gt < 0 || num_dt_a < 0 || num_dt_b < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (num_images >= (1ll << 31)) return fail(MI355DET_EINVAL, "%s: too many images", what);
  if (num_images > 0 && (!gt_offsets || !dt_offsets_a || !dt_offsets_b)) return fail(MI355DET_EINVAL, "%s: missing offsets", what);
  if (num_images == 0 || num_gt == 0) return MI355DET_OK;
  if (!gt_box || !gt_label || !best_iou || !best_index || !correct) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if ((num_dt_a > 0 && (!dt_box_a || !dt_label_a)) || (num_dt_b > 0 && (!dt_box_b || !dt_label_b)))
    return fail(MI355DET_EINVAL, "%s: missing detections", what);
  DtSides sides;
  sides.m[0] = DtSide{(const long long*)dt_offsets_a, dt_box_a, (const long long*)dt_label_a, num_dt_a};
  sides.m[1] = DtSide{(const long long*)dt_offsets_b, dt_box_b, (const long long*)dt_label_b, num_dt_b};
  hipLaunchKernelGGL(box_disagreement_kernel, dim3((unsigned)num_images, 2), dim3(BD_WAVES * WAVE), 0, S(stream),
                     (const long long*)gt_offsets, (long long)num_gt, gt_box, (const long long*)gt_label, sides, iou_threshold, best_iou,
                     best_index, correct);
  return check_launch(what);
}

}  // extern "C"
