// The torchvision box rules on xyxy float4 boxes, each stated once: box_iou, the Matcher's per-column step and verdict, BoxCoder encode /
// decode, clip_boxes_to_image, the side test of remove_small_boxes.  Used by box_kernels.hip and proposal_kernels.hip, which are built with
// -ffp-contract=off: the operation order written here is the reference's unfused float32 order, and every kernel that shares a function
// gives the same bits.  (nms_iou of box_kernels.hip and the xcycwh IoU family of yolo_kernels.hip are other rules and stay where they are.)
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

// torchvision box_iou (ops/boxes.py): a = ground truth, b = anchor / candidate in the matchers
__device__ __forceinline__ float box_iou(const float4 a, const float4 b) {
  const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
  const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.0f), h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.0f);
  const float inter = w * h;
  return inter / (area_a + area_b - inter);
}

// Matcher (tvision/_utils.py:271-344).  One step of the maximum over the ground-truth boxes q = 0, 1, ...: the first maximum wins, as
// torch.max(dim=0) ...
__device__ __forceinline__ void matcher_argmax(float v, int q, float& best, int& arg) {
  if (q == 0 || v > best) {
    best = v;
    arg = q;
  }
}

// ... and what the maximum becomes: BELOW_LOW_THRESHOLD = -1, BETWEEN_THRESHOLDS = -2, else the index
__device__ __forceinline__ int match_verdict(float best, int arg, float lo, float hi) { return best < lo ? -1 : (best < hi ? -2 : arg); }

// BoxCoder.encode_single (tvision/_utils.py:79-125): the code of `reference` (the matched ground truth) relative to `proposal`
__device__ __forceinline__ float4 box_encode(const float4 proposal, const float4 reference, float wx, float wy, float ww, float wh) {
  const float ew = proposal.z - proposal.x, eh = proposal.w - proposal.y, ecx = proposal.x + 0.5f * ew, ecy = proposal.y + 0.5f * eh;
  const float gw = reference.z - reference.x, gh = reference.w - reference.y, gcx = reference.x + 0.5f * gw, gcy = reference.y + 0.5f * gh;
  return make_float4(wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * logf(gw / ew), wh * logf(gh / eh));
}

// BoxCoder.decode_single (tvision/_utils.py:190-232): divide by the weights, clamp dw / dh at `clip`, exp, centre -+ half size.  With
// weights that are the constant 1.0f the divisions fold away (x / 1.0f == x): the RPN and RetinaNet coders.
__device__ __forceinline__ float4 box_decode(const float4 code, const float4 box, float wx, float wy, float ww, float wh, float clip) {
  const float w = box.z - box.x, h = box.w - box.y, cx = box.x + 0.5f * w, cy = box.y + 0.5f * h;
  const float dx = code.x / wx, dy = code.y / wy, dw = fminf(code.z / ww, clip), dh = fminf(code.w / wh, clip);
  const float pcx = dx * w + cx, pcy = dy * h + cy, pw = expf(dw) * w, ph = expf(dh) * h;
  return make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw, pcy + 0.5f * ph);
}

// clip_boxes_to_image (ops/boxes.py) against lim = (w, h, w, h)
__device__ __forceinline__ float4 box_clip(const float4 b, const float4 lim) {
  return make_float4(fminf(fmaxf(b.x, 0.f), lim.x), fminf(fmaxf(b.y, 0.f), lim.y), fminf(fmaxf(b.z, 0.f), lim.z), fminf(fmaxf(b.w, 0.f), lim.w));
}

// remove_small_boxes (ops/boxes.py): both sides at least min_size
__device__ __forceinline__ bool box_min_side(const float4 b, float min_size) { return (b.z - b.x >= min_size) && (b.w - b.y >= min_size); }

}  // namespace mi355
