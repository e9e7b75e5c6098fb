// Error breakdown of AP50 on the device (include/mi355det.h, "Error breakdown"): every false positive of an evaluated COCOEval / LVISEval is
// named Cls, Loc, Both, Dupe or Bkg by its best overlap with the counted ground truth of its own and of the other categories of its image,
// the ground truths nobody explains are Miss, and the flag arrays of the eight fixes are written in the layout mi355det_coco_accumulate reads.
//
//   tide_classify_kernel   block = one wavefront, grid-stride over images.  The image's counted ground truths go through LDS TIDE_CHUNK at a
//                          time (box, category, slot; compacted with a ballot, so the ascending slot order is kept); the 64 lanes stride over
//                          the image's detections in claim order, each false positive keeping its running (s, gs, o, go) over the chunks under
//                          strict >.  A batch of 64 detections without a false positive stages nothing.  `missed` is written as "counted and
//                          free" first; after a barrier the Loc and Cls lanes clear their partners' bytes (all of them store the same 0).
//   tide_fixes_kernel      the same walk.  A Loc / Cls detection with a free partner claims it unless an earlier detection of the image's
//                          claim order has the same kind and partner: the earlier keys go through LDS 64 at a time, so the winner depends on
//                          positions alone.  Every detection slot and every ground-truth slot is written by the one lane that owns it.
// float64 throughout, one division per overlapping pair, no atomics, 64-bit offsets.
// Compiled with -ffp-contract=off: the overlap has to be the bits mi355det_coco_iou writes for the same pair.
#include "common.h"

using namespace mi355;

namespace {

constexpr int TIDE_CHUNK = WAVE;          // ground truths staged at a time: one per lane
constexpr int TIDE_MAX_BLOCKS = 256 * 16;

enum : unsigned char { KIND_NONE = 0, KIND_CLS = 1, KIND_LOC = 2, KIND_BOTH = 3, KIND_DUPE = 4, KIND_BKG = 5 };
enum { ROW_BASE = 0, ROW_LOC = 1, ROW_BOTH = 2, ROW_DUPE = 3, ROW_BKG = 4, ROW_MISS = 5, ROW_FP = 6, ROW_FN = 7, NUM_ROWS = 8 };

// the image-major view of the category-major slots
struct ImageView {
  const long long* dt_off;       // [I + 1]
  const long long* dt_slot;      // [num_dt] detection slots, each image's in claim order
  long long num_dt;
  const long long* gt_off;       // [I + 1]
  const long long* gt_slot;      // [num_gt] ground-truth slots, each image's ascending
  long long num_gt;
};

struct Ranges {
  long long d0, d1, g0, g1;
};

// false: a range of this image does not fit, nothing of it may be read or written
__device__ __forceinline__ bool image_ranges(const ImageView& v, long long img, Ranges& r) {
  r.d0 = r.d1 = r.g0 = r.g1 = 0;
  if (v.num_dt > 0) {
    r.d0 = v.dt_off[img], r.d1 = v.dt_off[img + 1];
    if (r.d0 < 0 || r.d1 < r.d0 || r.d1 > v.num_dt) return false;
  }
  if (v.num_gt > 0) {
    r.g0 = v.gt_off[img], r.g1 = v.gt_off[img + 1];
    if (r.g0 < 0 || r.g1 < r.g0 || r.g1 > v.num_gt) return false;
  }
  return true;
}

__device__ __forceinline__ long long slot_at(const long long* slots, long long p, long long end, long long num) {
  if (p >= end) return -1;
  const long long s = slots[p];
  return (s < 0 || s >= num) ? -1 : s;
}

__global__ __launch_bounds__(WAVE) void tide_classify_kernel(ImageView v, long long num_images, const double* __restrict__ dt_box,
                                                             const int* __restrict__ dt_cat, const unsigned char* __restrict__ dt_fp,
                                                             const double* __restrict__ gt_box, const int* __restrict__ gt_cat,
                                                             const unsigned char* __restrict__ gt_counted,
                                                             const unsigned char* __restrict__ gt_free, double fg, double bg,
                                                             unsigned char* __restrict__ kind, long long* __restrict__ partner,
                                                             double* __restrict__ best_same, double* __restrict__ best_other,
                                                             unsigned char* missed) {
  __shared__ double s_box[TIDE_CHUNK][4];
  __shared__ long long s_slot[TIDE_CHUNK];
  __shared__ int s_cat[TIDE_CHUNK];
  const int lane = threadIdx.x;
  for (long long img = blockIdx.x; img < num_images; img += gridDim.x) {
    Ranges r;
    if (!image_ranges(v, img, r)) continue;
    for (long long q = r.g0 + lane; q < r.g1; q += WAVE) {
      const long long g = slot_at(v.gt_slot, q, r.g1, v.num_gt);
      if (g >= 0) missed[g] = (gt_counted[g] && gt_free[g]) ? 1 : 0;
    }
    __syncthreads();                                       // those bytes are in place before a partner's byte is cleared below
    for (long long p0 = r.d0; p0 < r.d1; p0 += WAVE) {
      const long long d = slot_at(v.dt_slot, p0 + lane, r.d1, v.num_dt);
      const bool fp = d >= 0 && dt_fp[d];
      double dx = 0, dy = 0, dw = 0, dh = 0;
      int dc = -1;
      if (fp) dx = dt_box[4 * d], dy = dt_box[4 * d + 1], dw = dt_box[4 * d + 2], dh = dt_box[4 * d + 3], dc = dt_cat[d];
      const double da = dw * dh, dx2 = dx + dw, dy2 = dy + dh;
      double s = 0.0, o = 0.0;
      long long gs = -1, go = -1;
      if (__ballot(fp)) {
        for (long long c0 = r.g0; c0 < r.g1; c0 += TIDE_CHUNK) {
          long long g = slot_at(v.gt_slot, c0 + lane, r.g1, v.num_gt);
          if (g >= 0 && !gt_counted[g]) g = -1;
          const unsigned long long m = __ballot(g >= 0);
          const int n = __popcll(m);
          __syncthreads();                                 // the previous chunk has been read
          if (g >= 0) {
            const int at = __popcll(m & ((1ull << lane) - 1));
            s_box[at][0] = gt_box[4 * g], s_box[at][1] = gt_box[4 * g + 1], s_box[at][2] = gt_box[4 * g + 2], s_box[at][3] = gt_box[4 * g + 3];
            s_slot[at] = g;
            s_cat[at] = gt_cat[g];
          }
          __syncthreads();
          if (fp) {
            for (int j = 0; j < n; ++j) {
              const double gx = s_box[j][0], gy = s_box[j][1], gw = s_box[j][2], gh = s_box[j][3];
              const double w = fmin(dx2, gx + gw) - fmax(dx, gx);
              if (w <= 0) continue;
              const double h = fmin(dy2, gy + gh) - fmax(dy, gy);
              if (h <= 0) continue;
              const double i = w * h;
              const double iou = i / (da + gw * gh - i);
              if (s_cat[j] == dc) {
                if (iou > s) s = iou, gs = s_slot[j];
              } else if (iou > o) {
                o = iou, go = s_slot[j];
              }
            }
          }
        }
      }
      if (d < 0) continue;
      unsigned char k = KIND_NONE;
      long long pa = -1;
      if (fp) {
        if (bg <= s && s < fg) k = KIND_LOC, pa = gs;
        else if (o >= fg) k = KIND_CLS, pa = go;
        else if (s >= fg) k = KIND_DUPE;
        else if (fmax(s, o) <= bg) k = KIND_BKG;
        else k = KIND_BOTH;
      }
      kind[d] = k;
      partner[d] = pa;
      best_same[d] = s;
      best_other[d] = o;
      if (pa >= 0) missed[pa] = 0;
    }
    __syncthreads();                                       // LDS and the image's bytes are settled before the next image
  }
}

__global__ __launch_bounds__(WAVE) void tide_fixes_kernel(ImageView v, long long num_images, const int* __restrict__ dt_match,
                                                          const unsigned char* __restrict__ dt_ignore, const int* __restrict__ dt_cat,
                                                          const int* __restrict__ gt_cat, const unsigned char* __restrict__ gt_counted,
                                                          const unsigned char* __restrict__ gt_free, const unsigned char* __restrict__ kind,
                                                          const long long* __restrict__ partner, const unsigned char* __restrict__ missed,
                                                          int* __restrict__ fix_dt_match, unsigned char* __restrict__ fix_dt_ignore,
                                                          unsigned char* __restrict__ fix_gt_ignore, int* __restrict__ cls_cat,
                                                          int* __restrict__ cls_match, unsigned char* __restrict__ cls_ignore) {
  __shared__ long long s_key[WAVE];
  const int lane = threadIdx.x;
  const size_t nd = (size_t)v.num_dt, ng = (size_t)v.num_gt;
  for (long long img = blockIdx.x; img < num_images; img += gridDim.x) {
    Ranges r;
    if (!image_ranges(v, img, r)) continue;
    for (long long q = r.g0 + lane; q < r.g1; q += WAVE) {
      const long long g = slot_at(v.gt_slot, q, r.g1, v.num_gt);
      if (g < 0) continue;
      const unsigned char off = gt_counted[g] ? 0 : 1, fr = (gt_counted[g] && gt_free[g]) ? 1 : 0;
#pragma unroll
      for (int row = 0; row < NUM_ROWS; ++row) fix_gt_ignore[row * ng + g] = off;
      if (fr && missed[g]) fix_gt_ignore[ROW_MISS * ng + g] = 1;
      if (fr) fix_gt_ignore[ROW_FN * ng + g] = 1;
    }
    for (long long p0 = r.d0; p0 < r.d1; p0 += WAVE) {
      const long long d = slot_at(v.dt_slot, p0 + lane, r.d1, v.num_dt);
      const unsigned char k = d >= 0 ? kind[d] : (unsigned char)KIND_NONE;
      const long long pa = (k == KIND_LOC || k == KIND_CLS) ? partner[d] : -1;
      const bool open = pa >= 0 && pa < v.num_gt && gt_counted[pa] && gt_free[pa];
      // the key of a claim: the partner and the walk it belongs to; -1 claims nothing
      const long long key = open ? pa * 2 + (k == KIND_CLS ? 1 : 0) : -1;
      bool wins = open;
      if (__ballot(open)) {
        for (long long c0 = r.d0; c0 <= p0; c0 += WAVE) {  // every earlier batch, then this one
          long long other = key;
          if (c0 != p0) {
            const long long e = slot_at(v.dt_slot, c0 + lane, r.d1, v.num_dt);
            const unsigned char ek = e >= 0 ? kind[e] : (unsigned char)KIND_NONE;
            const long long ep = (ek == KIND_LOC || ek == KIND_CLS) ? partner[e] : -1;
            other = (ep >= 0 && ep < v.num_gt && gt_counted[ep] && gt_free[ep]) ? ep * 2 + (ek == KIND_CLS ? 1 : 0) : -1;
          }
          __syncthreads();
          s_key[lane] = other;
          __syncthreads();
          const int n = c0 != p0 ? WAVE : lane;            // within the own batch only the lanes before this one are earlier
          if (open)
            for (int j = 0; j < n; ++j)
              if (s_key[j] == key) wins = false;
        }
      }
      if (d < 0) continue;
      const int m = dt_match[d];
      const unsigned char ig = dt_ignore[d];
#pragma unroll
      for (int row = 0; row < NUM_ROWS; ++row) {
        int rm = m;
        unsigned char ri = ig;
        if (row == ROW_LOC && k == KIND_LOC) rm = wins ? 1 : 0, ri = wins ? 0 : 1;
        if ((row == ROW_BOTH && k == KIND_BOTH) || (row == ROW_DUPE && k == KIND_DUPE) || (row == ROW_BKG && k == KIND_BKG) ||
            (row == ROW_FP && k != KIND_NONE))
          ri = 1;
        fix_dt_match[row * nd + d] = rm;
        fix_dt_ignore[row * nd + d] = ri;
      }
      const bool moved = k == KIND_CLS && wins;
      cls_cat[d] = moved ? gt_cat[pa] : dt_cat[d];
      cls_match[d] = k == KIND_CLS ? (wins ? 1 : 0) : m;
      cls_ignore[d] = k == KIND_CLS ? (wins ? 0 : 1) : ig;
    }
    __syncthreads();
  }
}

int check_view(const char* what, int64_t num_images, const int64_t* img_dt_offsets, const int64_t* img_dt_slots, int64_t num_dt,
               const int64_t* img_gt_offsets, const int64_t* img_gt_slots, int64_t num_gt) {
  if (num_images < 0 || num_dt < 0 || num_gt < 0) return fail(MI355DET_EINVAL, "%s: negative size", what);
  if (num_images > 0 && ((num_dt > 0 && (!img_dt_offsets || !img_dt_slots)) || (num_gt > 0 && (!img_gt_offsets || !img_gt_slots))))
    return fail(MI355DET_EINVAL, "%s: missing image view", what);
  return MI355DET_OK;
}

unsigned tide_grid(int64_t num_images) { return (unsigned)(num_images < TIDE_MAX_BLOCKS ? num_images : TIDE_MAX_BLOCKS); }

}  // namespace

extern "C" {

int mi355det_tide_classify(int64_t num_images, const int64_t* img_dt_offsets, const int64_t* img_dt_slots, int64_t num_dt,
                           const int64_t* img_gt_offsets, const int64_t* img_gt_slots, int64_t num_gt, const double* dt_boxes,
                           const int32_t* dt_cat, const uint8_t* dt_fp, const double* gt_boxes, const int32_t* gt_cat, const uint8_t* gt_counted,
                           const uint8_t* gt_free, double fg, double bg, uint8_t* kind, int64_t* partner, double* best_same, double* best_other,
                           uint8_t* missed, void* stream) {
  const char* what = "tide_classify";
  if (const int e = check_view(what, num_images, img_dt_offsets, img_dt_slots, num_dt, img_gt_offsets, img_gt_slots, num_gt)) return e;
  if (!(bg > 0 && bg <= 1 && fg > 0 && fg <= 1) || !(fg > bg)) return fail(MI355DET_EINVAL, "%s: the thresholds must lie in (0, 1] with fg > bg", what);
  if (num_images == 0 || (num_dt == 0 && num_gt == 0)) return MI355DET_OK;
  if (num_dt > 0 && (!dt_boxes || !dt_cat || !dt_fp || !kind || !partner || !best_same || !best_other))
    return fail(MI355DET_EINVAL, "%s: missing detection operand", what);
  if (num_gt > 0 && (!gt_boxes || !gt_cat || !gt_counted || !gt_free || !missed)) return fail(MI355DET_EINVAL, "%s: missing ground-truth operand", what);
  const ImageView v{(const long long*)img_dt_offsets, (const long long*)img_dt_slots, num_dt, (const long long*)img_gt_offsets,
                    (const long long*)img_gt_slots, num_gt};
  hipLaunchKernelGGL(tide_classify_kernel, dim3(tide_grid(num_images)), dim3(WAVE), 0, S(stream), v, (long long)num_images, dt_boxes, dt_cat,
                     dt_fp, gt_boxes, gt_cat, gt_counted, gt_free, fg, bg, kind, (long long*)partner, best_same, best_other, missed);
  return check_launch(what);
}

int mi355det_tide_fixes(int64_t num_images, const int64_t* img_dt_offsets, const int64_t* img_dt_slots, int64_t num_dt,
                        const int64_t* img_gt_offsets, const int64_t* img_gt_slots, int64_t num_gt, const int32_t* dt_match,
                        const uint8_t* dt_ignore, const int32_t* dt_cat, const int32_t* gt_cat, const uint8_t* gt_counted, const uint8_t* gt_free,
                        const uint8_t* kind, const int64_t* partner, const uint8_t* missed, int32_t* fix_dt_match, uint8_t* fix_dt_ignore,
                        uint8_t* fix_gt_ignore, int32_t* cls_cat, int32_t* cls_match, uint8_t* cls_ignore, void* stream) {
  const char* what = "tide_fixes";
  if (const int e = check_view(what, num_images, img_dt_offsets, img_dt_slots, num_dt, img_gt_offsets, img_gt_slots, num_gt)) return e;
  if (num_images == 0 || (num_dt == 0 && num_gt == 0)) return MI355DET_OK;
  if (num_dt > 0 && (!dt_match || !dt_ignore || !dt_cat || !kind || !partner || !fix_dt_match || !fix_dt_ignore || !cls_cat || !cls_match ||
                     !cls_ignore))
    return fail(MI355DET_EINVAL, "%s: missing detection operand", what);
  if (num_gt > 0 && (!gt_cat || !gt_counted || !gt_free || !missed || !fix_gt_ignore)) return fail(MI355DET_EINVAL, "%s: missing ground-truth operand", what);
  const ImageView v{(const long long*)img_dt_offsets, (const long long*)img_dt_slots, num_dt, (const long long*)img_gt_offsets,
                    (const long long*)img_gt_slots, num_gt};
  hipLaunchKernelGGL(tide_fixes_kernel, dim3(tide_grid(num_images)), dim3(WAVE), 0, S(stream), v, (long long)num_images, dt_match, dt_ignore,
                     dt_cat, gt_cat, gt_counted, gt_free, kind, (const long long*)partner, missed, fix_dt_match, fix_dt_ignore, fix_gt_ignore,
                     cls_cat, cls_match, cls_ignore);
  return check_launch(what);
}

}  // extern "C"
