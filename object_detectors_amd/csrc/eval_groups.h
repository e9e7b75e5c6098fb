// The ragged (image, category) groups of the evaluation kernels (include/mi355det.h, "COCO evaluation"): the three offset arrays as the
// kernels of cocoeval_kernels.hip and oks_kernels.hip take them, a group's bounds-checked view and the host check of the entry points.
#pragma once
#include "common.h"

namespace mi355 {

struct Groups {
  const long long *dt_off, *gt_off, *iou_off;      // [NG + 1] each, on the device
  long long num_dt, num_gt, iou_size;              // the last offsets as the host knows them: a group that does not fit is skipped
};

struct GroupView {
  long long d0, g0, o;
  int D, G;
};

__device__ __forceinline__ bool group_view(const Groups& S, long long grp, GroupView& v) {
  v.d0 = S.dt_off[grp];
  v.g0 = S.gt_off[grp];
  v.o = S.iou_off[grp];
  const long long d1 = S.dt_off[grp + 1], g1 = S.gt_off[grp + 1];
  if (v.d0 < 0 || d1 < v.d0 || d1 > S.num_dt || v.g0 < 0 || g1 < v.g0 || g1 > S.num_gt || d1 - v.d0 > INT32_MAX || g1 - v.g0 > INT32_MAX)
    return false;
  v.D = (int)(d1 - v.d0);
  v.G = (int)(g1 - v.g0);
  return v.o >= 0 && v.o + (long long)v.D * v.G <= S.iou_size;
}

inline int check_groups(const char* what, long long num_groups, const void* dt_off, const void* gt_off, const void* iou_off, long long num_dt,
                        long long num_gt, long long iou_size) {
  if (num_groups < 0 || num_dt < 0 || num_gt < 0 || iou_size < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (num_groups >= (1ll << 31)) return fail(MI355DET_EINVAL, "%s: too many groups", what);
  if (num_groups > 0 && (!dt_off || !gt_off || !iou_off)) return fail(MI355DET_EINVAL, "%s: missing offsets", what);
  return MI355DET_OK;
}

}  // namespace mi355
