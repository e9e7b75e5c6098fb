// Object keypoint similarity on the device (include/mi355det.h, "COCO keypoint evaluation"): what pycocotools' COCOeval.computeOks computes
// with a Python double loop over detections x ground truths per image, for all (image, category) groups in one launch.  The output is the
// ragged buffer of coco_iou (cocoeval_kernels.hip), so keypoints_match and coco_accumulate take it from there.
//
//   coco_oks_kernel   wave = group.  The group's ground truths go through LDS a tile of OKS_TILE at a time: their 3K values are read by
//                     every detection lane, so they are staged once (coalesced) together with what computeOks derives per ground truth:
//                     k1 = the number of keypoints with v > 0, the doubled box x0, x1, y0, y1 and area + 2^-52.  Then lane = one
//                     (detection, ground truth of the tile) pair: it walks the K keypoints in ascending order and adds exp(-e) in that
//                     order, which makes the order part of the contract.  A detection's own 2K values come from global memory.
// float64, no atomics, one writer per element, no workspace.  Compiled with -ffp-contract=off: every product, sum and quotient of e is the one
// correctly rounded float64 operation of the definition; exp is the device library's float64 exp.
#include "eval_groups.h"

using namespace mi355;

namespace {

constexpr int OKS_MAX_K = 64;      // keypoints per instance
constexpr int OKS_TILE = 8;        // ground truths staged at a time: 8 * 3 * K * 8 B of dynamic LDS, 3.2 KiB at K = 17, 12 KiB at K = 64

struct GtMeta {
  double x0, x1, y0, y1, area_eps;
  int k1;
};

__global__ __launch_bounds__(WAVE) void coco_oks_kernel(Groups S, int K, const double* __restrict__ dt_kp, const double* __restrict__ gt_kp,
                                                        const double* __restrict__ gt_boxes, const double* __restrict__ gt_area,
                                                        const double* __restrict__ vars, double* __restrict__ oks) {
  extern __shared__ double s_kp[];                                        // [OKS_TILE, K, 3], sized by the launch
  __shared__ double s_var[OKS_MAX_K];
  __shared__ GtMeta s_meta[OKS_TILE];
  GroupView v;
  if (!group_view(S, blockIdx.x, v)) return;                              // uniform over the block: nobody waits at a barrier below
  if (v.D == 0 || v.G == 0) return;
  const int lane = threadIdx.x;
  if (lane < K) s_var[lane] = vars[lane];
  const double eps = 2.220446049250313e-16;                                // 2^-52, numpy's spacing(1)
  for (int gb = 0; gb < v.G; gb += OKS_TILE) {
    const int tg = min(OKS_TILE, v.G - gb);
    const double* src = gt_kp + (size_t)(v.g0 + gb) * 3 * K;              // the tile's ground truths are adjacent slots
    for (int i = lane; i < tg * 3 * K; i += WAVE) s_kp[i] = src[i];
    __syncthreads();
    if (lane < tg) {
      const double* kp = s_kp + lane * 3 * K;
      int k1 = 0;
      for (int i = 0; i < K; ++i) k1 += kp[3 * i + 2] > 0 ? 1 : 0;
      const double* bb = gt_boxes + 4 * (size_t)(v.g0 + gb + lane);
      GtMeta m;
      m.x0 = bb[0] - bb[2];
      m.x1 = bb[0] + bb[2] * 2;
      m.y0 = bb[1] - bb[3];
      m.y1 = bb[1] + bb[3] * 2;
      m.area_eps = gt_area[v.g0 + gb + lane] + eps;
      m.k1 = k1;
      s_meta[lane] = m;
    }
    __syncthreads();
    for (long long p = lane; p < (long long)v.D * tg; p += WAVE) {
      const int d = (int)(p / tg), gl = (int)(p % tg);
      const double* dk = dt_kp + (size_t)(v.d0 + d) * 2 * K;
      const double* gk = s_kp + gl * 3 * K;
      const GtMeta m = s_meta[gl];
      double sum = 0.0;
      for (int i = 0; i < K; ++i) {
        const double xd = dk[2 * i], yd = dk[2 * i + 1];
        double dx, dy;
        if (m.k1 > 0) {
          if (!(gk[3 * i + 2] > 0)) continue;                              // only the labelled keypoints count
          dx = xd - gk[3 * i];
          dy = yd - gk[3 * i + 1];
        } else {                                                           // no labelled keypoint: the distance to the doubled box
          dx = fmax(0.0, m.x0 - xd) + fmax(0.0, xd - m.x1);
          dy = fmax(0.0, m.y0 - yd) + fmax(0.0, yd - m.y1);
        }
        const double e = (dx * dx + dy * dy) / s_var[i] / m.area_eps / 2;
        sum += exp(-e);
      }
      oks[v.o + (long long)d * v.G + gb + gl] = sum / (double)(m.k1 > 0 ? m.k1 : K);
    }
    __syncthreads();                                                       // the next tile overwrites what these lanes read
  }
}

}  // namespace

extern "C" {

int mi355det_coco_oks(int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets, int64_t num_dt,
                      int64_t num_gt, int64_t iou_size, int32_t num_keypoints, const double* dt_kp, const double* gt_kp,
                      const double* gt_boxes, const double* gt_area, const double* vars, double* oks, void* stream) {
  const char* what = "coco_oks";
  const int st = check_groups(what, num_groups, dt_offsets, gt_offsets, iou_offsets, num_dt, num_gt, iou_size);
  if (st != MI355DET_OK) return st;
  if (num_keypoints < 1 || num_keypoints > OKS_MAX_K)
    return fail(MI355DET_EINVAL, "%s: %lld keypoints per instance, must be 1..%lld", what, num_keypoints, OKS_MAX_K);
  if (num_groups == 0) return MI355DET_OK;
  if (!vars || (num_dt > 0 && !dt_kp) || (num_gt > 0 && (!gt_kp || !gt_boxes || !gt_area)) || (iou_size > 0 && !oks))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if (iou_size == 0) return MI355DET_OK;
  const Groups G{(const long long*)dt_offsets, (const long long*)gt_offsets, (const long long*)iou_offsets, num_dt, num_gt, iou_size};
  const size_t lds = (size_t)OKS_TILE * 3 * num_keypoints * sizeof(double);
  hipLaunchKernelGGL(coco_oks_kernel, dim3((unsigned)num_groups), dim3(WAVE), lds, S(stream), G, (int)num_keypoints, dt_kp, gt_kp, gt_boxes,
                     gt_area, vars, oks);
  return check_launch(what);
}

}  // extern "C"
