// COCO evaluation on the device (include/mi355det.h, "COCO evaluation"): what pycocotools' maskUtils.iou, COCOeval.evaluateImg and
// COCOeval.accumulate compute, for the tens of thousands of small independent (image, category) groups of a validation run.
//
// A group is one (image, category) pair: D detections in descending score order (cut to the largest maxDets by the caller) and G ground
// truths in annotation order.  Three passes, all float64, no atomics, every output element written by exactly one lane:
//   coco_iou_kernel         wave = group, lane = (d, g) pair: the [D, G] IoU matrix into one ragged buffer.  Box mode and run-length mode
//                           share iou_tail(); in run-length mode the tight boxes reject first and the lane then walks both count lists.
//   coco_match_kernel       wave = group, lane a*T + t = one (area range, IoU threshold): the sequential greedy match.  The ground truths are
//                           walked non-ignored first, ignored second, each in annotation order - the stable partition by the ignore flag,
//                           never stored.  The "already matched" state is gt_match itself.
//                           One body, two rules (template switch): COCO re-matches a taken crowd; LVIS (lvis-api's LVISEval) has no
//                           crowds, takes the annotation's ignore flag in their place and ignores an unmatched detection of a group whose
//                           category is not exhaustively annotated in its image.  A second switch keeps the two COCO flags apart for
//                           `keypoints`: the ignore flag (iscrowd or num_keypoints == 0) ignores, iscrowd alone re-matches.
//   coco_accumulate_kernel  wave = (category, area range, maxDets, threshold): a forward walk over the category's detections in score order
//                           for the totals, then a backward walk that rebuilds the cumulative sums from the totals (integers: exact), carries
//                           the running maximum of the precision and lets every detection that raises the recall write the recall thresholds
//                           it is the first to reach.  No workspace.
// Compiled with -ffp-contract=off: every quotient and product has to be the one correctly rounded float64 operation of the definition.
#include "eval_groups.h"
#include "wave_ops.h"

using namespace mi355;

namespace {

// i = intersection, da / ga = the two areas: i / (crowd ? da : da + ga - i)
__device__ __forceinline__ double iou_tail(double i, double da, double ga, bool crowd) {
  const double u = crowd ? da : da + ga - i;
  return i / u;
}

// [x, y, w, h] against [x, y, w, h]
__device__ __forceinline__ double box_iou(const double* __restrict__ d, const double* __restrict__ g, bool crowd) {
  const double da = d[2] * d[3], ga = g[2] * g[3];
  const double w = fmin(d[0] + d[2], g[0] + g[2]) - fmax(d[0], g[0]);
  if (w <= 0) return 0.0;
  const double h = fmin(d[1] + d[3], g[1] + g[3]) - fmax(d[1], g[1]);
  if (h <= 0) return 0.0;
  return iou_tail(w * h, da, ga, crowd);
}

// two run lists of one [H, W] (alternating runs of 0 and 1, a zero run first): set pixels of both, of a, of b.  Every step ends a run of at
// least one list, so the walk is bounded by the number of counts whatever they hold.
__device__ __forceinline__ void rle_overlap(const int* __restrict__ ca, long long a0, long long a1, const int* __restrict__ cb, long long b0,
                                            long long b1, long long& inter, long long& na, long long& nb) {
  inter = na = nb = 0;
  if (a0 >= a1 || b0 >= b1) return;
  long long ka = a0, kb = b0;
  long long ra = ca[ka], rb = cb[kb];
  bool va = false, vb = false;
  while (true) {
    const long long c = ra < rb ? ra : rb;
    if (va) na += c;
    if (vb) nb += c;
    if (va && vb) inter += c;
    ra -= c;
    rb -= c;
    if (ra == 0) {
      if (++ka >= a1) break;
      ra = ca[ka];
      va = !va;
    }
    if (rb == 0) {
      if (++kb >= b1) break;
      rb = cb[kb];
      vb = !vb;
    }
  }
}

struct RleSide {
  const int* counts;             // the masks' counts one after the other
  const long long* runs;         // [num_masks + 1]: mask k owns counts[runs[k]:runs[k + 1]]
  const long long* index;        // slot -> mask, or NULL for the identity
  long long num_masks, num_counts;
  __device__ __forceinline__ bool range(long long slot, long long& lo, long long& hi) const {
    const long long k = index ? index[slot] : slot;
    if (k < 0 || k >= num_masks) return false;
    lo = runs[k];
    hi = runs[k + 1];
    return lo >= 0 && hi >= lo && hi <= num_counts;
  }
};

template <bool RLE>
__global__ __launch_bounds__(WAVE) void coco_iou_kernel(Groups S, const double* __restrict__ dt_boxes, const double* __restrict__ gt_boxes,
                                                        const unsigned char* __restrict__ gt_crowd, RleSide A, RleSide B,
                                                        double* __restrict__ iou) {
  GroupView v;
  if (!group_view(S, blockIdx.x, v)) return;
  const long long pairs = (long long)v.D * v.G;
  for (long long p = threadIdx.x; p < pairs; p += WAVE) {
    const long long d = v.d0 + p / v.G, g = v.g0 + p % v.G;
    const bool crowd = gt_crowd[g] != 0;
    double r = box_iou(dt_boxes + 4 * d, gt_boxes + 4 * g, crowd);       // run-length mode: the tight boxes
    if (RLE && r != 0.0) {
      long long a0, a1, b0, b1, inter = 0, na = 0, nb = 0;
      if (A.range(d, a0, a1) && B.range(g, b0, b1)) rle_overlap(A.counts, a0, a1, B.counts, b0, b1, inter, na, nb);
      r = inter == 0 ? 0.0 : iou_tail((double)inter, (double)na, (double)nb, crowd);
    }
    iou[v.o + p] = r;
  }
}

// gt_ignore [A, num_gt]; dt_match / dt_ignore [A, T, num_dt]; gt_match [A, T, num_gt] (zeroed by the entry point).  gt_flag [num_gt]: COCO's
// iscrowd, or (LVIS) the annotation's ignore flag; group_nel [num_groups], read by the LVIS variant only: the group's category is not
// exhaustively annotated in its image.  gt_crowd [num_gt], read by the SPLIT variant only (keypoints): the flag that lets a taken ground
// truth match again, where gt_flag only ignores; without SPLIT gt_flag is both.
template <bool LVIS, bool SPLIT>
__global__ __launch_bounds__(WAVE) void coco_match_kernel(Groups S, const double* __restrict__ iou, const double* __restrict__ dt_area,
                                                          const double* __restrict__ gt_area, const unsigned char* __restrict__ gt_flag,
                                                          const unsigned char* __restrict__ gt_crowd,
                                                          const unsigned char* __restrict__ group_nel, const double* __restrict__ iou_thrs, int T,
                                                          const double* __restrict__ area_rngs, int A, int* __restrict__ dt_match,
                                                          unsigned char* __restrict__ dt_ignore, int* __restrict__ gt_match,
                                                          unsigned char* __restrict__ gt_ignore) {
  GroupView v;
  if (!group_view(S, blockIdx.x, v)) return;                              // uniform over the block: nobody waits at the barrier below
  const int lane = threadIdx.x;
  const bool nel = LVIS && group_nel[blockIdx.x] != 0;                    // one value per block
  for (long long e = lane; e < (long long)A * v.G; e += WAVE) {
    const int a = (int)(e / v.G);
    const long long g = v.g0 + e % v.G;
    const double ar = gt_area[g];
    gt_ignore[(size_t)a * S.num_gt + g] = (gt_flag[g] != 0 || ar < area_rngs[2 * a] || ar > area_rngs[2 * a + 1]) ? 1 : 0;
  }
  __syncthreads();
  if (lane >= A * T) return;
  const int a = lane / T, t = lane % T;
  const double lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
  const double thr = fmin(iou_thrs[t], 1 - 1e-10);
  const unsigned char* gi = gt_ignore + (size_t)a * S.num_gt + v.g0;
  const unsigned char* gc = (SPLIT ? gt_crowd : gt_flag) + v.g0;
  int* gm = gt_match + ((size_t)a * T + t) * S.num_gt + v.g0;
  int* dm = dt_match + ((size_t)a * T + t) * S.num_dt + v.d0;
  unsigned char* di = dt_ignore + ((size_t)a * T + t) * S.num_dt + v.d0;
  for (int d = 0; d < v.D; ++d) {
    const double* row = iou + v.o + (long long)d * v.G;
    double best = thr;
    int m = -1;
    for (int phase = 0; phase < 2; ++phase) {          // non-ignored ground truths, then ignored ones
      if (phase == 1 && m > -1) break;                 // a non-ignored match stands: the walk stops at the first ignored ground truth
      for (int g = 0; g < v.G; ++g) {
        if (gi[g] != phase) continue;
        if (gm[g] > 0 && (LVIS || !gc[g])) continue;   // taken at this threshold, and no crowd (LVIS: taken is taken)
        const double x = row[g];
        if (x < best) continue;                        // strict: an IoU equal to the threshold matches, an equal later one takes over
        best = x;
        m = g;
      }
    }
    unsigned char ig = 0;
    if (m > -1) {
      dm[d] = m + 1;
      gm[m] = d + 1;
      ig = gi[m];
    } else {
      const double ar = dt_area[v.d0 + d];
      ig = (ar < lo || ar > hi || nel) ? 1 : 0;
    }
    di[d] = ig;
  }
}

struct MaxDets {
  int v[8];
};

struct AccFlags {
  long long idx;
  int tp, fp, valid;
};

// block = one wave = (k, a, m, t).  order [num_dt]: per category the detection slots in descending score order (stable); the first-m-of-
// each-group subset in that order is the stable sort of the subset, so rank < max_dets[m] filters it.
__global__ __launch_bounds__(WAVE) void coco_accumulate_kernel(int K, const long long* __restrict__ cat_dt_off, const long long* __restrict__ cat_gt_off,
                                                               long long num_dt, long long num_gt, const long long* __restrict__ order,
                                                               const int* __restrict__ dt_rank, const double* __restrict__ dt_score,
                                                               const int* __restrict__ dt_match, const unsigned char* __restrict__ dt_ignore,
                                                               const unsigned char* __restrict__ gt_ignore, int T, int A, MaxDets MD, int M,
                                                               const double* __restrict__ rec_thrs, int R, double* __restrict__ precision,
                                                               double* __restrict__ recall, double* __restrict__ scores) {
  extern __shared__ double s_thr[];
  const int lane = threadIdx.x;
  long long b = blockIdx.x;
  const int t = (int)(b % T);
  b /= T;
  const int m = (int)(b % M);
  b /= M;
  const int a = (int)(b % A);
  const int k = (int)(b / A);
  for (int r = lane; r < R; r += WAVE) s_thr[r] = rec_thrs[r];
  __syncthreads();
  long long c0 = cat_dt_off[k], c1 = cat_dt_off[k + 1], g0 = cat_gt_off[k], g1 = cat_gt_off[k + 1];
  if (c0 < 0 || c1 < c0 || c1 > num_dt) c0 = c1 = 0;
  if (g0 < 0 || g1 < g0 || g1 > num_gt) g0 = g1 = 0;
  const long long N = c1 - c0;
  const int maxdet = MD.v[m];
  const int* dm = dt_match + ((size_t)a * T + t) * num_dt;
  const unsigned char* di = dt_ignore + ((size_t)a * T + t) * num_dt;
  const size_t out_r = (((size_t)t * K + k) * A + a) * M + m;                                   // recall [T, K, A, M]
  auto out_p = [&](int r) { return ((((size_t)t * R + r) * K + k) * A + a) * M + m; };          // precision, scores [T, R, K, A, M]

  long long npig = 0;
  for (long long g = g0 + lane; g < g1; g += WAVE) npig += gt_ignore[(size_t)a * num_gt + g] ? 0 : 1;
  npig = wave_sum_i64(npig);
  if (npig == 0) {
    for (int r = lane; r < R; r += WAVE) precision[out_p(r)] = scores[out_p(r)] = -1.0;
    if (lane == 0) recall[out_r] = -1.0;
    return;
  }
  auto flags = [&](long long p) {
    AccFlags f{-1, 0, 0, 0};
    if (p < N) {
      const long long idx = order[c0 + p];
      if (idx >= 0 && idx < num_dt && dt_rank[idx] < maxdet) {
        const bool matched = dm[idx] != 0, ign = di[idx] != 0;
        f.idx = idx;
        f.valid = 1;
        f.tp = matched && !ign;
        f.fp = !matched && !ign;
      }
    }
    return f;
  };
  // forward: the totals
  long long tot_tp = 0, tot_fp = 0, tot_nd = 0;
  for (long long p = lane; p < N; p += WAVE) {
    const AccFlags f = flags(p);
    tot_tp += f.tp;
    tot_fp += f.fp;
    tot_nd += f.valid;
  }
  tot_tp = wave_sum_i64(tot_tp);
  tot_fp = wave_sum_i64(tot_fp);
  tot_nd = wave_sum_i64(tot_nd);
  const double dn = (double)npig;
  // the number of recall thresholds <= x: the detection whose recall reaches x is the first index for all of them not reached before
  auto reached = [&](double x) {
    int lo = 0, hi = R;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_thr[mid] <= x) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const int r_end = tot_nd > 0 ? reached((double)tot_tp / dn) : 0;
  for (int r = r_end + lane; r < R; r += WAVE) precision[out_p(r)] = scores[out_p(r)] = 0.0;
  if (lane == 0) recall[out_r] = tot_nd > 0 ? (double)tot_tp / dn : 0.0;
  // backward: cumulative sums rebuilt from the totals, the running maximum of the precision carried from the right
  long long end_tp = tot_tp, end_fp = tot_fp, end_nd = tot_nd;
  double carry = -1.0;
  const double eps = 2.220446049250313e-16;            // 2^-52, numpy's spacing(1)
  for (long long base = ((N - 1) / WAVE) * WAVE; N > 0 && base >= 0; base -= WAVE) {
    const AccFlags f = flags(base + lane);
    const int itp = wave_scan_incl(f.tp, lane), ifp = wave_scan_incl(f.fp, lane), ind = wave_scan_incl(f.valid, lane);
    const long long start_tp = end_tp - __shfl(itp, WAVE - 1, WAVE), start_fp = end_fp - __shfl(ifp, WAVE - 1, WAVE),
                    start_nd = end_nd - __shfl(ind, WAVE - 1, WAVE);
    const long long tps = start_tp + itp, fps = start_fp + ifp, nds = start_nd + ind;
    double pr = f.valid ? (double)tps / ((double)fps + (double)tps + eps) : -1.0;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      const double y = __shfl_down(pr, o, WAVE);
      if (lane + o < WAVE) pr = fmax(pr, y);
    }
    pr = fmax(pr, carry);
    carry = __shfl(pr, 0, WAVE);
    if (f.valid && (f.tp || nds == 1)) {
      const int r0 = nds == 1 ? 0 : reached((double)(tps - 1) / dn), r1 = reached((double)tps / dn);
      const double sc = dt_score[f.idx];
      for (int r = r0; r < r1; ++r) {
        precision[out_p(r)] = pr;
        scores[out_p(r)] = sc;
      }
    }
    end_tp = start_tp;
    end_fp = start_fp;
    end_nd = start_nd;
  }
}

// the three match entry points: `lvis` picks the rule, `group_nel` is read by the LVIS rule only; `split`: gt_crowd is its own array
int match_entry(const char* what, bool lvis, bool split, int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets,
                int64_t num_dt, int64_t num_gt, int64_t iou_size, const double* iou, const double* dt_area, const double* gt_area,
                const uint8_t* gt_flag, const uint8_t* gt_crowd, const uint8_t* group_nel, const double* iou_thrs, int32_t num_thrs,
                const double* area_rngs, int32_t num_areas, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, void* stream) {
  const int st = check_groups(what, num_groups, dt_offsets, gt_offsets, iou_offsets, num_dt, num_gt, iou_size);
  if (st != MI355DET_OK) return st;
  if (num_thrs <= 0 || num_areas <= 0 || (long long)num_thrs * num_areas > WAVE)
    return fail(MI355DET_EINVAL, "%s: thresholds x area ranges = %lld must be 1..64 (one lane each)", what, (long long)num_thrs * num_areas);
  if (num_groups == 0) return MI355DET_OK;
  if (!iou_thrs || !area_rngs) return fail(MI355DET_EINVAL, "%s: missing parameters", what);
  if (lvis && !group_nel) return fail(MI355DET_EINVAL, "%s: missing group_not_exhaustive", what);
  if ((num_dt > 0 && (!dt_area || !dt_match || !dt_ignore)) || (num_gt > 0 && (!gt_area || !gt_flag || (split && !gt_crowd) || !gt_match || !gt_ignore)) ||
      (iou_size > 0 && !iou))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  const size_t cells = (size_t)num_thrs * num_areas;
  if (num_dt > 0 && hipMemsetAsync(dt_match, 0, cells * num_dt * sizeof(int32_t), S(stream)) != hipSuccess) return check_launch(what);
  if (num_gt > 0 && hipMemsetAsync(gt_match, 0, cells * num_gt * sizeof(int32_t), S(stream)) != hipSuccess) return check_launch(what);
  const Groups G{(const long long*)dt_offsets, (const long long*)gt_offsets, (const long long*)iou_offsets, num_dt, num_gt, iou_size};
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)num_groups), dim3(WAVE), 0, S(stream), G, iou, dt_area, gt_area, gt_flag, gt_crowd, group_nel, iou_thrs,
                       num_thrs, area_rngs, num_areas, dt_match, dt_ignore, gt_match, gt_ignore);
  };
  if (lvis) launch(coco_match_kernel<true, false>);
  else if (split) launch(coco_match_kernel<false, true>);
  else launch(coco_match_kernel<false, false>);
  return check_launch(what);
}

}  // namespace

extern "C" {

int mi355det_coco_iou(int32_t rle_mode, int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets,
                      int64_t num_dt, int64_t num_gt, int64_t iou_size, const double* dt_boxes, const double* gt_boxes, const uint8_t* gt_crowd,
                      const int32_t* dt_counts, const int64_t* dt_runs, const int64_t* dt_index, int64_t dt_masks, int64_t dt_num_counts,
                      const int32_t* gt_counts, const int64_t* gt_runs, const int64_t* gt_index, int64_t gt_masks, int64_t gt_num_counts,
                      const int32_t* dt_sizes, const int32_t* gt_sizes, double* iou, void* stream) {
  const char* what = "coco_iou";
  const int st = check_groups(what, num_groups, dt_offsets, gt_offsets, iou_offsets, num_dt, num_gt, iou_size);
  if (st != MI355DET_OK) return st;
  if (rle_mode != 0 && rle_mode != 1) return fail(MI355DET_EINVAL, "%s: rle_mode must be 0 or 1", what);
  if (rle_mode) {
    if (dt_masks < 0 || gt_masks < 0 || dt_num_counts < 0 || gt_num_counts < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
    if (num_groups > 0 && (!dt_sizes || !gt_sizes)) return fail(MI355DET_EINVAL, "%s: run-length mode needs the groups' mask sizes", what);
    for (int64_t g = 0; g < num_groups; ++g) {         // [h, w] per group and side, [0, 0] for a side without masks
      const int32_t *a = dt_sizes + 2 * g, *b = gt_sizes + 2 * g;
      if (a[0] < 0 || a[1] < 0 || b[0] < 0 || b[1] < 0) return fail(MI355DET_EINVAL, "%s: negative mask size in group %lld", what, g);
      const bool has_a = a[0] || a[1], has_b = b[0] || b[1];
      if (has_a && has_b && (a[0] != b[0] || a[1] != b[1]))
        return fail(MI355DET_EINVAL, "%s: the masks of group %lld differ in size", what, g);
    }
  }
  if (num_groups == 0 || iou_size == 0) return MI355DET_OK;
  if (!dt_boxes || !gt_boxes || !gt_crowd || !iou) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if (rle_mode && (!dt_counts || !dt_runs || !gt_counts || !gt_runs)) return fail(MI355DET_EINVAL, "%s: missing run lengths", what);
  const Groups G{(const long long*)dt_offsets, (const long long*)gt_offsets, (const long long*)iou_offsets, num_dt, num_gt, iou_size};
  const RleSide A{dt_counts, (const long long*)dt_runs, (const long long*)dt_index, dt_masks, dt_num_counts};
  const RleSide B{gt_counts, (const long long*)gt_runs, (const long long*)gt_index, gt_masks, gt_num_counts};
  if (rle_mode)
    hipLaunchKernelGGL(coco_iou_kernel<true>, dim3((unsigned)num_groups), dim3(WAVE), 0, S(stream), G, dt_boxes, gt_boxes, gt_crowd, A, B, iou);
  else
    hipLaunchKernelGGL(coco_iou_kernel<false>, dim3((unsigned)num_groups), dim3(WAVE), 0, S(stream), G, dt_boxes, gt_boxes, gt_crowd, A, B, iou);
  return check_launch(what);
}

int mi355det_coco_match(int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets, int64_t num_dt,
                        int64_t num_gt, int64_t iou_size, const double* iou, const double* dt_area, const double* gt_area,
                        const uint8_t* gt_crowd, const double* iou_thrs, int32_t num_thrs, const double* area_rngs, int32_t num_areas,
                        int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, void* stream) {
  return match_entry("coco_match", false, false, num_groups, dt_offsets, gt_offsets, iou_offsets, num_dt, num_gt, iou_size, iou, dt_area, gt_area,
                     gt_crowd, nullptr, nullptr, iou_thrs, num_thrs, area_rngs, num_areas, dt_match, dt_ignore, gt_match, gt_ignore, stream);
}

int mi355det_lvis_match(int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets, int64_t num_dt,
                        int64_t num_gt, int64_t iou_size, const double* iou, const double* dt_area, const double* gt_area,
                        const uint8_t* gt_flag, const uint8_t* group_not_exhaustive, const double* iou_thrs, int32_t num_thrs,
                        const double* area_rngs, int32_t num_areas, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore,
                        void* stream) {
  return match_entry("lvis_match", true, false, num_groups, dt_offsets, gt_offsets, iou_offsets, num_dt, num_gt, iou_size, iou, dt_area, gt_area,
                     gt_flag, nullptr, group_not_exhaustive, iou_thrs, num_thrs, area_rngs, num_areas, dt_match, dt_ignore, gt_match, gt_ignore, stream);
}

int mi355det_keypoints_match(int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets, int64_t num_dt,
                             int64_t num_gt, int64_t iou_size, const double* iou, const double* dt_area, const double* gt_area,
                             const uint8_t* gt_flag, const uint8_t* gt_crowd, const double* iou_thrs, int32_t num_thrs, const double* area_rngs,
                             int32_t num_areas, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, void* stream) {
  return match_entry("keypoints_match", false, true, num_groups, dt_offsets, gt_offsets, iou_offsets, num_dt, num_gt, iou_size, iou, dt_area,
                     gt_area, gt_flag, gt_crowd, nullptr, iou_thrs, num_thrs, area_rngs, num_areas, dt_match, dt_ignore, gt_match, gt_ignore,
                     stream);
}

int mi355det_coco_accumulate(int32_t num_cats, const int64_t* cat_dt_offsets, const int64_t* cat_gt_offsets, int64_t num_dt, int64_t num_gt,
                             const int64_t* order, const int32_t* dt_rank, const double* dt_score, const int32_t* dt_match,
                             const uint8_t* dt_ignore, const uint8_t* gt_ignore, int32_t num_thrs, int32_t num_areas, const int32_t* max_dets,
                             int32_t num_max_dets, const double* rec_thrs, int32_t num_recs, double* precision, double* recall, double* scores,
                             void* stream) {
  const char* what = "coco_accumulate";
  if (num_cats < 0 || num_dt < 0 || num_gt < 0 || num_thrs <= 0 || num_areas <= 0 || num_recs <= 0 || num_recs > 4096)
    return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (num_max_dets <= 0 || num_max_dets > 8 || !max_dets) return fail(MI355DET_EINVAL, "%s: 1..8 maxDets", what);
  if (num_cats == 0) return MI355DET_OK;
  const long long blocks = (long long)num_cats * num_areas * num_max_dets * num_thrs;
  if (blocks >= (1ll << 31)) return fail(MI355DET_EINVAL, "%s: too many categories", what);
  if (!cat_dt_offsets || !cat_gt_offsets || !rec_thrs || !precision || !recall || !scores)
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if ((num_dt > 0 && (!order || !dt_rank || !dt_score || !dt_match || !dt_ignore)) || (num_gt > 0 && !gt_ignore))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  MaxDets MD{};
  for (int i = 0; i < num_max_dets; ++i) MD.v[i] = max_dets[i];
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)blocks), dim3(WAVE), (size_t)num_recs * sizeof(double), S(stream), num_cats,
                     (const long long*)cat_dt_offsets, (const long long*)cat_gt_offsets, (long long)num_dt, (long long)num_gt,
                     (const long long*)order, dt_rank, dt_score, dt_match, dt_ignore, gt_ignore, num_thrs, num_areas, MD, num_max_dets, rec_thrs,
                     num_recs, precision, recall, scores);
  return check_launch(what);
}

}  // extern "C"
