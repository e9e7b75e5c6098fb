// Bootstrap replicates of the COCO / LVIS accumulate pass (include/mi355det.h, "Bootstrap replicates").
//
// After coco_match / lvis_match every match decision is fixed; a replicate - the data set in which image i occurs weights[i][b] times - only
// changes how often each detection slot and each ground truth counts.  coco_bootstrap_kernel is coco_accumulate_kernel
// (cocoeval_kernels.hip) with the axes turned: there a wave walks one replicate 64 slots at a time, here
//   block = one wave = (chunk of 64 replicates, k, a, m, t), lane = replicate.
// The wave walks the category's slots in score order, 64 at a time: lane j loads slot j's order / rank / match / ignore / image (coalesced)
// and three ballots turn the flags into wave-uniform masks; the inner walk then takes the slots one by one, in groups of 8 whose weights
// (weights [num_images, B]: 64 lanes = 256 contiguous bytes per slot) are loaded ahead of their use.  A group without a kept slot is skipped
// by the whole wave.  Forward for the totals, then backward: the cumulative sums are rebuilt from the totals (integers: exact), the running
// maximum of the precision is carried from the right, and a slot that is the first to reach recall thresholds adds the envelope once per
// threshold - in descending threshold order, one addition each - to the lane's ap_sum.  Nothing of size [.., num_recs, ..] is written.
// tp / fp / npig / carry / ap_sum live in registers, the recall thresholds in LDS.  float64, no atomics, one writer per output element.
// Compiled with -ffp-contract=off: the quotients are those of coco_accumulate_kernel, operation for operation.
#include "common.h"

using namespace mi355;

namespace {

constexpr int GROUP = 8;            // slots whose weights are in flight together

struct BootMaxDets {
  int v[8];
};

// the 64 slots [base, base + 64) of one walk as wave-uniform masks, and per lane the image of slot base + lane (0 where the slot does not count)
struct SlotChunk {
  unsigned long long valid, tp, fp;
  int image;
};

__global__ __launch_bounds__(WAVE) void coco_bootstrap_kernel(int K, const long long* __restrict__ cat_dt_off, const long long* __restrict__ cat_gt_off,
                                                              long long num_dt, long long num_gt, const long long* __restrict__ order,
                                                              const int* __restrict__ dt_rank, const int* __restrict__ dt_match,
                                                              const unsigned char* __restrict__ dt_ignore, const unsigned char* __restrict__ gt_ignore,
                                                              const int* __restrict__ dt_image, const int* __restrict__ gt_image,
                                                              const int* __restrict__ weights, int num_images, int B, int T, int A, BootMaxDets MD,
                                                              int M, const double* __restrict__ rec_thrs, int R, double* __restrict__ ap_sum,
                                                              double* __restrict__ recall) {
  extern __shared__ double s_thr[];
  const int lane = threadIdx.x;
  long long blk = blockIdx.x;
  const int t = (int)(blk % T);
  blk /= T;
  const int m = (int)(blk % M);
  blk /= M;
  const int a = (int)(blk % A);
  blk /= A;
  const int k = (int)(blk % K);
  const int rep = (int)(blk / K) * WAVE + lane;
  const bool live = rep < B;
  const int col = live ? rep : B - 1;                     // a lane past the last replicate reads the last column and writes nothing
  for (int r = lane; r < R; r += WAVE) s_thr[r] = rec_thrs[r];
  __syncthreads();
  long long c0 = cat_dt_off[k], c1 = cat_dt_off[k + 1], g0 = cat_gt_off[k], g1 = cat_gt_off[k + 1];
  if (c0 < 0 || c1 < c0 || c1 > num_dt) c0 = c1 = 0;
  if (g0 < 0 || g1 < g0 || g1 > num_gt) g0 = g1 = 0;
  const long long N = c1 - c0;
  const int maxdet = MD.v[m];
  const int* dm = dt_match + ((size_t)a * T + t) * num_dt;
  const unsigned char* di = dt_ignore + ((size_t)a * T + t) * num_dt;
  const size_t out = ((((size_t)rep * T + t) * K + k) * A + a) * M + m;                 // ap_sum, recall [B, T, K, A, M]
  auto weight = [&](int image) { return (long long)max(weights[(size_t)image * B + col], 0); };        // a negative weight counts as 0

  // npig: the weighted count of the category's non-ignored ground truths
  long long npig = 0;
  for (long long base = g0; base < g1; base += WAVE) {
    const long long g = base + lane;
    int image = 0;
    bool counts = false;
    if (g < g1) {
      image = gt_image[g];
      counts = !gt_ignore[(size_t)a * num_gt + g] && image >= 0 && image < num_images;
    }
    if (!counts) image = 0;
    unsigned long long mask = __ballot(counts);
    while (mask) {
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      npig += weight(__shfl(image, j, WAVE));
    }
  }
  // no image of the replicate holds a ground truth that counts: -1.  Not a return: the lanes of one wave differ here, and all of them take
  // part in the ballots and shuffles below.
  if (npig == 0 && live) ap_sum[out] = recall[out] = -1.0;

  auto chunk = [&](long long base) {
    const long long p = base + lane;
    bool valid = false, tp = false, fp = false;
    int image = 0;
    if (p < N) {
      const long long idx = order[c0 + p];
      if (idx >= 0 && idx < num_dt && dt_rank[idx] < maxdet) {
        const int im = dt_image[idx];
        if (im >= 0 && im < num_images) {                 // an image outside the table: weight 0, never dereferenced
          const bool matched = dm[idx] != 0, ign = di[idx] != 0;
          valid = true;
          image = im;
          tp = matched && !ign;
          fp = !matched && !ign;
        }
      }
    }
    return SlotChunk{__ballot(valid), __ballot(tp), __ballot(fp), image};
  };

  // forward: the totals
  long long tot_tp = 0, tot_fp = 0, tot_nd = 0;
  for (long long base = 0; base < N; base += WAVE) {
    const SlotChunk c = chunk(base);
    for (int j0 = 0; j0 < WAVE; j0 += GROUP) {
      if (((c.valid >> j0) & ((1ull << GROUP) - 1)) == 0) continue;
      long long w[GROUP];
#pragma unroll
      for (int u = 0; u < GROUP; ++u) w[u] = weight(__shfl(c.image, j0 + u, WAVE));
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        const int j = j0 + u;
        if (!((c.valid >> j) & 1)) continue;
        tot_nd += w[u];
        if ((c.tp >> j) & 1) tot_tp += w[u];
        if ((c.fp >> j) & 1) tot_fp += w[u];
      }
    }
  }
  const double dn = (double)npig;
  // the number of recall thresholds <= x
  auto reached = [&](double x) {
    int lo = 0, hi = R;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_thr[mid] <= x) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const bool scored = npig > 0;
  if (live && scored) recall[out] = tot_nd > 0 ? (double)tot_tp / dn : 0.0;

  // backward.  r_top: the thresholds below it are still to be claimed; a true-positive slot (and the first kept slot) claims [r0, r_top),
  // where r0 counts the thresholds the slots before it reach, and adds the envelope once for each of them, highest threshold first.
  long long end_tp = tot_tp, end_fp = tot_fp, end_nd = tot_nd;
  double carry = -1.0, ap = 0.0;
  const double eps = 2.220446049250313e-16;            // 2^-52, numpy's spacing(1)
  int r_top = (scored && tot_nd > 0) ? reached((double)tot_tp / dn) : 0;
  for (long long base = ((N - 1) / WAVE) * WAVE; N > 0 && base >= 0; base -= WAVE) {
    const SlotChunk c = chunk(base);
    for (int j0 = WAVE - GROUP; j0 >= 0; j0 -= GROUP) {
      if (((c.valid >> j0) & ((1ull << GROUP) - 1)) == 0) continue;
      long long w[GROUP];
#pragma unroll
      for (int u = 0; u < GROUP; ++u) w[u] = weight(__shfl(c.image, j0 + u, WAVE));
#pragma unroll
      for (int u = GROUP - 1; u >= 0; --u) {
        const int j = j0 + u;
        if (!((c.valid >> j) & 1)) continue;
        const long long wj = w[u];
        if (wj <= 0 || !scored) continue;                 // a slot of weight 0 is not in the replicate
        const bool tp = (c.tp >> j) & 1, fp = (c.fp >> j) & 1;
        const double pr = (double)end_tp / ((double)end_fp + (double)end_tp + eps);
        carry = fmax(carry, pr);
        const bool first = end_nd == wj;
        if (tp || first) {
          const int r0 = first ? 0 : reached((double)(end_tp - wj) / dn);
          for (int r = r_top; r > r0; --r) ap += carry;
          if (r0 < r_top) r_top = r0;
        }
        if (tp) end_tp -= wj;
        if (fp) end_fp -= wj;
        end_nd -= wj;
      }
    }
  }
  if (live && scored) ap_sum[out] = ap;
}

}  // namespace

extern "C" {

int mi355det_coco_bootstrap(int32_t num_cats, const int64_t* cat_dt_offsets, const int64_t* cat_gt_offsets, int64_t num_dt, int64_t num_gt,
                            const int64_t* order, const int32_t* dt_rank, const int32_t* dt_match, const uint8_t* dt_ignore,
                            const uint8_t* gt_ignore, int32_t num_thrs, int32_t num_areas, const int32_t* max_dets, int32_t num_max_dets,
                            const double* rec_thrs, int32_t num_recs, const int32_t* dt_image, const int32_t* gt_image, const int32_t* weights,
                            int32_t num_images, int32_t num_replicates, double* ap_sum, double* recall, void* stream) {
  const char* what = "coco_bootstrap";
  if (num_cats <= 0 || num_dt < 0 || num_gt < 0 || num_thrs <= 0 || num_areas <= 0 || num_recs <= 0 || num_images <= 0 || num_replicates <= 0)
    return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (num_recs > 4096) return fail(MI355DET_EINVAL, "%s: at most 4096 recall thresholds", what);
  if (num_max_dets <= 0 || num_max_dets > 8 || !max_dets) return fail(MI355DET_EINVAL, "%s: 1..8 maxDets", what);
  if (!cat_dt_offsets || !cat_gt_offsets || !rec_thrs || !weights || !ap_sum || !recall) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if ((num_dt > 0 && (!order || !dt_rank || !dt_match || !dt_ignore || !dt_image)) || (num_gt > 0 && (!gt_ignore || !gt_image)))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  const long long chunks = ((long long)num_replicates + WAVE - 1) / WAVE;
  const long long blocks = chunks * num_cats * num_areas * num_max_dets * num_thrs;
  if (blocks >= (1ll << 31)) return fail(MI355DET_EINVAL, "%s: too many categories x replicates", what);
  BootMaxDets MD{};
  for (int i = 0; i < num_max_dets; ++i) MD.v[i] = max_dets[i];
  hipLaunchKernelGGL(coco_bootstrap_kernel, dim3((unsigned)blocks), dim3(WAVE), (size_t)num_recs * sizeof(double), S(stream), num_cats,
                     (const long long*)cat_dt_offsets, (const long long*)cat_gt_offsets, (long long)num_dt, (long long)num_gt,
                     (const long long*)order, dt_rank, dt_match, dt_ignore, gt_ignore, dt_image, gt_image, weights, num_images, num_replicates,
                     num_thrs, num_areas, MD, num_max_dets, rec_thrs, num_recs, ap_sum, recall);
  return check_launch(what);
}

}  // extern "C"
