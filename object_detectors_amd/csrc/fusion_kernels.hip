// Weighted boxes fusion on the device (include/mi355det.h, "Weighted boxes fusion"): the candidates of one (image, category) group, already in
// fusion order, are clustered one after the other against the fused boxes of the clusters made so far.
//
//   wbf_fuse_kernel   block = one wavefront, grid-stride over groups.  Per candidate the 64 lanes stride over the group's clusters, cluster c
//                     always on lane c % 64: that lane evaluates the overlap against the cached fused box, a ballot finds the lanes past the
//                     threshold, a butterfly over the bits of the (positive) overlaps and one over the cluster indices pick the largest overlap
//                     and, among equals, the first cluster made; the winner's lane joins the candidate to its cluster and re-divides that one
//                     fused box, or lane count % 64 founds cluster number `count`.  A last walk writes each cluster's score and fused box.
//   storage           a cluster is its founder's slot: sums, maximum, member count, score and fused box are rows of the outputs at that slot.
//                     The fused boxes and founder slots of the first WBF_LDS_CLUSTERS clusters of a group are cached in LDS; later clusters
//                     are read back from the `fused` and `founders` rows the kernel wrote.
//   visibility        every row of a cluster - in LDS and in global memory - is written and read by the one lane c % 64, in that lane's program
//                     order, so no lane ever reads what another lane stored and the loop needs neither a barrier nor a fence; what the lanes
//                     exchange (the overlaps, the winner) goes through ballots and shuffles.  The candidates and the offsets are read only.
// float64 throughout, one division per overlapping pair and four per join, no atomics, 64-bit offsets, every element has one writer.
// Compiled with -ffp-contract=off: s' * coordinate is rounded before it is added, as the rule states it.
#include "common.h"
#include "wave_ops.h"

using namespace mi355;

namespace {

constexpr int WBF_LDS_CLUSTERS = 96;      // 96 * (32 + 8) B = 3840 B of LDS per one-wave workgroup: the LDS never limits the waves on a CU
constexpr int WBF_MAX_BLOCKS = 256 * 32;
constexpr int WBF_SUMS = 6;               // S1..S4, C, mx
enum { CONF_AVG = 0, CONF_MAX = 1 };

struct WbfOut {
  long long* leader;                      // [num_boxes] the founder slot of the cluster a candidate ended in
  long long* founders;                    // [num_boxes] row g0 + c: the founder slot of the group's cluster c
  double* sums;                           // [num_boxes, 6] at founder slots
  double* fused;                          // [num_boxes, 4] at founder slots, corners
  double* score;                          // [num_boxes] at founder slots
  int* members;                           // [num_boxes] at founder slots
};

__device__ __forceinline__ long long wave_max_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long w = shfl_xor_i64(v, o);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ long long wave_min_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long w = shfl_xor_i64(v, o);
    v = w < v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(WAVE) void wbf_fuse_kernel(const long long* __restrict__ offsets, long long num_groups, long long num_boxes,
                                                        const double* __restrict__ box, const double* __restrict__ score, double thr, int conf,
                                                        double wsum, double wmax, WbfOut o) {
  __shared__ double s_box[WBF_LDS_CLUSTERS][4];
  __shared__ long long s_slot[WBF_LDS_CLUSTERS];
  const int lane = threadIdx.x;
  for (long long g = blockIdx.x; g < num_groups; g += gridDim.x) {
    const long long g0 = offsets[g], g1 = offsets[g + 1];
    if (g0 < 0 || g1 < g0 || g1 > num_boxes) continue;     // the group does not fit: nothing of it is read or written
    long long count = 0;                                   // clusters so far; the same in every lane
    for (long long p = g0; p < g1; ++p) {
      const double bx1 = box[4 * p], by1 = box[4 * p + 1], bx2 = box[4 * p + 2], by2 = box[4 * p + 3], s = score[p];
      const double barea = (bx2 - bx1) * (by2 - by1);
      // this lane's clusters in creation order: strict > keeps the first of equal overlaps, and an overlap of 0 never joins (thr >= 0)
      double bv = 0.0;
      long long bc = -1;
      for (long long c = lane; c < count; c += WAVE) {
        double X1, Y1, X2, Y2;
        if (c < WBF_LDS_CLUSTERS) {
          X1 = s_box[c][0], Y1 = s_box[c][1], X2 = s_box[c][2], Y2 = s_box[c][3];
        } else {
          const long long f = o.founders[g0 + c];
          X1 = o.fused[4 * f], Y1 = o.fused[4 * f + 1], X2 = o.fused[4 * f + 2], Y2 = o.fused[4 * f + 3];
        }
        const double iw = fmin(X2, bx2) - fmax(X1, bx1);
        if (iw <= 0) continue;
        const double ih = fmin(Y2, by2) - fmax(Y1, by1);
        if (ih <= 0) continue;
        const double i = iw * ih;
        const double v = i / ((X2 - X1) * (Y2 - Y1) + barea - i);
        if (v > bv) bv = v, bc = c;
      }
      const bool past = bv > thr;
      const unsigned long long m = __ballot(past);
      long long win = -1;                                  // the cluster joined; -1: a new one
      if (m) {
        unsigned long long top = m;
        if (m & (m - 1)) {                                 // several lanes: the largest overlap (positive doubles order as their bits)
          const long long bits = past ? __double_as_longlong(bv) : -1;
          const long long best = wave_max_i64(bits);
          top = __ballot(past && bits == best);
        }
        // the first cluster made among the lanes that hold the largest overlap
        win = wave_min_i64(((top >> lane) & 1) ? bc : 0x7fffffffffffffffll);
      }
      const long long c = win >= 0 ? win : count;
      if (lane == (int)(c % WAVE)) {
        if (win >= 0) {
          const long long f = c < WBF_LDS_CLUSTERS ? s_slot[c] : o.founders[g0 + c];
          double* S = o.sums + WBF_SUMS * f;
          const double S1 = S[0] + s * bx1, S2 = S[1] + s * by1, S3 = S[2] + s * bx2, S4 = S[3] + s * by2, C = S[4] + s;
          S[0] = S1, S[1] = S2, S[2] = S3, S[3] = S4, S[4] = C, S[5] = fmax(S[5], s);
          o.members[f] += 1;
          const double X1 = S1 / C, Y1 = S2 / C, X2 = S3 / C, Y2 = S4 / C;
          if (c < WBF_LDS_CLUSTERS) s_box[c][0] = X1, s_box[c][1] = Y1, s_box[c][2] = X2, s_box[c][3] = Y2;
          else o.fused[4 * f] = X1, o.fused[4 * f + 1] = Y1, o.fused[4 * f + 2] = X2, o.fused[4 * f + 3] = Y2;
          o.leader[p] = f;
        } else {                                           // the founder's box is kept as it is: (s * x) / s need not be x
          if (c < WBF_LDS_CLUSTERS) s_box[c][0] = bx1, s_box[c][1] = by1, s_box[c][2] = bx2, s_box[c][3] = by2, s_slot[c] = p;
          else o.fused[4 * p] = bx1, o.fused[4 * p + 1] = by1, o.fused[4 * p + 2] = bx2, o.fused[4 * p + 3] = by2;
          o.founders[g0 + c] = p;
          double* S = o.sums + WBF_SUMS * p;
          S[0] = s * bx1, S[1] = s * by1, S[2] = s * bx2, S[3] = s * by2, S[4] = s, S[5] = s;
          o.members[p] = 1;
          o.leader[p] = p;
        }
      }
      if (win < 0) ++count;
    }
    // scores and the fused boxes still in LDS, each cluster by its own lane
    for (long long c = lane; c < count; c += WAVE) {
      const bool cached = c < WBF_LDS_CLUSTERS;
      const long long f = cached ? s_slot[c] : o.founders[g0 + c];
      if (cached) o.fused[4 * f] = s_box[c][0], o.fused[4 * f + 1] = s_box[c][1], o.fused[4 * f + 2] = s_box[c][2], o.fused[4 * f + 3] = s_box[c][3];
      const double n = (double)o.members[f];
      o.score[f] = conf == CONF_MAX ? o.sums[WBF_SUMS * f + 5] / wmax : ((o.sums[WBF_SUMS * f + 4] / n) * fmin(n, wsum)) / wsum;
    }
  }
}

}  // namespace

extern "C" {

int mi355det_wbf_lds_clusters(void) { return WBF_LDS_CLUSTERS; }

int mi355det_wbf_fuse(const int64_t* group_offsets, int64_t num_groups, int64_t num_boxes, const double* boxes, const double* scores,
                      double iou_thr, int32_t conf_type, double weight_sum, double weight_max, int64_t* leader, int64_t* founders, double* sums,
                      double* fused, double* out_scores, int32_t* members, void* stream) {
  const char* what = "wbf_fuse";
  if (num_groups < 0 || num_boxes < 0) return fail(MI355DET_EINVAL, "%s: negative size", what);
  if (!(iou_thr >= 0 && iou_thr < 1)) return fail(MI355DET_EINVAL, "%s: iou_thr must lie in [0, 1)", what);
  if (conf_type != CONF_AVG && conf_type != CONF_MAX) return fail(MI355DET_EINVAL, "%s: conf_type must be 0 (avg) or 1 (max)", what);
  if (!(weight_sum > 0 && weight_sum < INFINITY && weight_max > 0 && weight_max < INFINITY))
    return fail(MI355DET_EINVAL, "%s: the weight sum and the largest weight must be positive and finite", what);
  if (num_boxes > 0 && (!group_offsets || !boxes || !scores || !leader || !founders || !sums || !fused || !out_scores || !members))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if (num_groups > 0 && !group_offsets) return fail(MI355DET_EINVAL, "%s: missing group offsets", what);
  if (num_groups == 0 || num_boxes == 0) return MI355DET_OK;
  const WbfOut o{(long long*)leader, (long long*)founders, sums, fused, out_scores, members};
  const unsigned grid = (unsigned)(num_groups < WBF_MAX_BLOCKS ? num_groups : WBF_MAX_BLOCKS);
  hipLaunchKernelGGL(wbf_fuse_kernel, dim3(grid), dim3(WAVE), 0, S(stream), (const long long*)group_offsets, (long long)num_groups,
                     (long long)num_boxes, boxes, scores, iou_thr, (int)conf_type, weight_sum, weight_max, o);
  return check_launch(what);
}

}  // extern "C"
