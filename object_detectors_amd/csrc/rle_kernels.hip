// Mask results as COCO run lengths (include/mi355det.h, "Mask results as COCO run-length encodings"): what
// torchvision_models/detection/coco_eval.py:107-140 gets from `masks > 0.5` + pycocotools mask.encode, made on the device.
//
// pycocotools rleEncode: the pixels of one mask in column-major order i = x*H + y, bit(-1) = 0, a transition is an i with bit(i) != bit(i-1),
// the counts are the gaps between successive transitions (the first from 0, the last to H*W).  The predecessor of (x, 0) is (x-1, H-1): a
// run goes on across a column boundary, so a column's first transition is judged against the last pixel of the column before it.
//
// One column walk (walk_column) over a per-pixel predicate, with two predicates:
//   DenseSrc   dense[d][y][x] > threshold.  Thread = column, so adjacent lanes read adjacent x of one row.
//   PasteSrc   paste_value(...) > threshold: the pixel paste_masks_kernel would write (mask_paste.h), never stored.  A bilinearly enlarged
//              m x m mask is piecewise linear, so a column holds a few dozen runs at most; columns outside the clipped box end at once and
//              rows outside it are never evaluated.
// Passes (all fixed-order, no atomics):
//   rle_count_kernel    thread (d, x): the column's transitions, its last transition's position, its set pixels and their y range.
//   rle_scan_kernel     block d: exclusive prefix sum of the transitions (the column's first index among the mask's transitions) and
//                       exclusive prefix max of the last positions (positions grow with x, so this IS the transition before the column),
//                       plus the mask's area and tight box.
//   offsets scan        one block (offsets_scan.h): run_offsets[d] = sum over d' < d of (transitions + 1).
//   rle_emit_kernel     thread (d, x): walks the column again and writes each transition's gap to the one before; thread x = 0 also writes the
//                       mask's last count, area and box.
// Compiled with -ffp-contract=off like mask_kernels.hip: the paste predicate has to see the bits paste_masks_kernel writes.
#include "common.h"
#include "mask_paste.h"
#include "offsets_scan.h"
#include "rle_protocol.h"

#include <limits.h>

using namespace mi355;

namespace {

struct ColStats {
  int nset = 0, ymin = INT_MAX, ymax = -1;
};

// ---- the two predicates.  det(d) is one mask's view: rows(x, ylo, yhi) = the rows of column x that can hold a set bit (ylo == yhi: none),
//      bit(x, y) = the bit itself, valid for every pixel of the image.
struct DenseSrc {
  const float* p;
  int H, W;
  float thr;
  struct Det {
    const float* p;
    int H, W;
    float thr;
    __device__ __forceinline__ void rows(int, int& ylo, int& yhi) const {
      ylo = 0;
      yhi = H;
    }
    __device__ __forceinline__ bool bit(int x, int y) const { return p[(size_t)y * W + x] > thr; }
  };
  __device__ __forceinline__ Det det(int d) const { return Det{p + (size_t)d * H * W, H, W, thr}; }
};

struct PasteSrc {
  const float* masks;
  const float* boxes;
  int M, pad, H, W;
  float thr;
  struct Det {
    const float* m;
    PasteBox B;
    int M, pad;
    float thr;
    __device__ __forceinline__ void rows(int x, int& ylo, int& yhi) const {
      const bool live = x >= B.x0 && x < B.x1 && B.y1 > B.y0;
      ylo = live ? (int)B.y0 : 0;
      yhi = live ? (int)B.y1 : 0;
    }
    __device__ __forceinline__ bool bit(int x, int y) const { return B.has(x, y) && paste_value(m, M, pad, B, x, y) > thr; }
  };
  __device__ __forceinline__ Det det(int d) const {
    return Det{masks + (size_t)d * M * M, paste_box(boxes + 4 * (size_t)d, paste_scale(M, pad), H, W), M, pad, thr};
  }
};

// the transitions of column x in pixel order: emit(i) for every i = x*H + y with bit(i) != bit(i-1)
template <class Det, class Emit>
__device__ __forceinline__ void walk_column(const Det& det, int x, int H, ColStats& st, Emit&& emit) {
  int ylo, yhi;
  det.rows(x, ylo, yhi);
  bool prev = x > 0 && det.bit(x - 1, H - 1);
  const int base = x * H;                             // < 2^31: the entry points refuse H*W >= 2^31
  if (prev && (ylo > 0 || yhi <= ylo)) {              // the run of the column before ends at this column's first pixel
    emit(base);
    prev = false;
  }
#pragma unroll 4
  for (int y = ylo; y < yhi; ++y) {
    const bool b = det.bit(x, y);
    if (b != prev) {
      emit(base + y);
      prev = b;
    }
    if (b) {
      ++st.nset;
      st.ymin = min(st.ymin, y);
      st.ymax = y;
    }
  }
  if (prev && yhi > ylo && yhi < H) emit(base + yhi);
}

// ---- workspace: five int32 tables [D, W], then per mask transitions | last position | box[4] (int32) and area (int64, 8-byte aligned)
struct Tables {
  int *cnt, *last, *nset, *ymin, *ymax;          // [D, W]; after the scan cnt = the column's first transition index, last = the position before
  int *total, *tail, *box;                       // [D], [D], [D, 4]
  long long* area;                               // [D]
};

inline size_t table_ints(int D, int W) { return ((5 * (size_t)D * W + 6 * (size_t)D + 1) / 2) * 2; }

inline Tables tables(void* ws, int D, int W) {
  const size_t n = (size_t)D * W;
  int* p = (int*)ws;
  Tables T;
  T.cnt = p;
  T.last = p + n;
  T.nset = p + 2 * n;
  T.ymin = p + 3 * n;
  T.ymax = p + 4 * n;
  T.total = p + 5 * n;
  T.tail = T.total + D;
  T.box = T.tail + D;
  T.area = (long long*)(p + table_ints(D, W));
  return T;
}

template <class Src>
__global__ __launch_bounds__(256) void rle_count_kernel(Src S, int D, int H, int W, int chunks, Tables T) {
  const int d = blockIdx.x / chunks, x = (blockIdx.x % chunks) * 256 + threadIdx.x;
  if (d >= D || x >= W) return;
  const auto det = S.det(d);
  ColStats st;
  int n = 0, last = 0;
  walk_column(det, x, H, st, [&](int pos) {
    ++n;
    last = pos;
  });
  const size_t c = (size_t)d * W + x;
  T.cnt[c] = n;
  T.last[c] = last;
  T.nset[c] = st.nset;
  T.ymin[c] = st.ymin;
  T.ymax[c] = st.ymax;
}

__global__ __launch_bounds__(256) void rle_scan_kernel(int D, int W, Tables T) {
  __shared__ int s_sum[256], s_max[256];
  __shared__ long long s_area[256];
  const int d = blockIdx.x, t = threadIdx.x;
  if (d >= D) return;
  int carry_sum = 0, carry_max = 0;
  long long area = 0;
  int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
  for (int base = 0; base < W; base += 256) {
    const int x = base + t;
    const size_t c = (size_t)d * W + x;
    const int n = x < W ? T.cnt[c] : 0, l = x < W ? T.last[c] : 0;
    s_sum[t] = n;
    s_max[t] = l;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {               // inclusive scans: sum of the transitions, max of the last positions
      const int a = t >= o ? s_sum[t - o] : 0, b = t >= o ? s_max[t - o] : 0;
      __syncthreads();
      s_sum[t] += a;
      s_max[t] = max(s_max[t], b);
      __syncthreads();
    }
    if (x < W) {
      T.cnt[c] = carry_sum + s_sum[t] - n;
      T.last[c] = max(carry_max, t > 0 ? s_max[t - 1] : 0);
      const int ns = T.nset[c];
      if (ns > 0) {
        area += ns;
        xmin = min(xmin, x);
        xmax = max(xmax, x);
        ymin = min(ymin, T.ymin[c]);
        ymax = max(ymax, T.ymax[c]);
      }
    }
    carry_sum += s_sum[255];
    carry_max = max(carry_max, s_max[255]);
    __syncthreads();
  }
  // the mask's area and tight box: integer tree reductions (order-free, so exact)
  s_area[t] = area;
  s_sum[t] = xmin;
  s_max[t] = xmax;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      s_area[t] += s_area[t + s];
      s_sum[t] = min(s_sum[t], s_sum[t + s]);
      s_max[t] = max(s_max[t], s_max[t + s]);
    }
    __syncthreads();
  }
  area = s_area[0];
  xmin = s_sum[0];
  xmax = s_max[0];
  __syncthreads();
  s_sum[t] = ymin;
  s_max[t] = ymax;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      s_sum[t] = min(s_sum[t], s_sum[t + s]);
      s_max[t] = max(s_max[t], s_max[t + s]);
    }
    __syncthreads();
  }
  if (t == 0) {
    ymin = s_sum[0];
    ymax = s_max[0];
    T.total[d] = carry_sum;
    T.tail[d] = carry_max;
    T.area[d] = area;
    const bool any = area > 0;
    T.box[4 * d + 0] = any ? xmin : 0;
    T.box[4 * d + 1] = any ? ymin : 0;
    T.box[4 * d + 2] = any ? xmax - xmin + 1 : 0;
    T.box[4 * d + 3] = any ? ymax - ymin + 1 : 0;
  }
}

struct CountsOf {                                        // a mask's counts: its transitions + 1
  const int* total;
  __device__ __forceinline__ long long operator()(long long d) const { return (long long)total[d] + 1; }
};

template <class Src>
__global__ __launch_bounds__(256) void rle_emit_kernel(Src S, int D, int H, int W, int chunks, Tables T, const long long* __restrict__ run_offsets,
                                                       int* __restrict__ counts, long long capacity, long long* __restrict__ area,
                                                       int* __restrict__ bbox) {
  const int d = blockIdx.x / chunks, x = (blockIdx.x % chunks) * 256 + threadIdx.x;
  if (d >= D || x >= W) return;
  const long long first = run_offsets[d];
  if (x == 0) {                                       // the last count runs to H*W; the per-mask results of the scan
    const long long k = first + T.total[d];
    if (k >= 0 && k < capacity) counts[k] = H * W - T.tail[d];
    if (area) area[d] = T.area[d];
    if (bbox)
      for (int j = 0; j < 4; ++j) bbox[4 * d + j] = T.box[4 * d + j];
  }
  const auto det = S.det(d);
  const size_t c = (size_t)d * W + x;
  long long k = first + T.cnt[c];
  int before = T.last[c];
  ColStats st;
  walk_column(det, x, H, st, [&](int pos) {
    if (k >= 0 && k < capacity) counts[k] = pos - before;
    before = pos;
    ++k;
  });
}

int check_args(const char* what, const float* dense, const float* masks, const float* boxes, int D, int m, int padding, int H, int W,
               float threshold) {
  if (D < 0 || H <= 0 || W <= 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if ((long long)H * W >= (1ll << 31)) return fail(MI355DET_EINVAL, "%s: im_h*im_w = %lld does not fit the int32 counts", what, (long long)H * W);
  if (!dense) {
    if (m <= 0 || padding < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
    if (!(threshold >= 0.f)) return fail(MI355DET_EINVAL, "%s: the paste source needs threshold >= 0 (pixels outside the box are 0)", what);
    if (D > 0 && (!masks || !boxes)) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  }
  if ((long long)D * ((W + 255) / 256) >= (1ll << 31)) return fail(MI355DET_EINVAL, "%s: too many masks", what);
  return MI355DET_OK;
}

}  // namespace

extern "C" {

size_t mi355det_mask_rle_workspace(int32_t num_masks, int32_t im_w) {
  if (num_masks <= 0 || im_w <= 0) return 0;
  return table_ints(num_masks, im_w) * sizeof(int) + (size_t)num_masks * sizeof(long long);
}

int mi355det_mask_rle_count(const float* dense, const float* masks, const float* boxes, int32_t num_masks, int32_t m, int32_t padding,
                            int32_t im_h, int32_t im_w, float threshold, int64_t* run_offsets, void* workspace, size_t workspace_bytes,
                            void* stream) {
  const int st = check_args("mask_rle_count", dense, masks, boxes, num_masks, m, padding, im_h, im_w, threshold);
  if (st != MI355DET_OK) return st;
  if (num_masks == 0) return MI355DET_OK;
  if (!run_offsets) return fail(MI355DET_EINVAL, "%s: missing operand", "mask_rle_count");
  if (!workspace || workspace_bytes < mi355det_mask_rle_workspace(num_masks, im_w))
    return fail(MI355DET_EWORKSPACE, "%s: workspace too small", "mask_rle_count");
  const Tables T = tables(workspace, num_masks, im_w);
  const int chunks = (im_w + 255) / 256;
  if (dense)
    hipLaunchKernelGGL(rle_count_kernel<DenseSrc>, dim3(num_masks * chunks), dim3(256), 0, S(stream), DenseSrc{dense, im_h, im_w, threshold},
                       num_masks, im_h, im_w, chunks, T);
  else
    hipLaunchKernelGGL(rle_count_kernel<PasteSrc>, dim3(num_masks * chunks), dim3(256), 0, S(stream),
                       PasteSrc{masks, boxes, m, padding, im_h, im_w, threshold}, num_masks, im_h, im_w, chunks, T);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(num_masks), dim3(256), 0, S(stream), num_masks, im_w, T);
  launch_offsets_scan(num_masks, CountsOf{T.total}, (long long*)run_offsets, stream);
  return check_launch("mask_rle_count");
}

int mi355det_mask_rle_emit(const float* dense, const float* masks, const float* boxes, int32_t num_masks, int32_t m, int32_t padding,
                           int32_t im_h, int32_t im_w, float threshold, const int64_t* run_offsets, int64_t total_runs, int32_t* counts,
                           int64_t capacity, int64_t* area, int32_t* bbox, void* workspace, size_t workspace_bytes, void* stream) {
  const int st = check_args("mask_rle_emit", dense, masks, boxes, num_masks, m, padding, im_h, im_w, threshold);
  if (st != MI355DET_OK) return st;
  if (num_masks == 0) return MI355DET_OK;
  const int ce = check_emit("mask_rle_emit", "%s: total_runs %lld is below one count per mask", num_masks, total_runs, capacity, run_offsets, counts);
  if (ce != MI355DET_OK) return ce;
  if (!workspace || workspace_bytes < mi355det_mask_rle_workspace(num_masks, im_w))
    return fail(MI355DET_EWORKSPACE, "%s: workspace too small", "mask_rle_emit");
  const Tables T = tables(workspace, num_masks, im_w);
  const int chunks = (im_w + 255) / 256;
  if (dense)
    hipLaunchKernelGGL(rle_emit_kernel<DenseSrc>, dim3(num_masks * chunks), dim3(256), 0, S(stream), DenseSrc{dense, im_h, im_w, threshold},
                       num_masks, im_h, im_w, chunks, T, (const long long*)run_offsets, counts, (long long)capacity, (long long*)area, bbox);
  else
    hipLaunchKernelGGL(rle_emit_kernel<PasteSrc>, dim3(num_masks * chunks), dim3(256), 0, S(stream),
                       PasteSrc{masks, boxes, m, padding, im_h, im_w, threshold}, num_masks, im_h, im_w, chunks, T,
                       (const long long*)run_offsets, counts, (long long)capacity, (long long*)area, bbox);
  return check_launch("mask_rle_emit");
}

}  // extern "C"
