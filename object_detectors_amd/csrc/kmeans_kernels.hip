// Anchor k-means (include/mi355det.h, "Anchor k-means"): the box features, selection and area bands of the reference's
// yolo/utilities/kmeans_anchors.py, and Lloyd's iteration batched over problems (bands) and restarts, under the Euclidean or the 1 - IoU
// distance.  float64 throughout, compiled with -ffp-contract=off; no floating-point atomics anywhere.
//
// box_features_kernel   one thread per annotation: width, height, aspect, area and the band.
// kmeans_pass_kernel    one workgroup per KM_POINTS consecutive points, one point per thread.  The centres of every (problem, restart) are
//                       staged in LDS once; a thread reads its point once and walks the restarts: nearest centre of its own problem (strict <,
//                       so ties go to the lowest index), the label compared with and stored over the previous pass's (uint8 [R, N] in the
//                       workspace), the label key and the distance parked in LDS.  Then the workgroup turns round: one thread per accumulator
//                       (problem, restart, cluster, feature) adds the tile's points of that cluster in ascending point order, one more per
//                       (problem, restart) adds the minimal distances of the problem's points - in point order whatever their labels, so two
//                       restarts that reach the same clustering with the clusters numbered differently get the same inertia bits - and each
//                       stores its partial at part[accumulator][workgroup].  The tile is a compile-time constant, so the order of every sum depends on
//                       N alone.  Counts and changed labels are integers and go through atomics.
// kmeans_combine_kernel one workgroup per (problem, restart): a wave per accumulator, lane l adds the partials of workgroups l, l + 64, ... in
//                       ascending order, the 64 lane sums are folded by a fixed xor butterfly.  Thread 0 then applies the rules: counts,
//                       inertia, stop on an unchanged pass or at max_iter, otherwise centre = sum / count for non-empty clusters.  A finished
//                       (problem, restart) sets its done flag and adds 1 to status[0]; its workgroups return at once from then on, the pass
//                       kernel skips it per restart, and once status[0] = P * R both kernels return on a block-uniform read.  No workgroup
//                       ever waits for another: the only ordering is the stream's.
// kmeans_assign_kernel  labels and minimal distances against one centre set per problem.
#include "common.h"

using namespace mi355;

namespace {

constexpr int KM_POINTS = 256;          // points per workgroup = threads per workgroup: fixes the summation tree
constexpr int KM_MAX_P = 4;
constexpr int KM_MAX_R = 16;
constexpr int KM_MAX_K = 16;
constexpr int KM_MAX_F = 4;
constexpr int KM_ASSIGN_MAX_K = 64;
constexpr int KM_COMBINE_THREADS = 256;
constexpr int FEAT_THREADS = 256;

__global__ __launch_bounds__(FEAT_THREADS) void box_features_kernel(const double* __restrict__ wh, const int* __restrict__ image_index,
                                                                    const int* __restrict__ image_size, long long n_ann, int n_images,
                                                                    double* __restrict__ features, signed char* __restrict__ band,
                                                                    int* __restrict__ errors) {
  const long long i = (long long)blockIdx.x * FEAT_THREADS + threadIdx.x;
  if (i >= n_ann) return;
  const int im = image_index[i];
  double f[4];
  int b = -1;
  if (im < 0 || im >= n_images) {
    atomicAdd(errors, 1);
    f[0] = f[1] = f[2] = f[3] = __builtin_nan("");
  } else {
    const double W = (double)image_size[2 * (size_t)im], H = (double)image_size[2 * (size_t)im + 1];
    const double width = wh[2 * i] / W, height = wh[2 * i + 1] / H;
    const double aspect = width / height, area = width * height;
    f[0] = width, f[1] = height, f[2] = aspect, f[3] = area;
    if (aspect > 0.2 && aspect < 5.0) b = area < 0.01 ? 0 : (area > 0.01 && area < 0.1) ? 1 : area > 0.1 ? 2 : -1;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) features[4 * i + j] = f[j];
  band[i] = (signed char)b;
}

// the distance of the rules: squared differences summed in feature order, or 1 - IoU of two (w, h) boxes with a common corner
template <int F, bool IOU>
__device__ __forceinline__ double km_distance(const double* x, const double* c) {
  if (IOU) {
    const double i = fmin(x[0], c[0]) * fmin(x[1], c[1]);
    return 1.0 - i / (x[0] * x[1] + c[0] * c[1] - i);
  }
  double s = (x[0] - c[0]) * (x[0] - c[0]);
#pragma unroll
  for (int j = 1; j < F; ++j) s = s + (x[j] - c[j]) * (x[j] - c[j]);
  return s;
}

template <int F, bool IOU>
__device__ __forceinline__ int km_nearest(const double* x, const double* cent, int k, double* dmin) {
  int best = 0;
  double bd = km_distance<F, IOU>(x, cent);
  for (int c = 1; c < k; ++c) {
    const double d = km_distance<F, IOU>(x, cent + c * F);
    if (d < bd) bd = d, best = c;
  }
  *dmin = bd;
  return best;
}

size_t pass_lds_bytes(int P, int R, int k, int F) {
  return ((size_t)P * R * k * F + (size_t)R * KM_POINTS + (size_t)KM_POINTS * F) * sizeof(double) + (size_t)R * KM_POINTS + 2 * (size_t)P * R * sizeof(int);
}

template <int F, bool IOU>
__global__ __launch_bounds__(KM_POINTS) void kmeans_pass_kernel(const double* __restrict__ x, const signed char* __restrict__ problem, long long n,
                                                                int P, int R, int k, const double* __restrict__ centers,
                                                                const int* __restrict__ done, const int* __restrict__ status,
                                                                unsigned char* __restrict__ labels8, double* __restrict__ part, long long nblocks,
                                                                int* __restrict__ counts_acc, int* __restrict__ changed) {
  if (status[0] >= P * R) return;                           // every (problem, restart) has finished: the same word for the whole grid
  extern __shared__ double s_mem[];
  double* s_cent = s_mem;                                   // [P, R, k, F]
  double* s_dist = s_cent + P * R * k * F;                  // [R, KM_POINTS]
  double* s_x = s_dist + R * KM_POINTS;                     // [KM_POINTS, F]
  unsigned char* s_key = (unsigned char*)(s_x + KM_POINTS * F);   // [R, KM_POINTS]: problem * k + label, 255 = takes no part
  int* s_done = (int*)(s_key + R * KM_POINTS);              // [P, R]
  int* s_changed = s_done + P * R;                          // [P, R]
  const int tid = threadIdx.x;
  for (int e = tid; e < P * R * k * F; e += KM_POINTS) s_cent[e] = centers[e];
  for (int e = tid; e < P * R; e += KM_POINTS) s_done[e] = done[e], s_changed[e] = 0;
  __syncthreads();

  const long long i = (long long)blockIdx.x * KM_POINTS + tid;
  int p = -1;
  double xi[F];
#pragma unroll
  for (int j = 0; j < F; ++j) xi[j] = 0.0;
  if (i < n) {
    p = problem ? (int)problem[i] : 0;
    if (p >= P) p = -1;
    if (p >= 0) {
#pragma unroll
      for (int j = 0; j < F; ++j) xi[j] = x[i * F + j];
    }
  }
#pragma unroll
  for (int j = 0; j < F; ++j) s_x[tid * F + j] = xi[j];
  for (int r = 0; r < R; ++r) {
    unsigned char key = 255;
    double d = 0.0;
    if (p >= 0 && !s_done[p * R + r]) {
      const int best = km_nearest<F, IOU>(xi, s_cent + (size_t)(p * R + r) * k * F, k, &d);
      unsigned char* slot = labels8 + (size_t)r * (size_t)n + (size_t)i;
      if (*slot != (unsigned char)best) {
        atomicAdd(&s_changed[p * R + r], 1);
        *slot = (unsigned char)best;
      }
      key = (unsigned char)(p * k + best);
    }
    s_key[r * KM_POINTS + tid] = key;
    s_dist[r * KM_POINTS + tid] = d;
  }
  __syncthreads();

  const int items = k * F + 1, n_acc = P * R * items;    // per (problem, restart): k * F coordinate sums, then the inertia
  for (int a = tid; a < n_acc; a += KM_POINTS) {
    const int pr = a / items, item = a % items, pp = pr / R, r = pr % R;
    if (s_done[pr]) continue;
    const bool coord = item < k * F;
    const int c = coord ? item / F : 0, j = coord ? item % F : 0;
    // a coordinate sum takes the points of its cluster; the inertia takes every point of the problem, in point order whatever the labels
    const int lo = pp * k + c, hi = coord ? lo : pp * k + k - 1;
    const unsigned char* keys = s_key + r * KM_POINTS;
    const double* src = coord ? s_x + j : s_dist + r * KM_POINTS;
    const int stride = coord ? F : 1;
    double acc = 0.0;
    int cnt = 0;
    for (int q = 0; q < KM_POINTS; ++q) {
      const int key = keys[q];
      if (key >= lo && key <= hi) acc = acc + src[q * stride], ++cnt;
    }
    part[(long long)a * nblocks + blockIdx.x] = acc;
    if (coord && j == 0 && cnt) atomicAdd(&counts_acc[pr * k + c], cnt);
  }
  for (int e = tid; e < P * R; e += KM_POINTS)
    if (s_changed[e]) atomicAdd(&changed[e], s_changed[e]);
}

__global__ __launch_bounds__(KM_COMBINE_THREADS) void kmeans_combine_kernel(int R, int k, int F, int max_iter, const double* __restrict__ part,
                                                                            long long nblocks, int* __restrict__ counts_acc,
                                                                            int* __restrict__ changed, int* __restrict__ done,
                                                                            int* __restrict__ status, double* __restrict__ centers,
                                                                            double* __restrict__ sums, int* __restrict__ counts,
                                                                            double* __restrict__ inertia, int* __restrict__ n_iter,
                                                                            int* __restrict__ last_changed) {
  const int pr = blockIdx.x;
  if (done[pr]) return;                                     // frozen: centres, counts, inertia and n_iter stay as they are
  __shared__ double s_tot[KM_MAX_K * KM_MAX_F + 1];
  const int items = k * F + 1;
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  for (int item = wave; item < items; item += KM_COMBINE_THREADS / WAVE) {
    const double* row = part + ((long long)pr * items + item) * nblocks;
    double v = 0.0;
    for (long long b = lane; b < nblocks; b += WAVE) v = v + row[b];
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, WAVE);
    if (lane == 0) s_tot[item] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int ch = changed[pr], it = n_iter[pr] + 1;
  changed[pr] = 0;
  n_iter[pr] = it;
  last_changed[pr] = ch;
  inertia[pr] = s_tot[k * F];
  const bool finished = ch == 0 || it >= max_iter;
  for (int c = 0; c < k; ++c) {
    const int cnt = counts_acc[pr * k + c];
    counts_acc[pr * k + c] = 0;
    counts[pr * k + c] = cnt;
    for (int j = 0; j < F; ++j) {
      const double s = s_tot[c * F + j];
      sums[(size_t)(pr * k + c) * F + j] = s;
      if (!finished && cnt > 0) centers[(size_t)(pr * k + c) * F + j] = s / (double)cnt;   // an empty cluster keeps its centre
    }
  }
  if (finished) {
    done[pr] = 1;
    atomicAdd(status, 1);
  }
}

template <int F, bool IOU>
__global__ __launch_bounds__(KM_POINTS) void kmeans_assign_kernel(const double* __restrict__ x, const signed char* __restrict__ problem, long long n,
                                                                  int P, int k, const double* __restrict__ centers, int* __restrict__ labels,
                                                                  double* __restrict__ dist) {
  __shared__ double s_cent[KM_MAX_P * KM_ASSIGN_MAX_K * KM_MAX_F];
  for (int e = threadIdx.x; e < P * k * F; e += KM_POINTS) s_cent[e] = centers[e];
  __syncthreads();
  const long long i = (long long)blockIdx.x * KM_POINTS + threadIdx.x;
  if (i >= n) return;
  int p = problem ? (int)problem[i] : 0;
  if (p < 0 || p >= P) {
    labels[i] = -1;
    dist[i] = 0.0;
    return;
  }
  double xi[F];
#pragma unroll
  for (int j = 0; j < F; ++j) xi[j] = x[i * F + j];
  double d;
  labels[i] = km_nearest<F, IOU>(xi, s_cent + (size_t)p * k * F, k, &d);
  dist[i] = d;
}

// errors[0]: points that take part (problem >= 0) with a non-finite feature or, under the IoU distance, a non-positive one;
// errors[1]: points whose problem index is >= P
template <bool IOU>
__global__ __launch_bounds__(KM_POINTS) void kmeans_check_kernel(const double* __restrict__ x, const signed char* __restrict__ problem, long long n,
                                                                 int P, int F, int* __restrict__ errors) {
  const long long i = (long long)blockIdx.x * KM_POINTS + threadIdx.x;
  if (i >= n) return;
  const int p = problem ? (int)problem[i] : 0;
  if (p < 0) return;
  if (p >= P) {
    atomicAdd(&errors[1], 1);
    return;
  }
  bool bad = false;
  for (int j = 0; j < F; ++j) {
    const double v = x[i * F + j];
    bad = bad || !(fabs(v) < __builtin_inf()) || (IOU && !(v > 0.0));
  }
  if (bad) atomicAdd(&errors[0], 1);
}

struct Workspace {
  double* part;
  unsigned char* labels8;
  int *counts_acc, *changed, *done;
  size_t bytes, ints_offset, ints_bytes, labels_offset, labels_bytes;
};

long long km_blocks(long long n) { return (n + KM_POINTS - 1) / KM_POINTS; }

Workspace carve(void* base, long long n, int P, int R, int k, int F) {
  Workspace w;
  const size_t part_bytes = (size_t)P * R * ((size_t)k * F + 1) * (size_t)km_blocks(n) * sizeof(double);
  w.labels_offset = part_bytes;
  w.labels_bytes = ((size_t)R * (size_t)n + 7) / 8 * 8;
  w.ints_offset = w.labels_offset + w.labels_bytes;
  w.ints_bytes = ((size_t)P * R * k + 2 * (size_t)P * R) * sizeof(int);
  w.bytes = w.ints_offset + w.ints_bytes;
  char* b = (char*)base;
  w.part = (double*)b;
  w.labels8 = (unsigned char*)(b + w.labels_offset);
  w.counts_acc = (int*)(b + w.ints_offset);
  w.changed = w.counts_acc + (size_t)P * R * k;
  w.done = w.changed + (size_t)P * R;
  return w;
}

bool sizes_ok(int64_t n, int P, int R, int k, int F, int max_k) {
  return n > 0 && n < (1ll << 31) && P > 0 && P <= KM_MAX_P && R > 0 && R <= KM_MAX_R && k > 0 && k <= max_k && F > 0 && F <= KM_MAX_F;
}

typedef void (*pass_fn)(const double*, const signed char*, long long, int, int, int, const double*, const int*, const int*, unsigned char*, double*,
                        long long, int*, int*);
typedef void (*assign_fn)(const double*, const signed char*, long long, int, int, const double*, int*, double*);

pass_fn pass_kernel(int F, int metric) {
  if (metric == MI355DET_KMEANS_IOU) return kmeans_pass_kernel<2, true>;
  switch (F) {
    case 1: return kmeans_pass_kernel<1, false>;
    case 2: return kmeans_pass_kernel<2, false>;
    case 3: return kmeans_pass_kernel<3, false>;
    default: return kmeans_pass_kernel<4, false>;
  }
}

assign_fn assign_kernel(int F, int metric) {
  if (metric == MI355DET_KMEANS_IOU) return kmeans_assign_kernel<2, true>;
  switch (F) {
    case 1: return kmeans_assign_kernel<1, false>;
    case 2: return kmeans_assign_kernel<2, false>;
    case 3: return kmeans_assign_kernel<3, false>;
    default: return kmeans_assign_kernel<4, false>;
  }
}

bool metric_ok(int metric, int F) { return metric == MI355DET_KMEANS_EUCLID || (metric == MI355DET_KMEANS_IOU && F == 2); }

}  // namespace

extern "C" {

int mi355det_kmeans_limit(int which) {
  switch (which) {
    case 0: return KM_MAX_P;
    case 1: return KM_MAX_R;
    case 2: return KM_MAX_K;
    case 3: return KM_MAX_F;
    case 4: return KM_ASSIGN_MAX_K;
    case 5: return KM_POINTS;
    default: return -1;
  }
}

int mi355det_box_features(const double* box_wh, const int32_t* image_index, const int32_t* image_size, int64_t n_annotations, int32_t n_images,
                          double* features, int8_t* band, int32_t* errors, void* stream) {
  const char* what = "box_features";
  if (n_annotations <= 0 || n_annotations >= (1ll << 31) || n_images <= 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (!box_wh || !image_index || !image_size || !features || !band || !errors) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  hipStream_t s = S(stream);
  if (hipMemsetAsync(errors, 0, sizeof(int32_t), s) != hipSuccess) return check_launch(what);
  hipLaunchKernelGGL(box_features_kernel, dim3((unsigned)((n_annotations + FEAT_THREADS - 1) / FEAT_THREADS)), dim3(FEAT_THREADS), 0, s, box_wh,
                     image_index, image_size, (long long)n_annotations, n_images, features, (signed char*)band, errors);
  return check_launch(what);
}

size_t mi355det_kmeans_workspace(int64_t n, int32_t problems, int32_t restarts, int32_t k, int32_t features) {
  if (!sizes_ok(n, problems, restarts, k, features, KM_MAX_K)) return 0;
  return carve(nullptr, n, problems, restarts, k, features).bytes;
}

int mi355det_kmeans_check(const double* x, const int8_t* problem, int64_t n, int32_t problems, int32_t features, int32_t metric, int32_t* errors,
                          void* stream) {
  const char* what = "kmeans_check";
  if (n <= 0 || n >= (1ll << 31) || problems <= 0 || problems > KM_MAX_P || features <= 0 || features > KM_MAX_F || !metric_ok(metric, features))
    return fail(MI355DET_EINVAL, "%s: bad arguments or limits exceeded", what);
  if (!x || !errors) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  hipStream_t s = S(stream);
  if (hipMemsetAsync(errors, 0, 2 * sizeof(int32_t), s) != hipSuccess) return check_launch(what);
  const dim3 grid((unsigned)km_blocks(n));
  if (metric == MI355DET_KMEANS_IOU)
    hipLaunchKernelGGL(kmeans_check_kernel<true>, grid, dim3(KM_POINTS), 0, s, x, (const signed char*)problem, (long long)n, problems, features, errors);
  else
    hipLaunchKernelGGL(kmeans_check_kernel<false>, grid, dim3(KM_POINTS), 0, s, x, (const signed char*)problem, (long long)n, problems, features, errors);
  return check_launch(what);
}

int mi355det_kmeans_begin(int64_t n, int32_t problems, int32_t restarts, int32_t k, int32_t features, int32_t* n_iter, int32_t* status,
                          void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "kmeans_begin";
  if (!sizes_ok(n, problems, restarts, k, features, KM_MAX_K)) return fail(MI355DET_EINVAL, "%s: bad arguments or limits exceeded", what);
  if (!n_iter || !status || !workspace) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  const Workspace w = carve(workspace, n, problems, restarts, k, features);
  if (workspace_bytes < w.bytes) return fail(MI355DET_EINVAL, "%s: workspace too small", what);
  hipStream_t s = S(stream);
  if (hipMemsetAsync(w.labels8, 0xFF, w.labels_bytes, s) != hipSuccess || hipMemsetAsync(w.counts_acc, 0, w.ints_bytes, s) != hipSuccess ||
      hipMemsetAsync(n_iter, 0, (size_t)problems * restarts * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess)
    return check_launch(what);
  return MI355DET_OK;
}

int mi355det_kmeans_passes(const double* x, const int8_t* problem, int64_t n, int32_t problems, int32_t restarts, int32_t k, int32_t features,
                           int32_t metric, int32_t max_iter, int32_t n_passes, double* centers, double* sums, int32_t* counts, double* inertia,
                           int32_t* n_iter, int32_t* changed, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "kmeans_passes";
  if (!sizes_ok(n, problems, restarts, k, features, KM_MAX_K) || !metric_ok(metric, features) || max_iter <= 0 || n_passes <= 0)
    return fail(MI355DET_EINVAL, "%s: bad arguments or limits exceeded", what);
  if (!x || !centers || !sums || !counts || !inertia || !n_iter || !changed || !status || !workspace)
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  const Workspace w = carve(workspace, n, problems, restarts, k, features);
  if (workspace_bytes < w.bytes) return fail(MI355DET_EINVAL, "%s: workspace too small", what);
  static DeviceOnce attr_done;
  attr_done.once([&] {
    const int lds = (int)pass_lds_bytes(KM_MAX_P, KM_MAX_R, KM_MAX_K, KM_MAX_F);
    for (int f = 1; f <= KM_MAX_F; ++f)
      (void)hipFuncSetAttribute((const void*)pass_kernel(f, MI355DET_KMEANS_EUCLID), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute((const void*)pass_kernel(2, MI355DET_KMEANS_IOU), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  hipStream_t s = S(stream);
  const long long nblocks = km_blocks(n);
  const size_t lds = pass_lds_bytes(problems, restarts, k, features);
  const pass_fn pass = pass_kernel(features, metric);
  for (int it = 0; it < n_passes; ++it) {
    hipLaunchKernelGGL(pass, dim3((unsigned)nblocks), dim3(KM_POINTS), lds, s, x, (const signed char*)problem, (long long)n, problems, restarts, k,
                       (const double*)centers, (const int*)w.done, (const int*)status, w.labels8, w.part, nblocks, w.counts_acc, w.changed);
    hipLaunchKernelGGL(kmeans_combine_kernel, dim3((unsigned)(problems * restarts)), dim3(KM_COMBINE_THREADS), 0, s, restarts, k, features, max_iter,
                       (const double*)w.part, nblocks, w.counts_acc, w.changed, w.done, status, centers, sums, counts, inertia, n_iter, changed);
  }
  return check_launch(what);
}

int mi355det_kmeans_assign(const double* x, const int8_t* problem, int64_t n, int32_t problems, int32_t k, int32_t features, int32_t metric,
                           const double* centers, int32_t* labels, double* distance, void* stream) {
  const char* what = "kmeans_assign";
  if (!sizes_ok(n, problems, 1, k, features, KM_ASSIGN_MAX_K) || !metric_ok(metric, features))
    return fail(MI355DET_EINVAL, "%s: bad arguments or limits exceeded", what);
  if (!x || !centers || !labels || !distance) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  hipLaunchKernelGGL(assign_kernel(features, metric), dim3((unsigned)km_blocks(n)), dim3(KM_POINTS), 0, S(stream), x, (const signed char*)problem,
                     (long long)n, problems, k, centers, labels, distance);
  return check_launch(what);
}

}  // extern "C"
