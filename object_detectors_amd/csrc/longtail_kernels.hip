// Long-tail baselines of the RoI box classifier (include/mi355det.h, "Long-tail baselines"): Seesaw loss (Wang et al., CVPR 2021) and
// Equalization loss v1 (Tan et al., CVPR 2020) as fused forward + gradient kernels beside the five reference losses of frcnn_kernels.hip,
// the label histogram that is Seesaw's state, and the repeat factors of repeat-factor sampling (Gupta et al., LVIS 2019).  The rules are
// restated from the papers; nothing here is compared against mmdetection or detectron2.
//
//   x = class_scale[k] * logits (the tf-idf row); gradients are returned w.r.t. the UNSCALED logits; the box half is csrc/frcnn_rows.h.
//   seesaw  N_c = max(counts[c], 1), s = softmax(x) (no gradient);  for a row labelled y and every column j != y
//             log M_j = p (log N_j - log N_y) if N_j < N_y, else 0;   log C_j = q (log s_j - log max(s_y, eps)) if that is > 0, else 0
//           x'_j = x_j + log M_j + log C_j, x'_y = x_y;   loss = mean_rows (logsumexp(x') - x'_y);   grad_j = scale_j (softmax(x')_j - [j = y]) / n
//   eql     t_j = [j = y and j != 0], w_j = 1 - [y > 0] tail_j (1 - t_j);   loss = sum_rows sum_j w_j BCEWithLogits(x_j, t_j) / n;
//           grad_j = scale_j w_j (sigmoid(x_j) - t_j) / n
//
// Like frcnn_kernels.hip: one wave per row, lanes stride over the classes, row reductions by wave_max / wave_sum, per-row losses in a
// workspace summed by one workgroup in a fixed order.  Seesaw reads the row three times (L1/L2 hits after the first): max and sum-exp of
// x in one sweep (a running maximum per lane, merged across the wave), the same of x', then the gradient.  log N_c is computed once per
// call into the workspace, not once per row.  The only atomics are the integer adds of the histogram and the 64-bit integer maximum of
// the repeat factors: every output is the same from run to run.
//
// A label outside [0, k) is never used as an index: that row's class loss is NaN, its gradients are 0, it adds nothing to counts.
#include "common.h"
#include "frcnn_rows.h"

using namespace mi355;

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float bce_logits(float x, float t) { return fmaxf(x, 0.0f) - x * t + log1pf(expf(-fabsf(x))); }

// one sweep of max and sum-exp: (m, s) with s = sum exp(v - m) over the values fed so far
struct RunLse {
  float m = -INFINITY, s = 0.0f;
  __device__ __forceinline__ void feed(float v) {
    if (v > m) {
      s = s * expf(m - v) + 1.0f;       // m = -inf on the first value: s = 0 * 0 + 1
      m = v;
    } else {
      s += expf(v - m);
    }
  }
  // merge the 64 lanes; a lane that saw no class (k < 64) holds (-inf, 0) and adds 0 * exp(-inf) = 0
  __device__ __forceinline__ void reduce() {
    const float mx = wave_max(m);
    s = wave_sum(s * expf(m - mx));
    m = mx;
  }
};

constexpr int HIST_THREADS = 256;

// counts[labels[i]] += 1.  Whole waves enter each round so that the ballots see every lane; the lanes that share the first live lane's
// label (background, for three RoIs in four) are counted by one add of their number, the others add for themselves.
__global__ __launch_bounds__(HIST_THREADS) void label_histogram_kernel(const long long* __restrict__ labels, int n, int k,
                                                                       unsigned long long* __restrict__ counts) {
  const int stride = gridDim.x * HIST_THREADS;
  const int rounded = (n + WAVE - 1) / WAVE * WAVE;
  for (int i = blockIdx.x * HIST_THREADS + threadIdx.x; i < rounded; i += stride) {
    long long y = -1;
    if (i < n) y = labels[i];
    const bool ok = y >= 0 && y < (long long)k;
    const unsigned long long live = __ballot(ok);
    if (!live) continue;
    const int leader = __ffsll((long long)live) - 1;
    const int c = ok ? (int)y : -1;
    const int c0 = __shfl(c, leader, WAVE);
    const unsigned long long same = __ballot(ok && c == c0);
    if ((int)(threadIdx.x & (WAVE - 1)) == leader) atomicAdd(&counts[c0], (unsigned long long)__popcll(same));
    else if (ok && c != c0) atomicAdd(&counts[c], 1ull);
  }
}

__global__ __launch_bounds__(256) void log_counts_kernel(const long long* __restrict__ counts, int k, float* __restrict__ log_n) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < k) log_n[c] = logf((float)max(counts[c], 1ll));
}

// TYPE 0 seesaw, 1 eql
template <int TYPE>
__global__ __launch_bounds__(256) void longtail_loss_kernel(const float* __restrict__ logits, const float* __restrict__ breg,
                                                             const long long* __restrict__ labels, const float* __restrict__ tgt,
                                                             const float* __restrict__ cscale, const float* __restrict__ log_n,
                                                             const unsigned char* __restrict__ tail, float p, float q, float log_eps, int n, int k,
                                                             float* __restrict__ row_cls, float* __restrict__ row_box,
                                                             float* __restrict__ glogits, float* __restrict__ gbox) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const long long yl = labels[row];
  const bool ok = yl >= 0 && yl < (long long)k;
  const int y = ok ? (int)yl : -1;            // -1: compared, never an index
  const float* xr = logits + (size_t)row * k;
  float* gr = glogits ? glogits + (size_t)row * k : nullptr;
  const float inv_n = 1.0f / (float)n;
  float loss;
  if (!ok) {
    loss = NAN;
    if (gr)
      for (int c = lane; c < k; c += 64) gr[c] = 0.0f;
  } else if (TYPE == 0) {
    RunLse a;
    for (int c = lane; c < k; c += 64) a.feed(xr[c] * (cscale ? cscale[c] : 1.0f));
    a.reduce();
    const float lse = a.m + logf(a.s);
    const float xy = xr[y] * (cscale ? cscale[y] : 1.0f);
    const float ls_ref = fmaxf(xy - lse, log_eps);            // log max(s_y, eps)
    const float ln_y = log_n[y];
    // x'_c; M and C are 1 at c == y
    auto shifted = [&](int c) {
      const float x = xr[c] * (cscale ? cscale[c] : 1.0f);
      if (c == y) return x;
      const float dn = log_n[c] - ln_y;
      const float dr = (x - lse) - ls_ref;
      return x + ((dn < 0.0f ? p * dn : 0.0f) + (dr > 0.0f ? q * dr : 0.0f));
    };
    RunLse b;
    for (int c = lane; c < k; c += 64) b.feed(shifted(c));
    b.reduce();
    loss = ((b.m + logf(b.s)) - xy) * inv_n;
    if (gr) {
      const float inv_se = 1.0f / b.s;
      for (int c = lane; c < k; c += 64) {
        const float pr = expf(shifted(c) - b.m) * inv_se;
        gr[c] = inv_n * (pr - (c == y ? 1.0f : 0.0f)) * (cscale ? cscale[c] : 1.0f);
      }
    }
  } else {
    loss = 0.0f;
    for (int c = lane; c < k; c += 64) {
      const float s = cscale ? cscale[c] : 1.0f;
      const float x = xr[c] * s;
      const float t = (c == y && c != 0) ? 1.0f : 0.0f;
      const float w = (y > 0 && c != y && tail[c]) ? 0.0f : 1.0f;     // a foreground proposal spares the tail categories its negative gradient
      loss += w * bce_logits(x, t);
      if (gr) gr[c] = w * (sigmoidf_(x) - t) * inv_n * s;
    }
    loss = wave_sum(loss) * inv_n;
  }
  const float lb = frcnn_box_row(breg, tgt, gbox, row, k, y, lane, inv_n);
  if (lane == 0) {
    row_cls[row] = loss;
    row_box[row] = lb;
  }
}

__global__ __launch_bounds__(256) void longtail_finalize_kernel(const float* __restrict__ row_cls, const float* __restrict__ row_box, int n,
                                                                 float* __restrict__ losses) {
  float c, b;
  frcnn_sum_rows(row_cls, row_box, n, c, b);
  if (threadIdx.x == 0) {
    losses[0] = c;
    losses[1] = b;
  }
}

constexpr int RF_THREADS = 256;

// r_image[im] = max(r_image[im], r_c) with r_c = max(1, sqrt(t / (img_freq[c] / n_images))) in float64.  Non-negative doubles order as their
// bit patterns do, so the integer maximum is the floating-point one, whatever the order of the annotations.
__global__ __launch_bounds__(RF_THREADS) void repeat_factors_kernel(const int* __restrict__ image_index, const int* __restrict__ category_index,
                                                                    long long n_ann, const int* __restrict__ img_freq, int n_images, int n_cats,
                                                                    double t, unsigned long long* __restrict__ r_image, int* __restrict__ errors) {
  const long long stride = (long long)gridDim.x * RF_THREADS;
  for (long long i = (long long)blockIdx.x * RF_THREADS + threadIdx.x; i < n_ann; i += stride) {
    const int im = image_index[i], c = category_index[i];
    if (im < 0 || im >= n_images || c < 0 || c >= n_cats) {
      atomicAdd(errors, 1);
      continue;
    }
    const int df = img_freq[c];
    if (df <= 0) continue;                  // a frequency table that does not belong to these annotations: no factor to read
    const double f = (double)df / (double)n_images;
    const double r = fmax(1.0, sqrt(t / f));
    atomicMax(&r_image[im], (unsigned long long)__double_as_longlong(r));
  }
}

}  // namespace

extern "C" {

int mi355det_label_histogram(const int64_t* labels, int32_t n, int32_t k, int64_t* counts, void* stream) {
  const char* what = "label_histogram";
  if (n < 0 || k < 1) return fail(MI355DET_EINVAL, "%s: need n >= 0 labels and k >= 1 classes", what);
  if (!counts || (n > 0 && !labels)) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if (n == 0) return MI355DET_OK;
  const int blocks = min(1024, (n + HIST_THREADS - 1) / HIST_THREADS);
  hipLaunchKernelGGL(label_histogram_kernel, dim3(blocks), dim3(HIST_THREADS), 0, S(stream), (const long long*)labels, n, k,
                     (unsigned long long*)counts);
  return check_launch(what);
}

size_t mi355det_fastrcnn_loss_longtail_workspace(int32_t n, int32_t k) {
  return ((size_t)2 * (n > 0 ? n : 0) + (size_t)(k > 0 ? k : 0) + 8) * sizeof(float);
}

int mi355det_fastrcnn_loss_longtail(const float* class_logits, const float* box_regression, const int64_t* labels, const float* regression_targets,
                                    const float* class_scale, int32_t n, int32_t k, int32_t loss_type, int64_t* counts, const uint8_t* tail,
                                    float p, float q, float eps, int32_t update_counts, float* losses, float* grad_logits, float* grad_box,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "fastrcnn_loss_longtail";
  if (n <= 0 || k <= 1) return fail(MI355DET_EINVAL, "%s: need n >= 1 rows and k >= 2 classes", what);
  if (loss_type < 0 || loss_type > 1) return fail(MI355DET_EINVAL, "%s: loss_type must be 0 (seesaw) or 1 (eql)", what);
  if (!class_logits || !box_regression || !labels || !regression_targets || !losses || !workspace)
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if (loss_type == 0 && !counts) return fail(MI355DET_EINVAL, "%s: seesaw needs the class counts", what);
  if (loss_type == 1 && !tail) return fail(MI355DET_EINVAL, "%s: eql needs the tail mask", what);
  if (!(p >= 0.0f) || !(q >= 0.0f) || !std::isfinite(p) || !std::isfinite(q))
    return fail(MI355DET_EINVAL, "%s: p and q must be finite and >= 0", what);
  if (!(eps > 0.0f && eps <= 1.0f)) return fail(MI355DET_EINVAL, "%s: eps must lie in (0, 1]", what);
  if (workspace_bytes < mi355det_fastrcnn_loss_longtail_workspace(n, k)) return fail(MI355DET_EWORKSPACE, "%s: workspace too small", what);
  float* row_cls = (float*)workspace;
  float* row_box = row_cls + n;
  float* log_n = row_box + n;
  const long long* lab = (const long long*)labels;
  const int blocks = (n + 3) / 4;
  hipStream_t st = S(stream);
  if (loss_type == 0) {
    if (update_counts) {                    // before the loss reads them
      const int st_hist = mi355det_label_histogram(labels, n, k, counts, stream);
      if (st_hist != MI355DET_OK) return st_hist;
    }
    hipLaunchKernelGGL(log_counts_kernel, dim3((k + 255) / 256), dim3(256), 0, st, (const long long*)counts, k, log_n);
    hipLaunchKernelGGL(longtail_loss_kernel<0>, dim3(blocks), dim3(256), 0, st, class_logits, box_regression, lab, regression_targets, class_scale,
                       log_n, tail, p, q, logf(eps), n, k, row_cls, row_box, grad_logits, grad_box);
  } else {
    hipLaunchKernelGGL(longtail_loss_kernel<1>, dim3(blocks), dim3(256), 0, st, class_logits, box_regression, lab, regression_targets, class_scale,
                       log_n, tail, p, q, logf(eps), n, k, row_cls, row_box, grad_logits, grad_box);
  }
  hipLaunchKernelGGL(longtail_finalize_kernel, dim3(1), dim3(256), 0, st, row_cls, row_box, n, losses);
  return check_launch(what);
}

int mi355det_repeat_factors(const int32_t* image_index, const int32_t* category_index, int64_t n_annotations, const int32_t* img_freq,
                            int32_t n_images, int32_t n_categories, double t, double* r_image, int32_t* errors, void* stream) {
  const char* what = "repeat_factors";
  if (n_annotations < 0 || n_annotations >= (1ll << 31) || n_images <= 0 || n_categories <= 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (!(t > 0.0) || !std::isfinite(t)) return fail(MI355DET_EINVAL, "%s: the threshold t must be finite and > 0", what);
  if (!img_freq || !r_image || !errors || (n_annotations > 0 && (!image_index || !category_index)))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  hipStream_t s = S(stream);
  if (hipMemsetAsync(errors, 0, sizeof(int32_t), s) != hipSuccess) return check_launch(what);
  if (n_annotations == 0) return MI355DET_OK;
  const long long blocks = min((long long)2048, (long long)((n_annotations + RF_THREADS - 1) / RF_THREADS));
  hipLaunchKernelGGL(repeat_factors_kernel, dim3((unsigned)blocks), dim3(RF_THREADS), 0, s, image_index, category_index, (long long)n_annotations,
                     img_freq, n_images, n_categories, t, (unsigned long long*)r_image, errors);
  return check_launch(what);
}

}  // extern "C"
