// Dataset statistics for TF-IDF class re-weighting (include/mi355det.h, "Dataset statistics"): the per-category instance and image counts of
// an annotation list, and the table of idf variants derived from them - what the reference's yolo/utilities/get_idf.py and the build branch
// of IDFTransformer (custom.py:176-247) compute with one bincount, one coo_matrix and one vstack per image.
//
// category_freq_kernel: one thread per annotation, grid-stride.  instance_freq[c] counts the annotation; img_freq[c] counts it only if its
// atomic OR was the one that set bit (image, c) of a bitmap [n_images, ceil(n_categories / 32)], so every distinct pair counts once whatever
// the order.  While both histograms fit the LDS budget (n_categories <= LDS_CATS) a workgroup counts into LDS and adds its non-zero bins to
// the global rows at the end: COCO's `person` row takes 262 465 increments, which as global atomics would all queue on one address.  Inside
// a wave the lanes that share the first active lane's category are counted by one LDS add of their number (the hot category of a
// long-tailed set is that lane's category more often than any other); the other lanes add for themselves.  Beyond the budget the same
// thread mapping adds to the global rows directly.  Integer atomics only: exact, order-independent, bit-reproducible.
//
// idf_table_kernel: one thread per present category; N = sum of instance_freq is summed per workgroup in integers, then csrc/idf_formulas.h.
// Compiled with -ffp-contract=off: the quotients and the ndtri polynomials are numpy's and Cephes' operation for operation.
#include "common.h"
#include "idf_formulas.h"

using namespace mi355;

namespace {

constexpr int FREQ_THREADS = 256;
constexpr int LDS_CATS = 4096;          // 2 histograms x 4096 x 4 B = 32 KB of the CU's 160 KB: five workgroups per CU
constexpr int FREQ_PER_THREAD = 16;     // annotations per thread the grid is sized for; the loop strides over the rest
constexpr int TABLE_THREADS = 256;

template <bool USE_LDS>
__global__ __launch_bounds__(FREQ_THREADS) void category_freq_kernel(const int* __restrict__ image_index, const int* __restrict__ category_index,
                                                                     long long n_ann, int n_images, int n_cats, int words,
                                                                     unsigned* __restrict__ bitmap, int* __restrict__ instance_freq,
                                                                     int* __restrict__ img_freq, int* __restrict__ errors) {
  extern __shared__ int s_hist[];                           // [2, n_cats] with USE_LDS: instances, then images
  int* inst = USE_LDS ? s_hist : instance_freq;
  int* imgs = USE_LDS ? s_hist + n_cats : img_freq;
  if (USE_LDS) {
    for (int c = threadIdx.x; c < 2 * n_cats; c += FREQ_THREADS) s_hist[c] = 0;
    __syncthreads();
  }
  const long long stride = (long long)gridDim.x * FREQ_THREADS;
  // whole waves enter each round (the bound is rounded up to the wave), so the ballot below sees every lane of the wave
  const long long rounded = (n_ann + WAVE - 1) / WAVE * WAVE;
  for (long long i = (long long)blockIdx.x * FREQ_THREADS + threadIdx.x; i < rounded; i += stride) {
    int im = -1, c = -1;
    bool ok = false;
    if (i < n_ann) {
      im = image_index[i];
      c = category_index[i];
      ok = im >= 0 && im < n_images && c >= 0 && c < n_cats;
      if (!ok) atomicAdd(errors, 1);
    }
    if (USE_LDS) {
      const unsigned long long live = __ballot(ok);
      if (live) {
        const int leader = __ffsll((long long)live) - 1;
        const int c0 = __shfl(c, leader, WAVE);
        const unsigned long long same = __ballot(ok && c == c0);
        if ((int)(threadIdx.x & (WAVE - 1)) == leader) atomicAdd(&inst[c0], __popcll(same));
        else if (ok && c != c0) atomicAdd(&inst[c], 1);
      }
    } else if (ok) {
      atomicAdd(&inst[c], 1);
    }
    if (ok) {
      const unsigned bit = 1u << (c & 31);
      const unsigned old = atomicOr(&bitmap[(size_t)im * words + (c >> 5)], bit);
      if (!(old & bit)) atomicAdd(&imgs[c], 1);             // this thread set the bit: the image's first annotation of c
    }
  }
  if (USE_LDS) {
    __syncthreads();
    for (int c = threadIdx.x; c < n_cats; c += FREQ_THREADS) {
      const int a = s_hist[c], b = s_hist[n_cats + c];
      if (a) atomicAdd(&instance_freq[c], a);
      if (b) atomicAdd(&img_freq[c], b);
    }
  }
}

__global__ __launch_bounds__(TABLE_THREADS) void idf_table_kernel(const int* __restrict__ img_freq, const int* __restrict__ instance_freq, int R,
                                                                  long long n_images, double* __restrict__ table) {
  __shared__ unsigned long long s_total;
  if (threadIdx.x == 0) s_total = 0;
  __syncthreads();
  unsigned long long part = 0;
  for (int r = threadIdx.x; r < R; r += TABLE_THREADS) part += (unsigned long long)max(instance_freq[r], 0);
  if (part) atomicAdd(&s_total, part);
  __syncthreads();
  const int r = blockIdx.x * TABLE_THREADS + threadIdx.x;
  if (r >= R) return;
  double col[14];
  idf_columns((double)n_images, (double)img_freq[r], col);
  idf_columns((double)s_total, (double)instance_freq[r], col + 7);
#pragma unroll
  for (int k = 0; k < 14; ++k) table[(size_t)k * R + r] = col[k];
}

size_t bitmap_bytes(int n_images, int n_cats) { return (size_t)n_images * (size_t)((n_cats + 31) / 32) * sizeof(unsigned); }

}  // namespace

extern "C" {

size_t mi355det_category_frequencies_workspace(int32_t n_images, int32_t n_categories) {
  if (n_images <= 0 || n_categories <= 0) return 0;
  return bitmap_bytes(n_images, n_categories);
}

int mi355det_category_frequencies_lds_categories(void) { return LDS_CATS; }

int mi355det_category_frequencies(const int32_t* image_index, const int32_t* category_index, int64_t n_annotations, int32_t n_images,
                                  int32_t n_categories, int32_t* instance_freq, int32_t* img_freq, int32_t* errors, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  const char* what = "category_frequencies";
  if (n_annotations < 0 || n_annotations >= (1ll << 31) || n_images <= 0 || n_categories <= 0)
    return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (!instance_freq || !img_freq || !errors || !workspace || (n_annotations > 0 && (!image_index || !category_index)))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  const size_t need = bitmap_bytes(n_images, n_categories);
  if (workspace_bytes < need) return fail(MI355DET_EINVAL, "%s: workspace too small", what);
  hipStream_t s = S(stream);
  if (hipMemsetAsync(workspace, 0, need, s) != hipSuccess || hipMemsetAsync(instance_freq, 0, (size_t)n_categories * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(img_freq, 0, (size_t)n_categories * sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(errors, 0, sizeof(int32_t), s) != hipSuccess)
    return check_launch(what);
  if (n_annotations == 0) return MI355DET_OK;
  const int words = (n_categories + 31) / 32;
  const long long per_block = (long long)FREQ_THREADS * FREQ_PER_THREAD;
  long long blocks = (n_annotations + per_block - 1) / per_block;
  if (blocks > 2048) blocks = 2048;
  if (n_categories <= LDS_CATS)
    hipLaunchKernelGGL(category_freq_kernel<true>, dim3((unsigned)blocks), dim3(FREQ_THREADS), (size_t)2 * n_categories * sizeof(int), s, image_index,
                       category_index, (long long)n_annotations, n_images, n_categories, words, (unsigned*)workspace, instance_freq, img_freq,
                       errors);
  else
    hipLaunchKernelGGL(category_freq_kernel<false>, dim3((unsigned)blocks), dim3(FREQ_THREADS), 0, s, image_index, category_index,
                       (long long)n_annotations, n_images, n_categories, words, (unsigned*)workspace, instance_freq, img_freq, errors);
  return check_launch(what);
}

int mi355det_idf_table(const int32_t* img_freq, const int32_t* instance_freq, int32_t n_rows, int64_t n_images, double* table, void* stream) {
  const char* what = "idf_table";
  if (n_rows <= 0 || n_images <= 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (!img_freq || !instance_freq || !table) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  hipLaunchKernelGGL(idf_table_kernel, dim3((unsigned)((n_rows + TABLE_THREADS - 1) / TABLE_THREADS)), dim3(TABLE_THREADS), 0, S(stream), img_freq,
                     instance_freq, n_rows, (long long)n_images, table);
  return check_launch(what);
}

}  // extern "C"
