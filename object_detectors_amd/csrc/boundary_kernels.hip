// Mask boundaries as COCO run lengths (include/mi355det.h, "Mask boundaries as run lengths"): what the boundary-IoU APIs get from decode +
// copyMakeBorder + cv2.erode(3x3, iterations = d) + subtract + encode, made on the device from the run lengths, for `iou_type="boundary"`.
//
//   eroded(x, y) = 1 iff the whole (2d+1) x (2d+1) window centred on (x, y) lies inside the image and every pixel of it is set
//   boundary     = mask & ~eroded
//
// All work stays inside the mask's tight box: outside it the mask is 0, and the image border counts as 0 too, so "the window leaves the box"
// and "the window meets a 0" are the same event.  A box of bw x bh pixels is held as bit planes of nw = ceil(bh / 64) words per column, 64
// rows per word, word (x, j) at j * bw + x (adjacent columns adjacent, so every pass but the column walk of phase B reads and writes rows of
// words).  One block per mask, four phases with a block barrier between them; a mask's planes live in a global scratch slice of its own
// (three planes and the scanned counts), sized by the host from the boxes and handed out in chunks under a byte budget, so they stay in L2:
//   A  pos[i] = counts[0] + .. + counts[i] (block scan): run i covers the pixels pos[i-1] .. pos[i] - 1 in column-major order.
//   B  thread = column: a binary search finds the column's first run, then one walk over its runs of ones (runs that go on across a column
//      boundary are clipped to the column; runs separated by an empty run of zeros are joined) writes two planes: M, the mask, and V, the
//      mask eroded vertically - a run [a, b) of a column becomes [a + d, b - d), or nothing if b - a <= 2d.  No bitmap is ever decoded.
//   C  E(x) = AND of V(x - d .. x + d), 0 where the window leaves the box, by doubling: P1 = V, P2k(x) = Pk(x) & Pk(x + k), up to the largest
//      power of two p <= 2d + 1, then E(x) = Pp(x - d) & Pp(x + d - p + 1): floor(log2(2d + 1)) + 1 passes, not 2d + 1 reads.  B = M & ~E.
//      Where 2d + 1 exceeds the box's width or height E is 0 and B is M: no pass at all.
//   D  thread = column, 64 or 256 columns per step: a column's transitions are popcount(B ^ (B << 1 | carry)), the carry from the word above
//      and, at row 0 of the image, from the last row of the column before (pycocotools' column-major rule: csrc/rle_kernels.hip).  A block
//      scan gives each column its first index among the mask's transitions and the position of the transition before it; the emit pass then
//      walks the column's words once more and writes each gap.  The count pass stops after the scan's total.
// The count pass and the emit pass both run A - D (the planes of 5.9 million masks are never held at once); between them the host reads the
// run offsets once.  Small boxes (at most SMALL_WORDS words a plane) get a block of one wavefront, the others 256 threads: two launches over
// the same chunk, each block leaving at once if its mask is of the other class.
// Integers only, no atomics, one writer per element, 64-bit offsets: the same bits every run.
#include "rle_protocol.h"

#include <limits.h>

using namespace mi355;

namespace {

typedef unsigned long long u64;

constexpr int GEOM = 7;                                 // h, w, d, box x, y, w, h
constexpr int SMALL_WORDS = 512, SMALL_THREADS = WAVE, LARGE_THREADS = 256;

struct Geom {
  int h, w, d, bx, by, bw, bh;
};

// what one mask needs of the workspace: three planes, then its scanned counts (an even number of int32, so every slice stays 8-byte aligned)
inline long long plane_words(int bw, int bh) { return (long long)bw * ((bh + 63) / 64); }
inline long long slice_bytes(long long m, int bw, int bh) { return 8 * 3 * plane_words(bw, bh) + 4 * ((m + 1) & ~1ll); }

struct Args {
  const int* counts;
  const long long* runs;
  const long long* index;                                // nullable: mask k reads the counts of mask index[k]
  const int* geom;
  const long long* slices;                               // byte offset of mask k's scratch slice in the workspace
  long long first;
  char* ws;
  long long* num_runs;                                   // count: [n]
  const long long* run_offsets;                          // emit: [n + 1]
  int* out;
  long long capacity;
  long long* area;
  int* bbox;
};

__device__ __forceinline__ u64 bits(int lo, int hi) {    // rows lo .. hi - 1 of a word, 0 <= lo < hi <= 64
  return (hi >= 64 ? ~0ull : (1ull << hi) - 1) & ~((1ull << lo) - 1);
}

// the transitions of column x (0 .. bw; column bw is the one right of the box) in pixel order: f(position) for each
template <class F>
__device__ __forceinline__ void walk_column(const u64* B, const Geom& g, int nw, int x, F&& f) {
  const bool full = g.by + g.bh == g.h;                  // the box reaches the last row: a run can go on into the next column
  const int rem = g.bh - 64 * (nw - 1);                  // rows of a column's last word, 1 .. 64
  const bool prev = full && x > 0 && ((B[(size_t)(nw - 1) * g.bw + x - 1] >> (rem - 1)) & 1);
  const int base = (g.bx + x) * g.h;                     // < 2^31: the entry points refuse h*w >= 2^31
  if (x >= g.bw) {
    if (prev && g.bx + g.bw < g.w) f(base);
    return;
  }
  u64 carry = prev;
  if (g.by > 0) {                                        // rows above the box are 0
    if (prev) f(base);
    carry = 0;
  }
  u64 w = 0;
  for (int j = 0; j < nw; ++j) {
    w = B[(size_t)j * g.bw + x];
    u64 t = w ^ ((w << 1) | carry);
    if (j == nw - 1 && rem < 64) t &= (1ull << rem) - 1;
    carry = w >> 63;
    const int row = base + g.by + 64 * j;
    while (t) {
      f(row + __builtin_ctzll(t));
      t &= t - 1;
    }
  }
  if (!full && ((w >> (rem - 1)) & 1)) f(base + g.by + g.bh);          // the row below the box is 0
}

template <bool EMIT>
__global__ __launch_bounds__(LARGE_THREADS) void boundary_kernel(Args A, int small) {
  __shared__ int s_sum[LARGE_THREADS], s_max[LARGE_THREADS];
  __shared__ long long s_area[LARGE_THREADS];
  const int NT = blockDim.x, t = threadIdx.x;
  const long long k = A.first + blockIdx.x;
  Geom g;
  {
    const int* p = A.geom + GEOM * k;
    g = Geom{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
  }
  const bool none = g.bw <= 0 || g.bh <= 0;
  const int nw = (g.bh + 63) / 64;
  const int words = none ? 0 : g.bw * nw;                // <= w * ceil(h / 64) < 2^31
  if ((words <= SMALL_WORDS) != (small != 0)) return;
  const long long out0 = EMIT ? A.run_offsets[k] : 0, out1 = EMIT ? A.run_offsets[k + 1] : 0;
  auto put = [&](long long i, int v) {
    const long long at = out0 + i;
    if (at >= 0 && at < out1 && at < A.capacity) A.out[at] = v;
  };
  if (none) {                                            // the empty mask: one count
    if (t == 0) {
      if (!EMIT) {
        A.num_runs[k] = 1;
      } else {
        put(0, g.h * g.w);
        if (A.area) A.area[k] = 0;
        if (A.bbox)
          for (int j = 0; j < 4; ++j) A.bbox[4 * k + j] = 0;
      }
    }
    return;
  }
  const long long src = A.index ? A.index[k] : k;
  const int* c = A.counts + A.runs[src];
  const int m = (int)(A.runs[src + 1] - A.runs[src]);    // <= h*w + 1: checked on the host
  u64* M = (u64*)(A.ws + A.slices[k]);
  u64* V = M + words;
  u64* P = V + words;
  int* pos = (int*)(P + words);

  // ---- A: the runs' ends
  unsigned carry = 0;
  for (int base = 0; base < m; base += NT) {
    const int i = base + t;
    const unsigned v = i < m ? (unsigned)c[i] : 0u;
    s_sum[t] = (int)v;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {
      const unsigned a = t >= o ? (unsigned)s_sum[t - o] : 0u;
      __syncthreads();
      s_sum[t] = (int)((unsigned)s_sum[t] + a);
      __syncthreads();
    }
    if (i < m) pos[i] = (int)(carry + (unsigned)s_sum[t]);
    carry += (unsigned)s_sum[NT - 1];
    __syncthreads();
  }

  // ---- B: the planes M and V, a column per thread
  const long long d = g.d;
  for (int x = t; x < g.bw; x += NT) {
    const long long cs = (long long)(g.bx + x) * g.h, ce = cs + g.h;
    int lo = 0, hi = m;
    while (lo < hi) {                                    // the first run that ends behind the column's first pixel
      const int mid = (lo + hi) >> 1;
      if (pos[mid] > cs) hi = mid; else lo = mid + 1;
    }
    int i = lo | 1;                                      // the next run of ones
    long long a = 0, b = 0;                              // the current run of ones of the column, rows [a, b) of the image
    bool have = false, more = true;
    for (int j = 0; j < nw; ++j) {
      const long long wlo = g.by + 64 * j, whi = min(wlo + 64, (long long)(g.by + g.bh));
      u64 mw = 0, vw = 0;
      while (more) {
        if (!have) {
          long long s = 0, e = 0;
          while (i < m) {
            if (pos[i - 1] >= ce) {
              i = m;
              break;
            }
            s = max((long long)pos[i - 1], cs);
            e = min((long long)pos[i], ce);
            if (e > s) break;
            i += 2;
          }
          if (i >= m) {
            more = false;
            break;
          }
          while (i + 2 < m && pos[i + 1] == pos[i] && pos[i] < ce) {       // an empty run of zeros: the next run of ones joins this one
            i += 2;
            e = max(e, min((long long)pos[i], ce));
          }
          i += 2;
          a = s - cs;
          b = e - cs;
          have = true;
        }
        if (a >= whi) break;
        long long l = max(a, wlo), r = min(b, whi);
        if (r > l) mw |= bits((int)(l - wlo), (int)(r - wlo));
        if (b - a > 2 * d) {
          l = max(a + d, wlo);
          r = min(b - d, whi);
          if (r > l) vw |= bits((int)(l - wlo), (int)(r - wlo));
        }
        if (b > whi) break;                              // the run goes on into the next word
        have = false;
      }
      M[(size_t)j * g.bw + x] = mw;
      V[(size_t)j * g.bw + x] = vw;
    }
  }
  __syncthreads();

  // ---- C: the horizontal erosion by doubling, then B = M & ~E
  const u64* B = M;
  if (2 * d + 1 <= g.bw && 2 * d + 1 <= g.bh) {
    const int di = (int)d, win = 2 * di + 1;
    u64 *cur = V, *other = P;
    int p = 1;
    while (2 * p <= win) {
      for (int j = 0; j < nw; ++j)
        for (int x = t; x < g.bw; x += NT) {
          const size_t at = (size_t)j * g.bw + x;
          other[at] = x + p < g.bw ? cur[at] & cur[at + p] : 0ull;
        }
      __syncthreads();
      u64* sw = cur;
      cur = other;
      other = sw;
      p <<= 1;
    }
    for (int j = 0; j < nw; ++j)
      for (int x = t; x < g.bw; x += NT) {
        const size_t at = (size_t)j * g.bw + x;
        const u64 e = (x >= di && x + di < g.bw) ? cur[at - di] & cur[at + di - p + 1] : 0ull;
        other[at] = M[at] & ~e;
      }
    __syncthreads();
    B = other;
  }

  // ---- D: transitions per column, their scan, and (EMIT) the counts
  int carry_sum = 0, carry_max = 0;
  long long area = 0;
  int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
  for (int base = 0; base <= g.bw; base += NT) {
    const int x = base + t;
    int n = 0, last = 0;
    if (x <= g.bw)
      walk_column(B, g, nw, x, [&](int at) {
        ++n;
        last = at;
      });
    s_sum[t] = n;
    s_max[t] = last;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {                   // inclusive scans: sum of the transitions, max of the last positions
      const int a = t >= o ? s_sum[t - o] : 0, b = t >= o ? s_max[t - o] : 0;
      __syncthreads();
      s_sum[t] += a;
      s_max[t] = max(s_max[t], b);
      __syncthreads();
    }
    if (EMIT && x <= g.bw) {
      long long i = carry_sum + s_sum[t] - n;
      int before = max(carry_max, t > 0 ? s_max[t - 1] : 0);            // positions grow with x: this is the transition before the column
      walk_column(B, g, nw, x, [&](int at) {
        put(i, at - before);
        before = at;
        ++i;
      });
      if (x < g.bw) {                                    // the boundary's set pixels and their rows
        int ns = 0, y0 = INT_MAX, y1 = -1;
        for (int j = 0; j < nw; ++j) {
          const u64 w = B[(size_t)j * g.bw + x];
          if (w) {
            ns += __popcll(w);
            if (y0 == INT_MAX) y0 = 64 * j + __builtin_ctzll(w);
            y1 = 64 * j + 63 - __builtin_clzll(w);
          }
        }
        if (ns > 0) {
          area += ns;
          xmin = min(xmin, x);
          xmax = max(xmax, x);
          ymin = min(ymin, y0);
          ymax = max(ymax, y1);
        }
      }
    }
    carry_sum += s_sum[NT - 1];
    carry_max = max(carry_max, s_max[NT - 1]);
    __syncthreads();
  }
  if (!EMIT) {
    if (t == 0) A.num_runs[k] = (long long)carry_sum + 1;
    return;
  }
  // the boundary's area and tight box: integer tree reductions (order-free, so exact)
  s_area[t] = area;
  s_sum[t] = xmin;
  s_max[t] = xmax;
  __syncthreads();
  for (int s = NT >> 1; s > 0; s >>= 1) {
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
  for (int s = NT >> 1; s > 0; s >>= 1) {
    if (t < s) {
      s_sum[t] = min(s_sum[t], s_sum[t + s]);
      s_max[t] = max(s_max[t], s_max[t + s]);
    }
    __syncthreads();
  }
  if (t == 0) {
    put(carry_sum, g.h * g.w - carry_max);               // the last count runs to h*w
    const bool any = area > 0;
    if (A.area) A.area[k] = area;
    if (A.bbox) {
      A.bbox[4 * k + 0] = any ? g.bx + xmin : 0;
      A.bbox[4 * k + 1] = any ? g.by + s_sum[0] : 0;
      A.bbox[4 * k + 2] = any ? xmax - xmin + 1 : 0;
      A.bbox[4 * k + 3] = any ? s_max[0] - s_sum[0] + 1 : 0;
    }
  }
}

// ---- the host side: every refusal happens here, before any launch
int check_mask(const char* what, const long long* runs, long long num_src, long long num_counts, const long long* index, const int* geom,
               long long k, long long* m_out) {
  const int* p = geom + GEOM * k;
  const int h = p[0], w = p[1], d = p[2], bx = p[3], by = p[4], bw = p[5], bh = p[6];
  if (h < 1 || w < 1 || (long long)h * w >= (1ll << 31)) return fail(MI355DET_EINVAL, "%s: mask %lld: h, w >= 1 and h*w < 2^31", what, k);
  if (d < 1) return fail(MI355DET_EINVAL, "%s: mask %lld: the dilation %lld is below 1", what, k, d);
  if (bw < 0 || bh < 0) return fail(MI355DET_EINVAL, "%s: mask %lld: a box of negative size", what, k);
  if (bw > 0 && bh > 0 && (bx < 0 || by < 0 || (long long)bx + bw > w || (long long)by + bh > h))
    return fail(MI355DET_EINVAL, "%s: mask %lld: the box leaves the image", what, k);
  const long long src = index ? index[k] : k;
  if (src < 0 || src >= num_src) return fail(MI355DET_EINVAL, "%s: mask %lld: index %lld is not a source mask", what, k, src);
  const long long r0 = runs[src], r1 = runs[src + 1];
  if (r0 < 0 || r1 < r0 || r1 > num_counts) return fail(MI355DET_EINVAL, "%s: the runs of source mask %lld leave the counts", what, src);
  if (r1 - r0 > (long long)h * w + 1) return fail(MI355DET_EINVAL, "%s: source mask %lld has more counts than pixels", what, src);
  *m_out = r1 - r0;
  return MI355DET_OK;
}

struct Chunk {
  long long small = 0, large = 0;
};

int check_chunk(const char* what, const void* counts, long long num_counts, const long long* runs, const void* runs_dev, long long num_src,
                const long long* index, const void* index_dev, const int* geom, const void* geom_dev, const long long* slices,
                const void* slices_dev, long long n, long long first, long long num, const void* workspace, size_t workspace_bytes, Chunk* ch) {
  if (n < 0 || n >= (1ll << 31) || num_src < 0 || num_counts < 0 || first < 0 || num < 0 || first + num > n)
    return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (num == 0) return MI355DET_OK;
  if (!runs || !runs_dev || !geom || !geom_dev || !slices || !slices_dev || (index != nullptr) != (index_dev != nullptr) ||
      (num_counts > 0 && !counts))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  long long end = 0;
  for (long long k = first; k < first + num; ++k) {
    long long m = 0;
    const int st = check_mask(what, runs, num_src, num_counts, index, geom, k, &m);
    if (st != MI355DET_OK) return st;
    const int* p = geom + GEOM * k;
    const bool none = p[5] <= 0 || p[6] <= 0;
    const long long need = none ? 0 : slice_bytes(m, p[5], p[6]);
    if (slices[k] < end || (slices[k] & 7) || slices[k] + need > (long long)workspace_bytes)
      return fail(MI355DET_EWORKSPACE, "%s: the scratch slice of mask %lld overlaps its neighbour or leaves the workspace", what, k);
    end = slices[k] + need;
    if (none || plane_words(p[5], p[6]) <= SMALL_WORDS) ++ch->small; else ++ch->large;
  }
  if (end > 0 && !workspace) return fail(MI355DET_EWORKSPACE, "%s: no workspace", what);
  return MI355DET_OK;
}

template <bool EMIT>
void launch(const Args& A, long long num, const Chunk& ch, void* stream) {
  if (ch.small) hipLaunchKernelGGL(boundary_kernel<EMIT>, dim3((unsigned)num), dim3(SMALL_THREADS), 0, S(stream), A, 1);
  if (ch.large) hipLaunchKernelGGL(boundary_kernel<EMIT>, dim3((unsigned)num), dim3(LARGE_THREADS), 0, S(stream), A, 0);
}

}  // namespace

extern "C" {

int64_t mi355det_rle_boundary_plan(const int64_t* runs, int64_t num_src, int64_t num_counts, const int64_t* index, const int32_t* geom, int64_t n,
                                   int64_t budget_bytes, int64_t* slices, int64_t* chunk_starts, int64_t* workspace_bytes) {
  const char* what = "rle_boundary_plan";
  if (n < 0 || n >= (1ll << 31) || num_src < 0 || num_counts < 0 || budget_bytes < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (!chunk_starts || !workspace_bytes || (n > 0 && (!runs || !geom || !slices))) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  long long chunks = 0, used = 0, most = 0;
  for (long long k = 0; k < n; ++k) {
    long long m = 0;
    const int st = check_mask(what, (const long long*)runs, num_src, num_counts, (const long long*)index, geom, k, &m);
    if (st != MI355DET_OK) return st;
    const int* p = geom + GEOM * k;
    const long long need = (p[5] <= 0 || p[6] <= 0) ? 0 : slice_bytes(m, p[5], p[6]);
    if (k == 0 || (used > 0 && used + need > budget_bytes)) {         // a chunk holds one mask at least, whatever it needs
      chunk_starts[chunks++] = k;
      used = 0;
    }
    slices[k] = used;
    used += need;
    most = used > most ? used : most;
  }
  chunk_starts[chunks] = n;
  *workspace_bytes = most;
  return chunks;
}

int mi355det_rle_boundary_count(const int32_t* counts, int64_t num_counts, const int64_t* runs, const int64_t* runs_dev, int64_t num_src,
                                const int64_t* index, const int64_t* index_dev, const int32_t* geom, const int32_t* geom_dev,
                                const int64_t* slices, const int64_t* slices_dev, int64_t n, int64_t first, int64_t num, int64_t* num_runs,
                                void* workspace, size_t workspace_bytes, void* stream) {
  Chunk ch;
  const int st = check_chunk("rle_boundary_count", counts, num_counts, (const long long*)runs, runs_dev, num_src, (const long long*)index,
                             index_dev, geom, geom_dev, (const long long*)slices, slices_dev, n, first, num, workspace, workspace_bytes, &ch);
  if (st != MI355DET_OK) return st;
  if (num == 0) return MI355DET_OK;
  if (!num_runs) return fail(MI355DET_EINVAL, "%s: missing operand", "rle_boundary_count");
  Args A{counts, (const long long*)runs_dev, (const long long*)index_dev, geom_dev, (const long long*)slices_dev, first, (char*)workspace,
         (long long*)num_runs, nullptr, nullptr, 0, nullptr, nullptr};
  launch<false>(A, num, ch, stream);
  return check_launch("rle_boundary_count");
}

int mi355det_rle_boundary_emit(const int32_t* counts, int64_t num_counts, const int64_t* runs, const int64_t* runs_dev, int64_t num_src,
                               const int64_t* index, const int64_t* index_dev, const int32_t* geom, const int32_t* geom_dev,
                               const int64_t* slices, const int64_t* slices_dev, int64_t n, int64_t first, int64_t num,
                               const int64_t* run_offsets, int64_t total_runs, int32_t* out_counts, int64_t capacity, int64_t* area,
                               int32_t* bbox, void* workspace, size_t workspace_bytes, void* stream) {
  Chunk ch;
  const int st = check_chunk("rle_boundary_emit", counts, num_counts, (const long long*)runs, runs_dev, num_src, (const long long*)index,
                             index_dev, geom, geom_dev, (const long long*)slices, slices_dev, n, first, num, workspace, workspace_bytes, &ch);
  if (st != MI355DET_OK) return st;
  if (num == 0) return MI355DET_OK;
  const int ce = check_emit("rle_boundary_emit", "%s: total_runs %lld is below one count per mask", n, total_runs, capacity, run_offsets, out_counts);
  if (ce != MI355DET_OK) return ce;
  Args A{counts, (const long long*)runs_dev, (const long long*)index_dev, geom_dev, (const long long*)slices_dev, first, (char*)workspace,
         nullptr, (const long long*)run_offsets, out_counts, (long long)capacity, (long long*)area, bbox};
  launch<true>(A, num, ch, stream);
  return check_launch("rle_boundary_emit");
}

}  // extern "C"
