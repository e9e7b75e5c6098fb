// COCO polygons as run lengths (include/mi355det.h, "Polygon ground truth as COCO run-length encodings"): pycocotools rleFrPoly for every
// polygon, then the union over an annotation's parts (rleMerge), made on the device; and the decode of run lengths to bitmaps.  What
// torchvision_models/detection/coco_utils.py:33-47 (convert_coco_poly_to_mask) gets from frPyObjects + decode + any(dim=2).
//
// rleFrPoly walks the 5x upsampled ring edge by edge, keeps a point a = x*h + y wherever the walk crosses into another pixel column, sorts the
// points and takes differences, skipping a zero difference together with the one after it.  Two facts about that rule carry the mapping:
//   edge independence   the kept points are the union of the points of each edge walked alone (consecutive edges share their vertex's u, or
//                       differ only where the point is dropped), and u, v of walk step d are closed forms of d;
//   parity              the run boundaries are the positions below h*w that occur an odd number of times.
// Passes (fixed order, no atomics, one writer per element):
//   poly_points_kernel  one wavefront per polygon: the lanes stride over the walk steps of each edge in turn and evaluate the pair (d-1, d);
//                       ballot + popcount give the polygon's point count (count pass) and each lane's slot (emit pass).
//                       key = polygon index << 32 | a.  The caller sorts the keys (one device sort).
//   poly_events_kernel  one wavefront per polygon of a MULTI-part annotation: its odd-multiplicity positions in rising order, the r-th one as
//                       the event annotation << 32 | position << 1 | (r & 1): coverage +1 at even r, -1 at odd r.  The caller sorts the events.
//   poly_runs_kernel    one wavefront per annotation.  One part: the state after a position is the parity of the points up to it.  More
//                       parts: the state is "coverage > 0" after all events of a position.  A run boundary is a position where the state
//                       changes; the emit pass writes the gaps, the area (sum of the odd-indexed counts) and the tight box (toBbox).
//   offsets scan        one block (offsets_scan.h): per-item counts -> exclusive offsets, in place.
//   rle_decode_kernel   one wavefront per mask: scans the counts 64 at a time, the wavefront writes each run of ones over a zeroed output.
// All floating point is float64 and this file is compiled with -ffp-contract=off: ys + s*t + .5 must round twice, as the C of pycocotools does.
#include "offsets_scan.h"
#include "rle_protocol.h"

#include <limits.h>

using namespace mi355;

namespace {

typedef unsigned long long u64;

constexpr long long EVENT_NONE = LLONG_MAX;               // fills the unused tail of a polygon's event slots; sorts behind every event

__device__ __forceinline__ int top_bit(u64 m) { return 63 - __clzll((long long)m); }

// the annotation that owns polygon p: the largest a with ann_off[a] <= p (annotations without parts repeat an offset)
__device__ __forceinline__ int owner(const long long* __restrict__ ann_off, int A, long long p) {
  int lo = 0, hi = A;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (ann_off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- rleFrPoly, steps 1-3
__device__ __forceinline__ int scale5(double c) { return (int)(5 * c + .5); }

struct EdgeWalk {
  int xs, ys, len;
  double s;
  bool xmajor, flip;
  __device__ __forceinline__ EdgeWalk(int x0, int y0, int x1, int y1) {
    const int dx = abs(x1 - x0), dy = abs(y0 - y1);
    xmajor = dx >= dy;
    flip = (xmajor && x0 > x1) || (!xmajor && y0 > y1);
    if (flip) {
      int t = x0; x0 = x1; x1 = t;
      t = y0; y0 = y1; y1 = t;
    }
    xs = x0;
    ys = y0;
    len = xmajor ? dx : dy;
    s = xmajor ? (double)(y1 - y0) / dx : (double)(x1 - x0) / dy;      // 0/0 for a zero-length edge: it has no step, s is never read
  }
  __device__ __forceinline__ int2 at(int d) const {                    // (u, v) of walk step d
    const int t = flip ? len - d : d;
    const int r = (int)((xmajor ? ys : xs) + s * t + .5);
    return xmajor ? make_int2(t + xs, r) : make_int2(r, t + ys);
  }
};

// the point a = x*h + y that the pair (u0, v0) -> (u1, v1) of the walk leaves, or -1
__device__ __forceinline__ int boundary_point(int u0, int v0, int u1, int v1, int h, int w) {
  if (u1 == u0) return -1;
  double xd = (double)(u1 < u0 ? u1 : u1 - 1);
  xd = (xd + .5) / 5 - .5;
  if (floor(xd) != xd || xd < 0 || xd > w - 1) return -1;
  double yd = (double)(v1 < v0 ? v1 : v0);
  yd = (yd + .5) / 5 - .5;
  if (yd < 0) yd = 0;
  else if (yd > h) yd = h;
  yd = ceil(yd);
  return (int)xd * h + (int)yd;                           // <= (w-1)*h + h = h*w < 2^31
}

// EMIT = false: pt_off[p] = the polygon's point count.  EMIT = true: pt_off is the scanned table and the keys go to their slots.
template <bool EMIT>
__global__ __launch_bounds__(256) void poly_points_kernel(const double* __restrict__ xy, const long long* __restrict__ poly_off,
                                                          const long long* __restrict__ ann_off, const int* __restrict__ sizes, int NP, int A,
                                                          long long* __restrict__ pt_off, long long* __restrict__ keys, long long capacity) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= NP) return;
  const int ann = owner(ann_off, A, p);
  const int h = sizes[2 * ann], w = sizes[2 * ann + 1];
  const long long first = poly_off[p];
  const int k = (int)(poly_off[p + 1] - first);
  const u64 below = (1ull << lane) - 1ull;
  const long long base = EMIT ? pt_off[p] : 0;
  const long long limit = EMIT ? min(capacity, pt_off[p + 1]) : 0;
  long long n = 0;
  for (int j = 0; j < k; ++j) {
    const double* a = xy + 2 * (first + j);
    const double* b = xy + 2 * (first + (j + 1 == k ? 0 : j + 1));       // the ring closes on its first point
    const EdgeWalk E(scale5(a[0]), scale5(a[1]), scale5(b[0]), scale5(b[1]));
    for (int d0 = 1; d0 <= E.len; d0 += WAVE) {
      const int d = d0 + lane;
      int pos = -1;
      if (d <= E.len) {
        const int2 a0 = E.at(d - 1), a1 = E.at(d);
        pos = boundary_point(a0.x, a0.y, a1.x, a1.y, h, w);
      }
      const bool hit = pos >= 0;
      const u64 m = __ballot(hit);
      if (EMIT && hit) {
        const long long slot = base + n + __popcll(m & below);
        if (slot < limit) keys[slot] = (p << 32) | (long long)pos;
      }
      n += __popcll(m);
    }
  }
  if (!EMIT && lane == 0) pt_off[p] = n;
}

// ---- the two sorted streams a wavefront walks.  get(i): position and coverage weight of element i; state(cov): the bit after cov.
struct PointStream {                                      // one polygon's sorted keys: every point flips the bit
  const long long* keys;
  __device__ __forceinline__ int pos(long long i) const { return (int)(unsigned)keys[i]; }
  __device__ __forceinline__ int weight(long long) const { return 1; }
  __device__ __forceinline__ bool state(int cov) const { return cov & 1; }
};
struct EventStream {                                      // one annotation's sorted events: the bit is "some part covers the pixel"
  const long long* events;
  __device__ __forceinline__ int pos(long long i) const { return (int)((unsigned)events[i] >> 1); }
  __device__ __forceinline__ int weight(long long i) const { return (events[i] & 1) ? -1 : 1; }
  __device__ __forceinline__ bool state(int cov) const { return cov > 0; }
};

// The run boundaries of the sorted elements [s, e): positions below hw after whose last element the state differs from the state before
// the position.  f(is_boundary, position, ballot of the boundaries, boundaries before this chunk) runs once per chunk of 64 on every lane.
template <class Stream, class F>
__device__ __forceinline__ long long walk_boundaries(const Stream& S, long long s, long long e, int hw, int lane, F&& f) {
  const u64 below = (1ull << lane) - 1ull;
  int carry_cov = 0;
  bool carry_state = false;
  long long T = 0;
  for (long long c = s; c < e; c += WAVE) {
    const long long i = c + lane;
    int pos = 0, wgt = 0;
    bool last = false;                                    // the last element of its position
    if (i < e) {
      pos = S.pos(i);
      wgt = S.weight(i);
      last = i + 1 == e || S.pos(i + 1) != pos;
    }
    const int cov = carry_cov + wave_scan_incl(wgt, lane);
    const bool st = S.state(cov);
    const u64 ends = __ballot(last), states = __ballot(st);
    const u64 lower = ends & below;
    const bool before = lower ? ((states >> top_bit(lower)) & 1) != 0 : carry_state;
    const bool is_b = last && pos < hw && st != before;
    const u64 bm = __ballot(is_b);
    f(is_b, pos, bm, T);
    T += __popcll(bm);
    carry_cov = __shfl(cov, WAVE - 1, WAVE);
    if (ends) carry_state = ((states >> top_bit(ends)) & 1) != 0;
  }
  return T;
}

__global__ __launch_bounds__(256) void poly_events_kernel(const long long* __restrict__ keys, const long long* __restrict__ pt_off,
                                                          const long long* __restrict__ ann_off, const int* __restrict__ sizes,
                                                          const long long* __restrict__ event_base, int NP, int A,
                                                          long long* __restrict__ events, long long capacity, long long* __restrict__ tog_off) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= NP) return;
  const int ann = owner(ann_off, A, p);
  const long long base = event_base[p];
  if (ann_off[ann + 1] - ann_off[ann] < 2 || base < 0) {  // a single part goes straight from its points to counts
    if (lane == 0) tog_off[p] = 0;
    return;
  }
  const int hw = sizes[2 * ann] * sizes[2 * ann + 1];
  const long long s = pt_off[p], e = pt_off[p + 1];
  const u64 below = (1ull << lane) - 1ull;
  const long long T = walk_boundaries(PointStream{keys}, s, e, hw, lane, [&](bool is_b, int pos, u64 bm, long long before) {
    if (!is_b) return;
    const long long r = before + __popcll(bm & below);
    if (r < e - s && base + r < capacity) events[base + r] = ((long long)ann << 32) | (long long)(((unsigned)pos << 1) | (unsigned)(r & 1));
  });
  for (long long r = T + lane; r < e - s; r += WAVE)
    if (base + r < capacity) events[base + r] = EVENT_NONE;
  if (lane == 0) tog_off[p] = T;
}

struct RunStats {
  long long area = 0;
  int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
  bool whole = false;                                     // a run of ones that goes on into the next column covers y = 0 and y = h - 1
  __device__ __forceinline__ void add(int first, int last, int h) {
    area += last - first + 1;
    const int x0 = first / h, x1 = last / h;
    xmin = min(xmin, x0);
    xmax = max(xmax, x1);
    ymin = min(ymin, first - x0 * h);
    ymax = max(ymax, last - x1 * h);
    whole |= x1 > x0;
  }
};

template <bool EMIT>
__global__ __launch_bounds__(256) void poly_runs_kernel(const long long* __restrict__ keys, const long long* __restrict__ pt_off,
                                                        const long long* __restrict__ events, const long long* __restrict__ tog_off,
                                                        const long long* __restrict__ ann_off, const int* __restrict__ sizes, int A,
                                                        long long* __restrict__ run_off, int* __restrict__ counts, long long capacity,
                                                        long long* __restrict__ area, int* __restrict__ bbox) {
  const int lane = threadIdx.x & 63;
  const long long a = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= A) return;
  const long long p0 = ann_off[a], p1 = ann_off[a + 1];
  const int h = sizes[2 * a], hw = h * sizes[2 * a + 1];
  const bool multi = p1 - p0 > 1;
  const long long s = p1 == p0 ? 0 : multi ? tog_off[p0] : pt_off[p0];
  const long long e = p1 == p0 ? 0 : multi ? tog_off[p1] : pt_off[p1];
  const u64 below = (1ull << lane) - 1ull;
  const long long first = EMIT ? run_off[a] : 0;
  const long long limit = EMIT ? min(capacity, run_off[a + 1]) : 0;
  int carry_pos = 0;                                      // the boundary before the chunk (0: the first count is measured from pixel 0)
  RunStats st;
  auto emit = [&](bool is_b, int pos, u64 bm, long long before) {
    if (!EMIT) return;
    const u64 lower = bm & below;
    const int from = __shfl(pos, lower ? top_bit(lower) : 0, WAVE);
    if (is_b) {
      const int prev = lower ? from : carry_pos;
      const long long k = before + __popcll(lower);
      if (first + k < limit) counts[first + k] = pos - prev;
      if (k & 1) st.add(prev, pos - 1, h);
    }
    if (bm) carry_pos = __shfl(pos, top_bit(bm), WAVE);
  };
  const long long T = multi ? walk_boundaries(EventStream{events}, s, e, hw, lane, emit) : walk_boundaries(PointStream{keys}, s, e, hw, lane, emit);
  if (!EMIT) {
    if (lane == 0) run_off[a] = T + 1;
    return;
  }
  if (lane == 0) {                                        // the last count runs to h*w
    if (first + T < limit) counts[first + T] = hw - carry_pos;
    if (T & 1) st.add(carry_pos, hw - 1, h);
  }
  st.area = wave_sum_i64(st.area);                        // integer sums, minima and maxima: order-free, so exact
  st.xmin = wave_min_i(st.xmin);
  st.xmax = wave_max_i(st.xmax);
  st.ymin = wave_min_i(st.ymin);
  st.ymax = wave_max_i(st.ymax);
  const bool whole = __ballot(st.whole) != 0;
  if (lane == 0) {
    if (area) area[a] = st.area;
    if (bbox) {
      const bool any = st.area > 0;
      const int ymin = whole ? 0 : st.ymin, ymax = whole ? h - 1 : st.ymax;
      bbox[4 * a + 0] = any ? st.xmin : 0;
      bbox[4 * a + 1] = any ? ymin : 0;
      bbox[4 * a + 2] = any ? st.xmax - st.xmin + 1 : 0;
      bbox[4 * a + 3] = any ? ymax - ymin + 1 : 0;
    }
  }
}

// out is zeroed by the caller; counts that run past H*W are cut there
__global__ __launch_bounds__(256) void rle_decode_kernel(const int* __restrict__ counts, const long long* __restrict__ run_off, int D, int H,
                                                         int W, unsigned char* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long d = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= D) return;
  const long long s = run_off[d], e = run_off[d + 1];
  const int hw = H * W;
  unsigned char* o = out + (size_t)d * hw;
  int carry = 0;                                          // the pixels before the chunk, never above hw
  for (long long c = s; c < e && carry < hw; c += WAVE) {
    const long long i = c + lane;
    const int n = i < e ? min(max(counts[i], 0), hw) : 0;
    const long long end = carry + wave_scan_incl((long long)n, lane);       // in int64: 64 counts of up to hw each
    const int stop = (int)min(end, (long long)hw), start = (int)min(end - n, (long long)hw);
    const bool ones = i < e && ((i - s) & 1) && stop > start;
    u64 m = __ballot(ones);
    while (m) {                                           // the wavefront writes one run of ones at a time
      const int j = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int b0 = __shfl(start, j, WAVE), b1 = __shfl(stop, j, WAVE);
      for (int q = b0 + lane; q < b1; q += WAVE) {
        const int x = q / H, y = q - x * H;
        o[(size_t)y * W + x] = 1;
      }
    }
    carry = __shfl(stop, WAVE - 1, WAVE);
  }
}

inline unsigned waves4(long long n) { return (unsigned)((n + 3) / 4); }

int check_tables(const char* what, int NP, int A, const void* poly_off, const void* ann_off, const void* sizes) {
  if (NP < 0 || A < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (NP > 0 && A == 0) return fail(MI355DET_EINVAL, "%s: polygons without an annotation", what);
  if (A > 0 && (!ann_off || !sizes)) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if (NP > 0 && !poly_off) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  return MI355DET_OK;
}

}  // namespace

extern "C" {

int mi355det_poly_points_count(const double* xy, const int64_t* poly_offsets, const int64_t* ann_offsets, const int32_t* sizes,
                               int32_t num_polys, int32_t num_anns, int64_t* point_offsets, void* stream) {
  const int st = check_tables("poly_points_count", num_polys, num_anns, poly_offsets, ann_offsets, sizes);
  if (st != MI355DET_OK) return st;
  if (num_polys == 0) return MI355DET_OK;
  if (!xy || !point_offsets) return fail(MI355DET_EINVAL, "%s: missing operand", "poly_points_count");
  hipLaunchKernelGGL(poly_points_kernel<false>, dim3(waves4(num_polys)), dim3(256), 0, S(stream), xy, (const long long*)poly_offsets,
                     (const long long*)ann_offsets, sizes, num_polys, num_anns, (long long*)point_offsets, (long long*)nullptr, 0ll);
  launch_offsets_scan(num_polys, ScanInPlace{(const long long*)point_offsets}, (long long*)point_offsets, stream);
  return check_launch("poly_points_count");
}

int mi355det_poly_points_emit(const double* xy, const int64_t* poly_offsets, const int64_t* ann_offsets, const int32_t* sizes,
                              int32_t num_polys, int32_t num_anns, const int64_t* point_offsets, int64_t total_points, int64_t* keys,
                              int64_t capacity, void* stream) {
  const int st = check_tables("poly_points_emit", num_polys, num_anns, poly_offsets, ann_offsets, sizes);
  if (st != MI355DET_OK) return st;
  if (total_points < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", "poly_points_emit");
  if (capacity < total_points)
    return fail(MI355DET_EINVAL, "%s: capacity %lld is smaller than the %lld points", "poly_points_emit", capacity, total_points);
  if (num_polys == 0 || total_points == 0) return MI355DET_OK;
  if (!xy || !point_offsets || !keys) return fail(MI355DET_EINVAL, "%s: missing operand", "poly_points_emit");
  hipLaunchKernelGGL(poly_points_kernel<true>, dim3(waves4(num_polys)), dim3(256), 0, S(stream), xy, (const long long*)poly_offsets,
                     (const long long*)ann_offsets, sizes, num_polys, num_anns, (long long*)point_offsets, (long long*)keys,
                     (long long)capacity);
  return check_launch("poly_points_emit");
}

int mi355det_poly_events(const int64_t* keys, const int64_t* point_offsets, const int64_t* ann_offsets, const int32_t* sizes,
                         const int64_t* event_base, int32_t num_polys, int32_t num_anns, int64_t* events, int64_t capacity,
                         int64_t* toggle_offsets, void* stream) {
  const int st = check_tables("poly_events", num_polys, num_anns, point_offsets, ann_offsets, sizes);
  if (st != MI355DET_OK) return st;
  if (capacity < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", "poly_events");
  if (num_polys == 0) return MI355DET_OK;
  if (!event_base || !toggle_offsets || (capacity > 0 && (!events || !keys))) return fail(MI355DET_EINVAL, "%s: missing operand", "poly_events");
  hipLaunchKernelGGL(poly_events_kernel, dim3(waves4(num_polys)), dim3(256), 0, S(stream), (const long long*)keys,
                     (const long long*)point_offsets, (const long long*)ann_offsets, sizes, (const long long*)event_base, num_polys, num_anns,
                     (long long*)events, (long long)capacity, (long long*)toggle_offsets);
  launch_offsets_scan(num_polys, ScanInPlace{(const long long*)toggle_offsets}, (long long*)toggle_offsets, stream);
  return check_launch("poly_events");
}

int mi355det_poly_runs_count(const int64_t* keys, const int64_t* point_offsets, const int64_t* events, const int64_t* toggle_offsets,
                             const int64_t* ann_offsets, const int32_t* sizes, int32_t num_polys, int32_t num_anns, int64_t* run_offsets,
                             void* stream) {
  const int st = check_tables("poly_runs_count", num_polys, num_anns, point_offsets, ann_offsets, sizes);
  if (st != MI355DET_OK) return st;
  if (num_anns == 0) return MI355DET_OK;
  if (!run_offsets || (num_polys > 0 && !toggle_offsets)) return fail(MI355DET_EINVAL, "%s: missing operand", "poly_runs_count");
  hipLaunchKernelGGL(poly_runs_kernel<false>, dim3(waves4(num_anns)), dim3(256), 0, S(stream), (const long long*)keys,
                     (const long long*)point_offsets, (const long long*)events, (const long long*)toggle_offsets,
                     (const long long*)ann_offsets, sizes, num_anns, (long long*)run_offsets, (int*)nullptr, 0ll, (long long*)nullptr,
                     (int*)nullptr);
  launch_offsets_scan(num_anns, ScanInPlace{(const long long*)run_offsets}, (long long*)run_offsets, stream);
  return check_launch("poly_runs_count");
}

int mi355det_poly_runs_emit(const int64_t* keys, const int64_t* point_offsets, const int64_t* events, const int64_t* toggle_offsets,
                            const int64_t* ann_offsets, const int32_t* sizes, int32_t num_polys, int32_t num_anns, const int64_t* run_offsets,
                            int64_t total_runs, int32_t* counts, int64_t capacity, int64_t* area, int32_t* bbox, void* stream) {
  const int st = check_tables("poly_runs_emit", num_polys, num_anns, point_offsets, ann_offsets, sizes);
  if (st != MI355DET_OK) return st;
  if (num_anns == 0) return MI355DET_OK;
  const int ce = check_emit("poly_runs_emit", "%s: total_runs %lld is below one count per annotation", num_anns, total_runs, capacity, run_offsets, counts);
  if (ce != MI355DET_OK) return ce;
  if (num_polys > 0 && !toggle_offsets) return fail(MI355DET_EINVAL, "%s: missing operand", "poly_runs_emit");
  hipLaunchKernelGGL(poly_runs_kernel<true>, dim3(waves4(num_anns)), dim3(256), 0, S(stream), (const long long*)keys,
                     (const long long*)point_offsets, (const long long*)events, (const long long*)toggle_offsets,
                     (const long long*)ann_offsets, sizes, num_anns, (long long*)run_offsets, counts, (long long)capacity, (long long*)area,
                     bbox);
  return check_launch("poly_runs_emit");
}

int mi355det_rle_decode(const int32_t* counts, const int64_t* run_offsets, int32_t num_masks, int32_t im_h, int32_t im_w, uint8_t* out,
                        void* stream) {
  if (num_masks < 0 || im_h <= 0 || im_w <= 0) return fail(MI355DET_EINVAL, "%s: bad arguments", "rle_decode");
  if ((long long)im_h * im_w >= (1ll << 31))
    return fail(MI355DET_EINVAL, "%s: im_h*im_w = %lld does not fit the int32 counts", "rle_decode", (long long)im_h * im_w);
  if (num_masks == 0) return MI355DET_OK;
  if (!counts || !run_offsets || !out) return fail(MI355DET_EINVAL, "%s: missing operand", "rle_decode");
  if (hipMemsetAsync(out, 0, (size_t)num_masks * im_h * im_w, S(stream)) != hipSuccess) return check_launch("rle_decode");
  hipLaunchKernelGGL(rle_decode_kernel, dim3(waves4(num_masks)), dim3(256), 0, S(stream), counts, (const long long*)run_offsets, num_masks,
                     im_h, im_w, out);
  return check_launch("rle_decode");
}

}  // extern "C"
