// AP-pool on the device (include/mi355det.h, "Pooled precision-recall"): the precision-recall pass of coco_accumulate_kernel
// (cocoeval_kernels.hip) for a few very long lists instead of many short ones.  A pool's list - the detection slots of a set of categories in
// one descending score order - is cut into tiles of POOL_TILE positions; one wavefront owns a tile in every pass, and what a tile needs from
// the others travels through small per-tile tables BETWEEN launches.  No kernel waits on another workgroup.
//
//   pooled_plan_kernel     the device copy of the pool offsets, clamped into [0, P] and made non-decreasing, and the first tile of every pool
//   pooled_pack_kernel     the one gather: order[p], then the A*T planes of dt_match / dt_ignore -> per position one 64-bit tp mask and one
//                          64-bit fp mask (bit a*T + t), 16 contiguous bytes that every later pass streams; the tile's tp / fp totals per cell
//   pooled_scan_kernel     block = pool, lane = cell: the exclusive sums of the tile totals (integers: exact in any order)
//   pooled_tilemax_kernel  per tile and cell the largest precision at a true positive of the tile (0 without one)
//   pooled_finish_kernel   block = pool, lane = cell: the maximum over the LATER tiles, exclusive; and the cells nobody else writes: recall,
//                          the thresholds past the last recall (0), everything where npig == 0 (-1)
//   pooled_emit_kernel     per tile a walk from the right over its true positives: the running maximum of the precision, and every true
//                          positive writes the recall thresholds it is the first to reach (the first position: from threshold 0, whatever
//                          its flags)
//
// Lane c = a*T + t keeps cell c, the mapping of coco_match_kernel: a ballot of bit c of the masks of 64 consecutive positions IS cell c's flag
// word for those positions, so the transposition costs two ballots per cell and the cumulative counts inside a word are popcounts.
// The precision is evaluated at true positives only.  That gives the bits of the literal form: between two true positives tp stays and fp
// grows, so fl(tp / (fl(fp + tp) + 2^-52)) cannot rise (every operation is correctly rounded, hence monotone), and a position that owns a
// threshold is a true positive or the first one, where the maximum from the right is max(0, the true positives').
// No atomics, one writer per output element, 64-bit positions: the same bits from run to run.
// Compiled with -ffp-contract=off: the quotients are those of coco_accumulate_kernel, operation for operation.
#include "wave_ops.h"

using namespace mi355;

namespace {

constexpr int POOL_CHUNKS = 16;                  // 64-position words per tile
constexpr int POOL_TILE = POOL_CHUNKS * WAVE;    // positions one wavefront owns per pass
constexpr int SCAN_WAVES = 16;                   // the per-pool passes over the tile tables: segments of tiles, one per wave

typedef unsigned long long u64;

struct PoolWs {
  ulonglong2* packed;        // [P] (tp mask, fp mask)
  long long* off;            // [S + 1] the clamped offsets
  long long* tile_base;      // [S + 1] first tile of each pool
  long long* pre_tp;         // [tiles, C] true positives before the tile
  long long* pre_fp;
  double* tile_max;          // [tiles, C]
  double* suf_max;           // [tiles, C] maximum of the later tiles of the pool
  int* tile_tp;              // [tiles, C]
  int* tile_fp;
};

inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// the workspace layout; -> bytes.  A pool adds at most one partial tile.
size_t carve(void* base, long long P, long long S, int C, PoolWs* w) {
  const size_t tiles = (size_t)(P / POOL_TILE + S), cells = tiles * (size_t)C;
  char* p = (char*)base;
  size_t n = 0;
  auto take = [&](size_t bytes) {
    char* at = p + n;
    n += up16(bytes);
    return at;
  };
  PoolWs t;
  t.packed = (ulonglong2*)take((size_t)P * sizeof(ulonglong2));
  t.off = (long long*)take((size_t)(S + 1) * sizeof(long long));
  t.tile_base = (long long*)take((size_t)(S + 1) * sizeof(long long));
  t.pre_tp = (long long*)take(cells * sizeof(long long));
  t.pre_fp = (long long*)take(cells * sizeof(long long));
  t.tile_max = (double*)take(cells * sizeof(double));
  t.suf_max = (double*)take(cells * sizeof(double));
  t.tile_tp = (int*)take(cells * sizeof(int));
  t.tile_fp = (int*)take(cells * sizeof(int));
  if (w) *w = t;
  return n;
}

__global__ __launch_bounds__(WAVE) void pooled_plan_kernel(const long long* __restrict__ pool_offsets, int S, long long P,
                                                           long long* __restrict__ off, long long* __restrict__ tile_base) {
  if (threadIdx.x != 0) return;
  long long prev = 0, tiles = 0;
  for (int s = 0; s <= S; ++s) {
    long long o = pool_offsets[s];
    o = o < prev ? prev : (o > P ? P : o);
    if (s > 0) tiles += (o - prev + POOL_TILE - 1) / POOL_TILE;
    off[s] = o;
    tile_base[s] = tiles;
    prev = o;
  }
}

// the pool that owns `tile`: the last s < S with tile_base[s] <= tile (an empty pool shares its base with the next one)
__device__ __forceinline__ int pool_of(const long long* __restrict__ tile_base, int S, long long tile) {
  int lo = 0, hi = S;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_base[mid] <= tile) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct Tile {
  int s;
  long long first, p0, p1;      // the pool's first position, the tile's positions p0..p1 (absolute, in pool_order)
  int chunks;
};

__device__ __forceinline__ bool tile_of(const long long* __restrict__ off, const long long* __restrict__ tile_base, int S, long long tile, Tile& t) {
  if (tile >= tile_base[S]) return false;
  t.s = pool_of(tile_base, S, tile);
  t.first = off[t.s];
  t.p0 = t.first + (tile - tile_base[t.s]) * POOL_TILE;
  const long long end = off[t.s + 1];
  t.p1 = end - t.p0 < POOL_TILE ? end : t.p0 + POOL_TILE;
  t.chunks = (int)((t.p1 - t.p0 + WAVE - 1) / WAVE);
  return t.p1 > t.p0;
}

// the transposition: per lane the masks of one position (bit c = cell c) -> lane c: cell c's flags of the 64 positions (bit l = lane l's)
__device__ __forceinline__ void cell_words(u64 tpm, u64 fpm, int C, int lane, u64& tpw, u64& fpw) {
  tpw = fpw = 0;
  for (int c = 0; c < C; ++c) {
    const u64 bt = __ballot((int)((tpm >> c) & 1)), bf = __ballot((int)((fpm >> c) & 1));
    if (lane == c) {
      tpw = bt;
      fpw = bf;
    }
  }
}

// chunk ch of a tile from the packed masks, transposed
__device__ __forceinline__ void load_words(const ulonglong2* __restrict__ packed, const Tile& t, int ch, int C, int lane, u64& tpw, u64& fpw) {
  const long long p = t.p0 + (long long)ch * WAVE + lane;
  ulonglong2 m = make_ulonglong2(0, 0);
  if (p < t.p1) m = packed[p];
  cell_words(m.x, m.y, C, lane, tpw, fpw);
}

__device__ __forceinline__ u64 upto(int i) { return (2ull << i) - 1; }      // bits 0..i (i = 63: all)

__device__ __forceinline__ double precision_at(long long tps, long long fps) {
  const double eps = 2.220446049250313e-16;            // 2^-52, numpy's spacing(1)
  return (double)tps / ((double)fps + (double)tps + eps);
}

__global__ __launch_bounds__(WAVE) void pooled_pack_kernel(PoolWs W, int S, const long long* __restrict__ order, long long num_dt,
                                                           const int* __restrict__ dt_match, const unsigned char* __restrict__ dt_ignore,
                                                           int C) {
  const int lane = threadIdx.x;
  const long long tile = blockIdx.x;
  Tile t;
  if (!tile_of(W.off, W.tile_base, S, tile, t)) return;
  int tot_tp = 0, tot_fp = 0;
  for (int ch = 0; ch < t.chunks; ++ch) {
    const long long p = t.p0 + (long long)ch * WAVE + lane;
    u64 tpm = 0, fpm = 0;
    if (p < t.p1) {
      const long long idx = order[p];
      if (idx >= 0 && idx < num_dt) {
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
          const bool matched = dt_match[(size_t)c * num_dt + idx] != 0, ign = dt_ignore[(size_t)c * num_dt + idx] != 0;
          tpm |= (u64)(matched && !ign) << c;
          fpm |= (u64)(!matched && !ign) << c;
        }
      }
      W.packed[p] = make_ulonglong2(tpm, fpm);
    }
    u64 tpw, fpw;
    cell_words(tpm, fpm, C, lane, tpw, fpw);
    tot_tp += __popcll(tpw);
    tot_fp += __popcll(fpw);
  }
  if (lane < C) {
    W.tile_tp[tile * C + lane] = tot_tp;
    W.tile_fp[tile * C + lane] = tot_fp;
  }
}

// the tiles of pool `s` that wave `w` of a per-pool block walks: j0..j1 of nt
__device__ __forceinline__ void segment(long long nt, int w, long long& j0, long long& j1) {
  const long long seg = (nt + SCAN_WAVES - 1) / SCAN_WAVES;
  j0 = (long long)w * seg < nt ? (long long)w * seg : nt;
  j1 = j0 + seg < nt ? j0 + seg : nt;
}

__global__ __launch_bounds__(SCAN_WAVES* WAVE) void pooled_scan_kernel(PoolWs W, int C) {
  __shared__ long long s_tp[SCAN_WAVES][WAVE], s_fp[SCAN_WAVES][WAVE];
  const int lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE, s = blockIdx.x;
  const long long b = W.tile_base[s], nt = W.tile_base[s + 1] - b;
  long long j0, j1;
  segment(nt, w, j0, j1);
  long long tp = 0, fp = 0;
  if (lane < C) {
#pragma unroll 8
    for (long long j = j0; j < j1; ++j) {
      tp += W.tile_tp[(b + j) * C + lane];
      fp += W.tile_fp[(b + j) * C + lane];
    }
  }
  s_tp[w][lane] = tp;
  s_fp[w][lane] = fp;
  __syncthreads();
  if (lane >= C) return;
  tp = fp = 0;
  for (int v = 0; v < w; ++v) {
    tp += s_tp[v][lane];
    fp += s_fp[v][lane];
  }
  for (long long j = j0; j < j1; ++j) {
    W.pre_tp[(b + j) * C + lane] = tp;
    W.pre_fp[(b + j) * C + lane] = fp;
    tp += W.tile_tp[(b + j) * C + lane];
    fp += W.tile_fp[(b + j) * C + lane];
  }
}

__global__ __launch_bounds__(WAVE) void pooled_tilemax_kernel(PoolWs W, int S, int C) {
  const int lane = threadIdx.x;
  const long long tile = blockIdx.x;
  Tile t;
  if (!tile_of(W.off, W.tile_base, S, tile, t)) return;
  long long tps = 0, fps = 0;
  if (lane < C) {
    tps = W.pre_tp[tile * C + lane];
    fps = W.pre_fp[tile * C + lane];
  }
  double mx = 0.0;
  for (int ch = 0; ch < t.chunks; ++ch) {
    u64 tpw, fpw;
    load_words(W.packed, t, ch, C, lane, tpw, fpw);
    for (u64 w = tpw; w; w &= w - 1) {
      const int i = __ffsll((long long)w) - 1;
      mx = fmax(mx, precision_at(tps + __popcll(tpw & upto(i)), fps + __popcll(fpw & upto(i))));
    }
    tps += __popcll(tpw);
    fps += __popcll(fpw);
  }
  if (lane < C) W.tile_max[tile * C + lane] = mx;
}

// the number of recall thresholds <= x
__device__ __forceinline__ int reached(const double* thr, int R, double x) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct PoolOut {
  double *precision, *scores, *recall;
  int T, R, S, A;
  __device__ size_t p(int t, int r, int s, int a) const { return (((size_t)t * R + r) * S + s) * A + a; }      // [T, R, S, A]
  __device__ size_t r(int t, int s, int a) const { return ((size_t)t * S + s) * A + a; }                       // [T, S, A]
};

__global__ __launch_bounds__(SCAN_WAVES* WAVE) void pooled_finish_kernel(PoolWs W, int C, const long long* __restrict__ pool_npig,
                                                                         const double* __restrict__ rec_thrs, PoolOut O) {
  __shared__ double s_mx[SCAN_WAVES][WAVE];
  const int lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE, s = blockIdx.x;
  const long long b = W.tile_base[s], nt = W.tile_base[s + 1] - b;
  long long j0, j1;
  segment(nt, w, j0, j1);
  double mx = 0.0;
  if (lane < C) {
#pragma unroll 8
    for (long long j = j0; j < j1; ++j) mx = fmax(mx, W.tile_max[(b + j) * C + lane]);
  }
  s_mx[w][lane] = mx;
  __syncthreads();
  if (lane >= C) return;
  mx = 0.0;
  for (int v = w + 1; v < SCAN_WAVES; ++v) mx = fmax(mx, s_mx[v][lane]);
  for (long long j = j1 - 1; j >= j0; --j) {
    W.suf_max[(b + j) * C + lane] = mx;
    mx = fmax(mx, W.tile_max[(b + j) * C + lane]);
  }
  if (w != 0) return;
  // the cells no tile writes
  const int a = lane / O.T, t = lane % O.T;
  const long long npig = pool_npig[(size_t)s * O.A + a], len = W.off[s + 1] - W.off[s];
  if (npig <= 0) {
    for (int r = 0; r < O.R; ++r) O.precision[O.p(t, r, s, a)] = O.scores[O.p(t, r, s, a)] = -1.0;
    O.recall[O.r(t, s, a)] = -1.0;
    return;
  }
  const long long tot = nt > 0 ? W.pre_tp[(b + nt - 1) * C + lane] + W.tile_tp[(b + nt - 1) * C + lane] : 0;
  const double rc = len > 0 ? (double)tot / (double)npig : 0.0;
  for (int r = len > 0 ? reached(rec_thrs, O.R, rc) : 0; r < O.R; ++r) O.precision[O.p(t, r, s, a)] = O.scores[O.p(t, r, s, a)] = 0.0;
  O.recall[O.r(t, s, a)] = rc;
}

__global__ __launch_bounds__(WAVE) void pooled_emit_kernel(PoolWs W, int S, int C, const long long* __restrict__ order, long long num_dt,
                                                           const double* __restrict__ dt_score, const long long* __restrict__ pool_npig,
                                                           const double* __restrict__ rec_thrs, PoolOut O) {
  extern __shared__ double s_thr[];
  const int lane = threadIdx.x;
  const long long tile = blockIdx.x;
  for (int r = lane; r < O.R; r += WAVE) s_thr[r] = rec_thrs[r];
  __syncthreads();
  Tile tl;
  if (!tile_of(W.off, W.tile_base, S, tile, tl)) return;
  const int a = lane / O.T, t = lane % O.T, s = tl.s;
  long long npig = 0, end_tp = 0, end_fp = 0;
  double run = 0.0;
  if (lane < C) {
    npig = pool_npig[(size_t)s * O.A + a];
    end_tp = W.pre_tp[tile * C + lane] + W.tile_tp[tile * C + lane];
    end_fp = W.pre_fp[tile * C + lane] + W.tile_fp[tile * C + lane];
    run = W.suf_max[tile * C + lane];
  }
  const bool live = lane < C && npig > 0;
  const double dn = (double)npig;
  auto write = [&](int r0, int r1, long long p) {
    if (r1 <= r0) return;
    const long long idx = order[p];
    const double sc = idx >= 0 && idx < num_dt ? dt_score[idx] : 0.0;
    for (int r = r0; r < r1; ++r) {
      O.precision[O.p(t, r, s, a)] = run;
      O.scores[O.p(t, r, s, a)] = sc;
    }
  };
  u64 tpw = 0, fpw = 0;
  for (int ch = tl.chunks - 1; ch >= 0; --ch) {
    load_words(W.packed, tl, ch, C, lane, tpw, fpw);
    const long long start_tp = end_tp - __popcll(tpw), start_fp = end_fp - __popcll(fpw);
    if (live) {
      for (u64 w = tpw; w;) {
        const int i = 63 - __clzll((long long)w);
        w &= ~(1ull << i);
        const long long tps = start_tp + __popcll(tpw & upto(i)), fps = start_fp + __popcll(fpw & upto(i));
        run = fmax(run, precision_at(tps, fps));
        const long long p = tl.p0 + (long long)ch * WAVE + i;
        write(p == tl.first ? 0 : reached(s_thr, O.R, (double)(tps - 1) / dn), reached(s_thr, O.R, (double)tps / dn), p);
      }
    }
    end_tp = start_tp;
    end_fp = start_fp;
  }
  // the pool's first position owns the thresholds its recall of 0 reaches, whatever its flags
  if (live && tl.p0 == tl.first && !(tpw & 1)) write(0, reached(s_thr, O.R, 0.0 / dn), tl.first);
}

}  // namespace

extern "C" {

int mi355det_pooled_tile(void) { return POOL_TILE; }

size_t mi355det_pooled_accumulate_workspace(int64_t num_order, int32_t num_pools, int32_t num_thrs, int32_t num_areas) {
  if (num_order < 0 || num_pools <= 0 || num_thrs <= 0 || num_areas <= 0 || (long long)num_thrs * num_areas > WAVE) return 0;
  return carve(nullptr, num_order, num_pools, num_thrs * num_areas, nullptr);
}

int mi355det_pooled_accumulate(const int64_t* pool_order, int64_t num_order, const int64_t* pool_offsets, const int64_t* pool_offsets_host,
                               int32_t num_pools, const int64_t* pool_npig, int64_t num_dt, const double* dt_score, const int32_t* dt_match,
                               const uint8_t* dt_ignore, int32_t num_thrs, int32_t num_areas, const double* rec_thrs, int32_t num_recs,
                               double* precision, double* recall, double* scores, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "pooled_accumulate";
  if (num_order < 0 || num_dt < 0) return fail(MI355DET_EINVAL, "%s: negative size", what);
  if (num_pools <= 0 || num_thrs <= 0 || num_areas <= 0 || num_recs <= 0)
    return fail(MI355DET_EINVAL, "%s: pools, thresholds, area ranges and recall thresholds must be positive", what);
  if ((long long)num_thrs * num_areas > WAVE)
    return fail(MI355DET_EINVAL, "%s: thresholds x area ranges = %lld must be 1..64 (one lane each)", what, (long long)num_thrs * num_areas);
  if (num_recs > 4096) return fail(MI355DET_EINVAL, "%s: at most 4096 recall thresholds, not %lld", what, num_recs);
  if (!pool_offsets || !pool_offsets_host || !pool_npig || !rec_thrs || !precision || !recall || !scores || !workspace)
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  if (num_order > 0 && (!pool_order || (num_dt > 0 && (!dt_score || !dt_match || !dt_ignore))))
    return fail(MI355DET_EINVAL, "%s: missing operand", what);
  long long tiles = 0, prev = 0;
  for (int s = 0; s <= num_pools; ++s) {
    const long long o = pool_offsets_host[s];
    if (o < prev) return fail(MI355DET_EINVAL, "%s: pool offsets must be non-negative and non-decreasing (entry %lld)", what, s);
    if (o > num_order) return fail(MI355DET_EINVAL, "%s: pool offsets end past the %lld entries of pool_order", what, num_order);
    if (s > 0) tiles += (o - prev + POOL_TILE - 1) / POOL_TILE;
    prev = o;
  }
  const int C = num_thrs * num_areas;
  PoolWs W;
  const size_t need = carve(workspace, num_order, num_pools, C, &W);
  if (workspace_bytes < need) return fail(MI355DET_EINVAL, "%s: the workspace must hold %lld bytes, not %lld", what, (long long)need, (long long)workspace_bytes);
  if (tiles >= (1ll << 31)) return fail(MI355DET_EINVAL, "%s: too many tiles", what);
  const PoolOut O{precision, scores, recall, num_thrs, num_recs, num_pools, num_areas};
  const long long* order = (const long long*)pool_order;
  const long long* npig = (const long long*)pool_npig;
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(pooled_plan_kernel, dim3(1), dim3(WAVE), 0, st, (const long long*)pool_offsets, num_pools, (long long)num_order, W.off,
                     W.tile_base);
  if (tiles > 0)
    hipLaunchKernelGGL(pooled_pack_kernel, dim3((unsigned)tiles), dim3(WAVE), 0, st, W, num_pools, order, (long long)num_dt, dt_match, dt_ignore, C);
  hipLaunchKernelGGL(pooled_scan_kernel, dim3((unsigned)num_pools), dim3(SCAN_WAVES * WAVE), 0, st, W, C);
  if (tiles > 0) hipLaunchKernelGGL(pooled_tilemax_kernel, dim3((unsigned)tiles), dim3(WAVE), 0, st, W, num_pools, C);
  hipLaunchKernelGGL(pooled_finish_kernel, dim3((unsigned)num_pools), dim3(SCAN_WAVES * WAVE), 0, st, W, C, npig, rec_thrs, O);
  if (tiles > 0)
    hipLaunchKernelGGL(pooled_emit_kernel, dim3((unsigned)tiles), dim3(WAVE), (size_t)num_recs * sizeof(double), st, W, num_pools, C, order,
                       (long long)num_dt, dt_score, npig, rec_thrs, O);
  return check_launch(what);
}

}  // extern "C"
