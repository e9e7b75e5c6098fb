// Result masks from their COCO `counts` strings (include/mi355det.h, "Run lengths from counts strings"): mi355det_rle_from_string
// (csrc/rle_codec.cpp = pycocotools rleFrString) for many strings at once, with the checks and the area / tight box that the evaluators'
// mask store otherwise works out per mask on the host.
//
// One wavefront per mask, grid-stride over the masks.  The mask's bytes go by in chunks of 64 lanes: lanes 0..6 re-read the 7 bytes before
// the chunk (a token has at most 7 characters, so every look-back stays inside the wave), lanes 7..63 own 57 new bytes.  Per chunk:
//   tokens    a byte without bit 0x20 ends a token.  Its lane counts the continuation bytes right before it (a ballot, count-leading-zeros)
//             and rebuilds the token from them with six shuffles; nothing outside str_offsets[k]:str_offsets[k + 1] is ever read.
//   compact   a ballot + popcount gives each token its slot; one permutation (ds_permute: token lanes to their slots, the other lanes
//             behind them) moves token s of the chunk to lane s.
//   counts    count m = token m + count m - 2 for m > 2: an inclusive scan over the lanes of equal parity (strides 2..32), plus the two
//             sums carried from the chunks before.  Token 0 is outside both sums.
//   emit      a scan of the counts gives each run's first pixel; the runs of ones give the area and the tight box (a run that goes on
//             into the next column spans y = 0..h-1).
// The count pass decodes and checks everything (status, tokens per mask); the emit pass decodes again and writes.  Integers only, no
// atomics, one writer per element, 64-bit offsets.
#include "offsets_scan.h"
#include "rle_protocol.h"

#include <limits.h>

using namespace mi355;

namespace {

constexpr int HALO = 7, STEP = WAVE - HALO;
constexpr int WAVES = 4;                               // per block
constexpr long long MAX_CHARS = 1ll << 28;             // per string: keeps every 64-bit sum of 35-bit tokens far from overflow

// EMIT = false: tokens[k] = the mask's number of counts, status[k].  EMIT = true: counts, area, bbox (runs = the scanned tokens).
template <bool EMIT>
__global__ __launch_bounds__(WAVES * WAVE) void rle_strings_kernel(const unsigned char* __restrict__ bytes, long long num_bytes,
                                                                    const long long* __restrict__ str_off, const int* __restrict__ sizes,
                                                                    long long n, long long* __restrict__ tokens,
                                                                    unsigned char* __restrict__ status, const long long* __restrict__ runs,
                                                                    int* __restrict__ counts, long long capacity,
                                                                    long long* __restrict__ area, int* __restrict__ bbox) {
  const int lane = threadIdx.x & (WAVE - 1);
  const unsigned long long below = (1ull << lane) - 1;
  const long long stride = (long long)gridDim.x * WAVES;
  for (long long k = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6); k < n; k += stride) {
    const long long b0 = str_off[k], b1 = str_off[k + 1];
    const int h = sizes[2 * k], w = sizes[2 * k + 1];
    unsigned bad = 0;
    if (b0 < 0 || b1 < b0 || b1 > num_bytes || b1 - b0 > MAX_CHARS) bad |= MI355DET_RLESTR_RANGE;
    if (h < 1 || w < 1 || (long long)h * w >= (1ll << 31)) bad |= MI355DET_RLESTR_SIZE;
    if (bad) {                                         // skipped: no byte is read, no count is owned
      if (lane == 0) {
        if (!EMIT) {
          tokens[k] = 0;
          status[k] = (unsigned char)bad;
        } else {
          if (area) area[k] = 0;
          if (bbox)
            for (int j = 0; j < 4; ++j) bbox[4 * k + j] = 0;
        }
      }
      continue;
    }
    long long out0 = 0, out1 = 0;
    if (EMIT) {
      out0 = runs[k];
      out1 = runs[k + 1];
    }
    long long base = 0, carry_even = 0, carry_odd = 0;   // tokens before the chunk; the two running sums
    unsigned pos = 0;                                    // pixels before the chunk (below 2^31 wherever the status is 0)
    long long total = 0, ones = 0;                       // per lane, reduced after the last chunk
    int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
    bool whole = false;
    for (long long c0 = b0; c0 < b1; c0 += STEP) {
      const long long p = c0 - HALO + lane;
      const bool valid = p >= b0 && p < b1;
      const int c = valid ? (int)bytes[p] - 48 : 0;
      const bool own = valid && lane >= HALO;
      const bool more = valid && (c & 0x20) != 0;
      if (own && (c < 0 || c > 0x3f)) bad |= MI355DET_RLESTR_ALPHABET;
      if (own && more && p == b1 - 1) bad |= MI355DET_RLESTR_OPEN;
      const unsigned long long more_mask = __ballot(more);
      const bool end = own && !more;
      const unsigned long long end_mask = __ballot(end);
      // the continuation bytes right before this lane's byte: bit lane - 1 of more_mask moved to the top, leading ones counted
      const int before = lane > 0 ? __clzll(~(more_mask << (WAVE - lane))) : 0;
      if (own && before >= 7) bad |= MI355DET_RLESTR_LONG;
      const int r = min(before, 6);
      long long x = (long long)(c & 0x1f) << (5 * r);
#pragma unroll
      for (int j = 1; j <= 6; ++j) {
        const int pj = __shfl(c, (lane - j) & (WAVE - 1), WAVE) & 0x1f;
        if (j <= r) x |= (long long)pj << (5 * (r - j));
      }
      if (c & 0x10) x |= (long long)(~0ull << (5 * (r + 1)));
      // token s of the chunk to lane s
      const int T = __popcll(end_mask);
      const int slot = end ? __popcll(end_mask & below) : T + __popcll(~end_mask & below);
      const int lo = __builtin_amdgcn_ds_permute(slot << 2, (int)x), hi = __builtin_amdgcn_ds_permute(slot << 2, (int)(x >> 32));
      const long long tok = ((long long)hi << 32) | (unsigned)lo;
      const bool live = lane < T;
      const long long g = base + lane;                   // the count's index in the mask
      long long v = (live && g > 0) ? tok : 0;
#pragma unroll
      for (int o = 2; o < WAVE; o <<= 1) {
        const long long u = shfl_up_i64(v, o);
        if (lane >= o) v += u;
      }
      v += (g & 1) ? carry_odd : carry_even;
      const long long last1 = shfl_i64(v, (T - 1) & (WAVE - 1)), last2 = shfl_i64(v, (T - 2) & (WAVE - 1));
      if (T >= 2) {
        if ((base + T) & 1) { carry_even = last1; carry_odd = last2; } else { carry_odd = last1; carry_even = last2; }
      } else if (T == 1) {
        if ((base + T) & 1) carry_even = last1; else carry_odd = last1;
      }
      const long long cnt = g == 0 ? tok : v;
      const bool fits = cnt <= INT_MAX && cnt >= INT_MIN;
      if (live) {
        if (!fits) bad |= MI355DET_RLESTR_INT32;
        else if (cnt < 0) bad |= MI355DET_RLESTR_NEGATIVE;
        if (fits) total += cnt;
      }
      if (EMIT) {
        const unsigned cu = live ? (unsigned)cnt : 0u;
        unsigned incl = cu;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
          const unsigned u = (unsigned)__shfl_up((int)incl, o, WAVE);
          if (lane >= o) incl += u;
        }
        const unsigned first = pos + incl - cu;
        pos += (unsigned)__shfl((int)incl, WAVE - 1, WAVE);
        if (live) {
          const long long at = out0 + g;
          if (at < out1 && at < capacity) counts[at] = (int)cnt;
          if ((g & 1) && cnt > 0 && fits) {                     // a run of ones: pixels first .. last in column-major order
            const unsigned last = first + cu - 1, x0 = first / (unsigned)h, x1 = last / (unsigned)h;
            ones += cnt;
            xmin = min(xmin, (int)x0);
            xmax = max(xmax, (int)x1);
            if (x1 > x0) {
              whole = true;
            } else {
              ymin = min(ymin, (int)(first - x0 * (unsigned)h));
              ymax = max(ymax, (int)(last - x1 * (unsigned)h));
            }
          }
        }
      }
      base += T;
    }
    if (!EMIT) {
      total = wave_sum_i64(total);
      bad = wave_or(bad);
      if (total != (long long)h * w) bad |= MI355DET_RLESTR_SUM;
      if (lane == 0) {
        tokens[k] = base;
        status[k] = (unsigned char)bad;
      }
    } else {
      ones = wave_sum_i64(ones);
      xmin = wave_min_i(xmin);
      xmax = wave_max_i(xmax);
      ymin = wave_min_i(ymin);
      ymax = wave_max_i(ymax);
      if (__any(whole)) {
        ymin = 0;
        ymax = h - 1;
      }
      if (lane == 0) {
        const bool any = ones > 0;
        if (area) area[k] = ones;
        if (bbox) {
          bbox[4 * k + 0] = any ? xmin : 0;
          bbox[4 * k + 1] = any ? ymin : 0;
          bbox[4 * k + 2] = any ? xmax - xmin + 1 : 0;
          bbox[4 * k + 3] = any ? ymax - ymin + 1 : 0;
        }
      }
    }
  }
}

// the side count of mi355det_rle_strings_count's scan: the masks with a status
struct HasStatus {
  const unsigned char* status;
  __device__ __forceinline__ bool operator()(long long k) const { return status[k] != 0; }
};

int check_tables(const char* what, const void* bytes, long long num_bytes, const void* str_offsets_dev, const void* sizes, long long n) {
  if (n < 0 || n >= (1ll << 31) || num_bytes < 0) return fail(MI355DET_EINVAL, "%s: bad arguments", what);
  if (n > 0 && (!str_offsets_dev || !sizes || (num_bytes > 0 && !bytes))) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  return MI355DET_OK;
}

inline int grid_for(long long n) { return (int)((n + WAVES - 1) / WAVES < 65536 ? (n + WAVES - 1) / WAVES : 65536); }

}  // namespace

extern "C" {

int mi355det_rle_strings_count(const uint8_t* bytes, int64_t num_bytes, const int64_t* str_offsets, const int64_t* str_offsets_dev,
                               const int32_t* sizes, int64_t n, int64_t* run_offsets, uint8_t* status, int64_t* num_bad, void* stream) {
  const int st = check_tables("rle_strings_count", bytes, num_bytes, str_offsets_dev, sizes, n);
  if (st != MI355DET_OK) return st;
  if (!str_offsets || !run_offsets || !num_bad || (n > 0 && !status)) return fail(MI355DET_EINVAL, "%s: missing operand", "rle_strings_count");
  if (str_offsets[0] != 0 || str_offsets[n] != num_bytes)
    return fail(MI355DET_EINVAL, "%s: str_offsets must run from 0 to num_bytes = %lld", "rle_strings_count", num_bytes);
  for (int64_t k = 0; k < n; ++k) {
    if (str_offsets[k + 1] < str_offsets[k]) return fail(MI355DET_EINVAL, "%s: str_offsets descend at mask %lld", "rle_strings_count", k);
    if (str_offsets[k + 1] - str_offsets[k] > MAX_CHARS)
      return fail(MI355DET_EINVAL, "%s: the string of mask %lld has more than 2^28 characters", "rle_strings_count", k);
  }
  if (n > 0)
    hipLaunchKernelGGL(rle_strings_kernel<false>, dim3(grid_for(n)), dim3(WAVES * WAVE), 0, S(stream), bytes, (long long)num_bytes,
                       (const long long*)str_offsets_dev, sizes, (long long)n, (long long*)run_offsets, status, (const long long*)nullptr,
                       (int*)nullptr, 0ll, (long long*)nullptr, (int*)nullptr);
  launch_offsets_scan(n, ScanInPlace{(const long long*)run_offsets}, (long long*)run_offsets, stream, HasStatus{status}, (long long*)num_bad);
  return check_launch("rle_strings_count");
}

int mi355det_rle_strings_emit(const uint8_t* bytes, int64_t num_bytes, const int64_t* str_offsets_dev, const int32_t* sizes, int64_t n,
                              const int64_t* run_offsets, int64_t total_runs, int32_t* counts, int64_t capacity, int64_t* area,
                              int32_t* bbox, void* stream) {
  const int st = check_tables("rle_strings_emit", bytes, num_bytes, str_offsets_dev, sizes, n);
  if (st != MI355DET_OK) return st;
  if (n == 0) return MI355DET_OK;
  const int ce = check_emit("rle_strings_emit", "%s: total_runs %lld is negative", 0, total_runs, capacity, run_offsets, counts);
  if (ce != MI355DET_OK) return ce;
  hipLaunchKernelGGL(rle_strings_kernel<true>, dim3(grid_for(n)), dim3(WAVES * WAVE), 0, S(stream), bytes, (long long)num_bytes,
                     (const long long*)str_offsets_dev, sizes, (long long)n, (long long*)nullptr, (unsigned char*)nullptr,
                     (const long long*)run_offsets, counts, (long long)capacity, (long long*)area, bbox);
  return check_launch("rle_strings_emit");
}

}  // extern "C"
