// Grouped 3x3 convolution (ResNeXt conv2: utilities/resnet.py Bottleneck with groups > 1): forward, data gradient, weight gradient.
// NHWC bf16 activations, fp32 accumulation on MFMA 16x16x32, gfx950 only.  DESIGN.md section 4.9.
//
// A workgroup owns a tile of output pixels (TH rows x 16 columns) times a BUNDLE of 32 output channels.  The bundle's input channels are
// the KB = max(32, channels per group) channels its groups read; the tile's input halo of those channels is staged in LDS once and the
// nine taps run on it as a small block-diagonal dense product: the packed weight image holds zeros outside the groups, so a bundle of
// eight 4-channel groups does 8 x the true arithmetic and the layer still moves every byte once.
//   forward / data gradient   one kernel; the data gradient is the forward of the flipped, transposed weight image, for stride 2 over
//                             the zero-upsampled dy (built while staging: nothing upsampled ever exists in memory)
//   weight gradient           pixels are the reduction axis: per 32 x 32 channel unit a workgroup walks a fixed range of pixel tiles, its
//                             four waves each take 32 pixels of a tile, their sums are folded in wave order through LDS and go to the
//                             workspace with plain stores; a second kernel adds the partials in split order and keeps the in-group
//                             entries.  No atomics anywhere: two calls give the same bits.
// Stores go through plain global pointers (no buffer stores: tests/test_isa_hazards.py).
#include "mfma_prims.h"

namespace mi355 {
namespace {

constexpr int GC_TW = 16;      // output tile width = one MFMA column block
constexpr int GC_LP = 8;       // LDS pixel pitch padding (elements): 80 / 144 byte pitches spread 16-byte reads over the banks
constexpr int GC_THREADS = 256;

struct GcGeom {
  int groups, cpg, c, kb, nb;  // kb = input channels of a bundle (32 | 64), nb = c / 32 bundles
};

// ------------------------------------------------------------------------------------------------ host: argument checks
int gc_check(const mi355det_conv_shape* s, int32_t groups, GcGeom* g, const char* what) {
  if (!s) return fail(MI355DET_EINVAL, "%s: null shape", what);
  if (s->ksize != 3 || s->pad != 1 || (s->stride != 1 && s->stride != 2))
    return fail(MI355DET_EINVAL, "%s: grouped convolution is 3x3, pad 1, stride 1 or 2 (ksize %lld, stride %lld)", what, s->ksize, s->stride);
  if (s->cin != s->cout || s->cin <= 0) return fail(MI355DET_EINVAL, "%s: grouped convolution needs cin == cout (%lld, %lld)", what, s->cin, s->cout);
  if (groups <= 0 || s->cin % groups) return fail(MI355DET_EINVAL, "%s: groups %lld does not divide cin %lld", what, groups, s->cin);
  const int cpg = s->cin / groups;
  if (cpg != 4 && cpg != 8 && cpg != 16 && cpg != 32 && cpg != 64)
    return fail(MI355DET_EINVAL, "%s: channels per group must be 4, 8, 16, 32 or 64 (got %lld)", what, cpg);
  if (s->cin % 32) return fail(MI355DET_EINVAL, "%s: cin %lld is not a multiple of the 32-channel bundle", what, s->cin);
  if (s->n <= 0 || s->h <= 0 || s->w <= 0) return fail(MI355DET_EINVAL, "%s: empty input", what);
  if (s->ho != (s->h - 1) / s->stride + 1 || s->wo != (s->w - 1) / s->stride + 1)
    return fail(MI355DET_EINVAL, "%s: output size does not match the input (ho %lld, wo %lld)", what, s->ho, s->wo);
  if (s->in_ld < s->cin || s->out_ld < s->cout) return fail(MI355DET_EINVAL, "%s: pixel pitch below the channel count", what);
  g->groups = groups;
  g->cpg = cpg;
  g->c = s->cin;
  g->kb = cpg == 64 ? 64 : 32;
  g->nb = s->cin / 32;
  return MI355DET_OK;
}

inline bool vec16(const void* p, int ld) { return ((uintptr_t)p % 16 == 0) && (ld % 8 == 0); }

// ------------------------------------------------------------------------------------------------ weight images
// Forward image: [bundle][tap][k-step][m-tile][lane][8]: the A fragment of one MFMA is one 16-byte load per lane.  Row r of m-tile mt is
// output channel bundle*32 + (r / 4) * 8 + mt * 4 + r % 4, so that the eight accumulator values a lane holds for a pixel (two m-tiles x four
// rows) are eight CONSECUTIVE channels: one 16-byte store.  k = k-step * 32 + (lane / 16) * 8 + e is input channel kbase + k.
// Data-gradient image: the same with the roles of input and output channel exchanged and the taps flipped.
struct GcPackParams {
  const float* w;
  bf16_t* img[2];
  int c, cpg, kb, nb, ohwi;
  long long frags;   // fragments (lane x 8 elements) per image
};

__global__ void __launch_bounds__(256) gconv_pack_kernel(GcPackParams p) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int which = blockIdx.y;
  bf16_t* img = p.img[which];
  if (t >= p.frags || img == nullptr) return;
  const int lane = (int)(t & 63), fr = lane & 15, fq = lane >> 4;
  long long q = t >> 6;
  const int ks_n = p.kb / 32;
  const int mt = (int)(q & 1);
  q >>= 1;
  const int ks = (int)(q % ks_n);
  q /= ks_n;
  const int tap = (int)(q % 9);
  const int b = (int)(q / 9);
  const int rowc = b * 32 + (fr >> 2) * 8 + mt * 4 + (fr & 3);
  const int kbase = (b * 32 / p.kb) * p.kb;
  const int g = rowc / p.cpg;
  unsigned short v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int kc = kbase + ks * 32 + fq * 8 + e;
    float val = 0.f;
    if (kc / p.cpg == g) {
      // forward: row = output channel, k = input channel, tap as is; data gradient: row = input channel, k = output channel, tap flipped
      const int co = which == 0 ? rowc : kc;
      const int cil = (which == 0 ? kc : rowc) - g * p.cpg;
      const int tp = which == 0 ? tap : 8 - tap;
      val = p.ohwi ? p.w[((long long)co * 9 + tp) * p.cpg + cil] : p.w[((long long)co * p.cpg + cil) * 9 + tp];
    }
    v[e] = f2bf(val);
  }
  uint4 u;
  u.x = v[0] | ((unsigned)v[1] << 16);
  u.y = v[2] | ((unsigned)v[3] << 16);
  u.z = v[4] | ((unsigned)v[5] << 16);
  u.w = v[6] | ((unsigned)v[7] << 16);
  *(uint4*)(img + t * 8) = u;
}

// ------------------------------------------------------------------------------------------------ forward / data gradient
struct GcFwdParams {
  const bf16_t* x;      // source map [n, hs, ws, .] with pixel pitch x_ld
  const bf16_t* w;      // weight image
  bf16_t* y;            // [n, ho, wo, .] with pixel pitch y_ld
  const float* scale;
  const float* shift;
  int hs, ws;           // source map
  int hv, wv;           // the map the taps walk: the source, or (UP) its zero-upsampled form cut to the dx size
  int ho, wo;
  int x_ld, y_ld;
  int nb, tiles_x, tiles_y;
  int relu, x_vec, y_vec;
};

__device__ __forceinline__ uint4 gc_load8(const bf16_t* p, int vec) {
  if (vec) return *(const uint4*)p;
  uint4 u;
  u.x = p[0] | ((unsigned)p[1] << 16);
  u.y = p[2] | ((unsigned)p[3] << 16);
  u.z = p[4] | ((unsigned)p[5] << 16);
  u.w = p[6] | ((unsigned)p[7] << 16);
  return u;
}

// KB: input channels per bundle; STRIDE: of the taps over the staged map; UP: the staged map is the source zero-upsampled by two
// (stride-2 data gradient); TH: output rows per tile (a multiple of 4: each wave owns TH / 4 rows)
template <int KB, int STRIDE, int UP, int TH>
__global__ void __launch_bounds__(GC_THREADS) gconv_fwd_kernel(GcFwdParams p) {
  constexpr int HH = (TH - 1) * STRIDE + 3, HW = (GC_TW - 1) * STRIDE + 3;
  constexpr int PITCH = KB + GC_LP, PIECES = KB / 8, KS = KB / 32, NT = TH / 4;
  __shared__ __attribute__((aligned(16))) bf16_t sx[HH * HW * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int bundle = blockIdx.x % p.nb;
  int tile = blockIdx.x / p.nb;
  const int tx = tile % p.tiles_x;
  tile /= p.tiles_x;
  const int ty = tile % p.tiles_y;
  const int img = tile / p.tiles_y;
  const int oh0 = ty * TH, ow0 = tx * GC_TW;
  const int ih0 = oh0 * STRIDE - 1, iw0 = ow0 * STRIDE - 1;
  const int kbase = (bundle * 32 / KB) * KB;

  // ---- stage the halo: every staged position is written (zeros outside the map and, UP, between the samples)
  for (int i = tid; i < HH * HW * PIECES; i += GC_THREADS) {
    const int pix = i / PIECES, piece = i % PIECES;
    const int r = pix / HW, cc = pix % HW;
    const int ih = ih0 + r, iw = iw0 + cc;
    uint4 u = make_uint4(0, 0, 0, 0);
    if (ih >= 0 && iw >= 0 && ih < p.hv && iw < p.wv) {
      int sh = ih, sw = iw;
      bool ok = true;
      if (UP) {
        ok = !((ih | iw) & 1);
        sh = ih >> 1;
        sw = iw >> 1;
        ok = ok && sh < p.hs && sw < p.ws;
      }
      if (ok) u = gc_load8(p.x + (((long long)img * p.hs + sh) * p.ws + sw) * p.x_ld + kbase + piece * 8, p.x_vec);
    }
    *(uint4*)(sx + pix * PITCH + piece * 8) = u;
  }
  __syncthreads();

  f32x4_t acc[NT][2];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[j][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const bf16_t* wb = p.w + (long long)bundle * 9 * KS * 2 * 64 * 8 + lane * 8;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int kh = tap / 3, kw = tap % 3;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      st16x8_t wf[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) wf[mt] = *(const st16x8_t*)(wb + ((tap * KS + ks) * 2 + mt) * 64 * 8);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int r = wave * NT + j;
        const st16x8_t xf = *(const st16x8_t*)(sx + ((r * STRIDE + kh) * HW + fr * STRIDE + kw) * PITCH + ks * 32 + fq * 8);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[j][mt] = MI355_MFMA_16x16x32(wf[mt], xf, acc[j][mt]);
      }
    }
  }

  // ---- epilogue: a lane holds channels c0 .. c0 + 7 of pixel (oh, ow0 + fr)
  const int c0 = bundle * 32 + fq * 8;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = p.scale ? p.scale[c0 + e] : 1.f;
    sh[e] = p.shift ? p.shift[c0 + e] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int oh = oh0 + wave * NT + j, ow = ow0 + fr;
    if (oh >= p.ho || ow >= p.wo) continue;
    unsigned short v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float z = acc[j][e >> 2][e & 3] * sc[e] + sh[e];
      if (p.relu) z = fmaxf(z, 0.f);
      v[e] = f2bf(z);
    }
    bf16_t* dst = p.y + (((long long)img * p.ho + oh) * p.wo + ow) * p.y_ld + c0;
    if (p.y_vec) {
      uint4 u;
      u.x = v[0] | ((unsigned)v[1] << 16);
      u.y = v[2] | ((unsigned)v[3] << 16);
      u.z = v[4] | ((unsigned)v[5] << 16);
      u.w = v[6] | ((unsigned)v[7] << 16);
      *(uint4*)dst = u;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[e] = v[e];
    }
  }
}

template <int KB, int STRIDE, int UP, int TH>
int gc_launch_fwd(GcFwdParams p, int n, hipStream_t st, const char* what) {
  p.tiles_x = (p.wo + GC_TW - 1) / GC_TW;
  p.tiles_y = (p.ho + TH - 1) / TH;
  const long long blocks = (long long)n * p.tiles_x * p.tiles_y * p.nb;
  if (blocks > 0x7fffffffll) return fail(MI355DET_EINVAL, "%s: too many tiles", what);
  hipLaunchKernelGGL((gconv_fwd_kernel<KB, STRIDE, UP, TH>), dim3((unsigned)blocks), dim3(GC_THREADS), 0, st, p);
  return check_launch(what);
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int GW_TH = 8;                 // output rows per pixel tile: 8 x 16 = 128 pixels = four k-steps of 32, one per wave
constexpr int GW_P = 32 + GC_LP;         // LDS pixel pitch (elements)
constexpr int GW_UNIT = 9 * 32 * 32;     // fp32 partial of one unit: [tap][co 32][ci 32]

struct GcWgParams {
  const bf16_t* x;
  const bf16_t* dy;
  float* part;           // [split][unit][9][32][32]
  int h, w, ho, wo;
  int x_ld, dy_ld;
  int units, uh;         // uh: units per bundle of 32 output channels (2 when a group has 64 channels, else 1)
  int tiles_x, tiles_y, ntiles, splits;
  int x_vec, dy_vec;
};

template <int STRIDE>
__global__ void __launch_bounds__(GC_THREADS) gconv_wgrad_kernel(GcWgParams p) {
  constexpr int HH = (GW_TH - 1) * STRIDE + 3, HW = (GC_TW - 1) * STRIDE + 3;
  constexpr int SX = HH * HW * GW_P * 2, SDY = GW_TH * GC_TW * GW_P * 2, RED = 144 * 64 * 4;
  constexpr int SMEM = SX + SDY > RED ? SX + SDY : RED;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  bf16_t* sx = (bf16_t*)smem;
  bf16_t* sdy = (bf16_t*)(smem + SX);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int unit = blockIdx.x % p.units, split = blockIdx.x / p.units;
  const int co0 = (unit / p.uh) * 32;
  const int ci0 = p.uh == 2 ? (co0 / 64) * 64 + (unit & 1) * 32 : co0;
  const int t0 = (int)((long long)split * p.ntiles / p.splits), t1 = (int)((long long)(split + 1) * p.ntiles / p.splits);

  f32x4_t acc[9][2][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[t][a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // this wave's 32 pixels of a tile: k = fq * 8 + e -> row 2 * wave + fq / 2, column (fq % 2) * 8 + e
  const int prow = 2 * wave + (fq >> 1), pcol = (fq & 1) * 8;
#pragma nounroll
  for (int tile = t0; tile < t1; ++tile) {
    int q = tile;
    const int tx = q % p.tiles_x;
    q /= p.tiles_x;
    const int ty = q % p.tiles_y;
    const int img = q / p.tiles_y;
    const int oh0 = ty * GW_TH, ow0 = tx * GC_TW;
    const int ih0 = oh0 * STRIDE - 1, iw0 = ow0 * STRIDE - 1;
    __syncthreads();          // the previous tile's fragments are read
    for (int i = tid; i < HH * HW * 4; i += GC_THREADS) {
      const int pix = i >> 2, piece = i & 3;
      const int ih = ih0 + pix / HW, iw = iw0 + pix % HW;
      uint4 u = make_uint4(0, 0, 0, 0);
      if (ih >= 0 && iw >= 0 && ih < p.h && iw < p.w)
        u = gc_load8(p.x + (((long long)img * p.h + ih) * p.w + iw) * p.x_ld + ci0 + piece * 8, p.x_vec);
      *(uint4*)(sx + pix * GW_P + piece * 8) = u;
    }
    for (int i = tid; i < GW_TH * GC_TW * 4; i += GC_THREADS) {
      const int pix = i >> 2, piece = i & 3;
      const int oh = oh0 + pix / GC_TW, ow = ow0 + pix % GC_TW;
      uint4 u = make_uint4(0, 0, 0, 0);
      if (oh < p.ho && ow < p.wo) u = gc_load8(p.dy + (((long long)img * p.ho + oh) * p.wo + ow) * p.dy_ld + co0 + piece * 8, p.dy_vec);
      *(uint4*)(sdy + pix * GW_P + piece * 8) = u;
    }
    __syncthreads();
    // A = dy^T (rows = output channel), B = x (columns = input channel), k = pixel: eight 2-byte LDS reads per fragment
    st16x8_t af[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      unsigned short v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = sdy[(prow * GC_TW + pcol + e) * GW_P + mt * 16 + fr];
      uint4 u;
      u.x = v[0] | ((unsigned)v[1] << 16);
      u.y = v[2] | ((unsigned)v[3] << 16);
      u.z = v[4] | ((unsigned)v[5] << 16);
      u.w = v[6] | ((unsigned)v[7] << 16);
      af[mt] = __builtin_bit_cast(st16x8_t, u);
    }
    // the three taps of a kernel row read overlapping columns: e * STRIDE + kw covers NV = 7 * STRIDE + 3 distinct ones, each read once
    constexpr int NV = 7 * STRIDE + 3;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        unsigned short v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = sx[((prow * STRIDE + kh) * HW + pcol * STRIDE + i) * GW_P + nt * 16 + fr];
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          uint4 u;
          u.x = v[kw] | ((unsigned)v[STRIDE + kw] << 16);
          u.y = v[2 * STRIDE + kw] | ((unsigned)v[3 * STRIDE + kw] << 16);
          u.z = v[4 * STRIDE + kw] | ((unsigned)v[5 * STRIDE + kw] << 16);
          u.w = v[6 * STRIDE + kw] | ((unsigned)v[7 * STRIDE + kw] << 16);
          const st16x8_t bfm = __builtin_bit_cast(st16x8_t, u);
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) acc[kh * 3 + kw][mt][nt] = MI355_MFMA_16x16x32(af[mt], bfm, acc[kh * 3 + kw][mt][nt]);
        }
      }
    }
  }

  // ---- fold the four waves in wave order (1, 2, 3 into 0) through LDS, then plain stores of the partial
  float* red = (float*)smem;
#pragma unroll 1
  for (int wv = 1; wv < 4; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[(((t * 2 + a) * 2 + b) * 4 + i) * 64 + lane] = acc[t][a][b][i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][a][b][i] += red[(((t * 2 + a) * 2 + b) * 4 + i) * 64 + lane];
    }
  }
  if (wave == 0) {
    float* dst = p.part + ((long long)split * p.units + unit) * GW_UNIT;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[t * 1024 + (a * 16 + fq * 4 + i) * 32 + b * 16 + fr] = acc[t][a][b][i];
  }
}

// dw[co][tap][cil] = sum over the splits, in split order, of the in-group entry of the unit partial
__global__ void __launch_bounds__(256) gconv_wgrad_reduce_kernel(const float* part, float* dw, int c, int cpg, int units, int uh, int splits) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)c * 9 * cpg) return;
  const int cil = (int)(idx % cpg);
  const int tap = (int)((idx / cpg) % 9);
  const int co = (int)(idx / (9 * cpg));
  int unit, col;
  if (uh == 2) {
    unit = (co / 32) * 2 + cil / 32;
    col = cil % 32;
  } else {
    unit = co / 32;
    col = ((co % 32) / cpg) * cpg + cil;
  }
  const float* src = part + (long long)unit * GW_UNIT + tap * 1024 + (co % 32) * 32 + col;
  float sum = 0.f;
  for (int s = 0; s < splits; ++s) sum += src[(long long)s * units * GW_UNIT];
  dw[idx] = sum;
}

struct GcWgPlan {
  int units, uh, tiles_x, tiles_y, ntiles, splits;
  size_t bytes;
};

// split count: a function of the shape alone (the summation order is part of the result)
int gc_wgrad_plan(const mi355det_conv_shape* s, const GcGeom& g, GcWgPlan* pl) {
  pl->uh = g.cpg == 64 ? 2 : 1;
  pl->units = g.nb * pl->uh;
  pl->tiles_x = (s->wo + GC_TW - 1) / GC_TW;
  pl->tiles_y = (s->ho + GW_TH - 1) / GW_TH;
  const long long nt = (long long)s->n * pl->tiles_x * pl->tiles_y;
  if (nt > 0x3fffffffll) return MI355DET_EINVAL;
  pl->ntiles = (int)nt;
  int sp = (1024 + pl->units - 1) / pl->units;
  if (sp > pl->ntiles) sp = pl->ntiles;
  if (sp < 1) sp = 1;
  pl->splits = sp;
  pl->bytes = (size_t)sp * pl->units * GW_UNIT * sizeof(float);
  return MI355DET_OK;
}

}  // namespace
}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355det_gconv_pack_elems(const mi355det_conv_shape* s, int32_t groups) {
  GcGeom g;
  if (gc_check(s, groups, &g, "gconv_pack_elems") != MI355DET_OK) return 0;
  return (size_t)9 * g.kb * g.c;      // per image: [c / 32 bundles][9][kb / 32][2][64][8]
}

int mi355det_gconv_pack_weights(const mi355det_conv_shape* s, int32_t groups, const float* w, int w_is_ohwi, void* w_fwd, void* w_dgrad,
                                void* stream) {
  GcGeom g;
  int st = gc_check(s, groups, &g, "gconv_pack_weights");
  if (st != MI355DET_OK) return st;
  if (!w || (!w_fwd && !w_dgrad)) return fail(MI355DET_EINVAL, "%s: null pointer", "gconv_pack_weights");
  GcPackParams p;
  p.w = w;
  p.img[0] = (bf16_t*)w_fwd;
  p.img[1] = (bf16_t*)w_dgrad;
  p.c = g.c;
  p.cpg = g.cpg;
  p.kb = g.kb;
  p.nb = g.nb;
  p.ohwi = w_is_ohwi ? 1 : 0;
  p.frags = (long long)9 * g.kb * g.c / 8;
  hipLaunchKernelGGL(gconv_pack_kernel, dim3((unsigned)((p.frags + 255) / 256), 2), dim3(256), 0, S(stream), p);
  return check_launch("gconv_pack_weights");
}

int mi355det_gconv_fwd_ex(const mi355det_conv_shape* s, int32_t groups, const void* x, const void* w_fwd, const mi355det_conv_epilogue* e,
                          void* y, int out_f32, void* stream) {
  GcGeom g;
  int st = gc_check(s, groups, &g, "gconv_fwd_ex");
  if (st != MI355DET_OK) return st;
  if (!x || !w_fwd || !y) return fail(MI355DET_EINVAL, "%s: null pointer", "gconv_fwd_ex");
  if (out_f32) return fail(MI355DET_EINVAL, "%s: fp32 output is not supported", "gconv_fwd_ex");
  if (e && e->residual) return fail(MI355DET_EINVAL, "%s: a residual is not supported", "gconv_fwd_ex");
  if (e && e->relu != 0 && e->relu != 1) return fail(MI355DET_EINVAL, "%s: relu must be 0 or 1 (got %lld)", "gconv_fwd_ex", e->relu);
  GcFwdParams p;
  p.x = (const bf16_t*)x;
  p.w = (const bf16_t*)w_fwd;
  p.y = (bf16_t*)y;
  p.scale = e ? e->scale : nullptr;
  p.shift = e ? e->shift : nullptr;
  p.relu = e ? e->relu : 0;
  p.hs = p.hv = s->h;
  p.ws = p.wv = s->w;
  p.ho = s->ho;
  p.wo = s->wo;
  p.x_ld = s->in_ld;
  p.y_ld = s->out_ld;
  p.nb = g.nb;
  p.x_vec = vec16(x, s->in_ld);
  p.y_vec = vec16(y, s->out_ld);
  hipStream_t hs = S(stream);
  if (s->stride == 1) return g.kb == 32 ? gc_launch_fwd<32, 1, 0, 8>(p, s->n, hs, "gconv_fwd_ex") : gc_launch_fwd<64, 1, 0, 8>(p, s->n, hs, "gconv_fwd_ex");
  return g.kb == 32 ? gc_launch_fwd<32, 2, 0, 4>(p, s->n, hs, "gconv_fwd_ex") : gc_launch_fwd<64, 2, 0, 4>(p, s->n, hs, "gconv_fwd_ex");
}

int mi355det_gconv_dgrad(const mi355det_conv_shape* s, int32_t groups, const void* dy, const void* w_dgrad, void* dx, void* stream) {
  GcGeom g;
  int st = gc_check(s, groups, &g, "gconv_dgrad");
  if (st != MI355DET_OK) return st;
  if (!dy || !w_dgrad || !dx) return fail(MI355DET_EINVAL, "%s: null pointer", "gconv_dgrad");
  GcFwdParams p;
  p.x = (const bf16_t*)dy;
  p.w = (const bf16_t*)w_dgrad;
  p.y = (bf16_t*)dx;
  p.scale = p.shift = nullptr;
  p.relu = 0;
  p.hs = s->ho;
  p.ws = s->wo;
  p.hv = s->h;          // stride 1: ho == h; stride 2: the upsampled dy, cut to the dx map
  p.wv = s->w;
  p.ho = s->h;
  p.wo = s->w;
  p.x_ld = s->out_ld;
  p.y_ld = s->in_ld;
  p.nb = g.nb;
  p.x_vec = vec16(dy, s->out_ld);
  p.y_vec = vec16(dx, s->in_ld);
  hipStream_t hs = S(stream);
  if (s->stride == 1) return g.kb == 32 ? gc_launch_fwd<32, 1, 0, 8>(p, s->n, hs, "gconv_dgrad") : gc_launch_fwd<64, 1, 0, 8>(p, s->n, hs, "gconv_dgrad");
  return g.kb == 32 ? gc_launch_fwd<32, 1, 1, 8>(p, s->n, hs, "gconv_dgrad") : gc_launch_fwd<64, 1, 1, 8>(p, s->n, hs, "gconv_dgrad");
}

size_t mi355det_gconv_wgrad_workspace(const mi355det_conv_shape* s, int32_t groups) {
  GcGeom g;
  GcWgPlan pl;
  if (gc_check(s, groups, &g, "gconv_wgrad_workspace") != MI355DET_OK || gc_wgrad_plan(s, g, &pl) != MI355DET_OK) return 0;
  return pl.bytes;
}

int mi355det_gconv_wgrad(const mi355det_conv_shape* s, int32_t groups, const void* x, const void* dy, float* dw, void* workspace,
                         size_t workspace_bytes, void* stream) {
  GcGeom g;
  GcWgPlan pl;
  int st = gc_check(s, groups, &g, "gconv_wgrad");
  if (st != MI355DET_OK) return st;
  if (gc_wgrad_plan(s, g, &pl) != MI355DET_OK) return fail(MI355DET_EINVAL, "%s: too many tiles", "gconv_wgrad");
  if (!x || !dy || !dw) return fail(MI355DET_EINVAL, "%s: null pointer", "gconv_wgrad");
  if (!workspace || workspace_bytes < pl.bytes)
    return fail(MI355DET_EWORKSPACE, "%s: workspace of %lld bytes needed, %lld given", "gconv_wgrad", (long long)pl.bytes, (long long)workspace_bytes);
  GcWgParams p;
  p.x = (const bf16_t*)x;
  p.dy = (const bf16_t*)dy;
  p.part = (float*)workspace;
  p.h = s->h;
  p.w = s->w;
  p.ho = s->ho;
  p.wo = s->wo;
  p.x_ld = s->in_ld;
  p.dy_ld = s->out_ld;
  p.units = pl.units;
  p.uh = pl.uh;
  p.tiles_x = pl.tiles_x;
  p.tiles_y = pl.tiles_y;
  p.ntiles = pl.ntiles;
  p.splits = pl.splits;
  p.x_vec = vec16(x, s->in_ld);
  p.dy_vec = vec16(dy, s->out_ld);
  hipStream_t hs = S(stream);
  const unsigned blocks = (unsigned)(pl.units * pl.splits);
  if (s->stride == 1) hipLaunchKernelGGL(gconv_wgrad_kernel<1>, dim3(blocks), dim3(GC_THREADS), 0, hs, p);
  else hipLaunchKernelGGL(gconv_wgrad_kernel<2>, dim3(blocks), dim3(GC_THREADS), 0, hs, p);
  st = check_launch("gconv_wgrad");
  if (st != MI355DET_OK) return st;
  const long long elems = (long long)g.c * 9 * g.cpg;
  hipLaunchKernelGGL(gconv_wgrad_reduce_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, hs, (const float*)workspace, dw, g.c, g.cpg,
                     pl.units, pl.uh, pl.splits);
  return check_launch("gconv_wgrad");
}

}  // extern "C"
