// Every plan-time and launch-time DECISION of the weight gradient (wgrad_kernels.hip), as functions of the shape and plain integers: no HIP
// types, compiles with a host compiler (tests/wgrad_choice_main.cpp prints them; tests/test_wgrad_choice.py checks them against a fixture).
#pragma once
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/mi355det.h"

namespace mi355 {

constexpr int WGC_STEP = 64, WGC_TILE = 128, WGC_TILE8 = 256;      // pixels per k-step; co / n' tile of the two kernels
constexpr int WG_FORM8 = 1 << 16;                                  // + split count = the 256 x 256 phase-staggered kernel
constexpr int WG_SPLITS[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 96, 128, 192, 256, 384, 512, 768, 1024};

struct WgradGeom {
  int M, NP, co_tiles, np_tiles, tiles;      // pixels, k*k*Cin, 128 x 128 tiles
  size_t per_split;                          // slab bytes of one split
  explicit WgradGeom(const mi355det_conv_shape* s)
      : M(s->n * s->ho * s->wo), NP(s->ksize * s->ksize * s->cin), co_tiles((s->cout + WGC_TILE - 1) / WGC_TILE), np_tiles((NP + WGC_TILE - 1) / WGC_TILE),
        tiles(co_tiles * np_tiles), per_split((size_t)tiles * WGC_TILE * WGC_TILE * sizeof(float)) {}
  int chunk_of(int sp) const { return ((M + sp - 1) / sp + WGC_STEP - 1) / WGC_STEP * WGC_STEP; }      // pixels per split: whole k-steps
  bool split_valid(int sp) const { return sp >= 1 && (M + chunk_of(sp) - 1) / chunk_of(sp) == sp; }    // no empty split
};

// room for the largest split count the autotuner may pick: capped at 128 MiB, but never below three splits (the 1204-class cls_logits has
// 100 MB of dW: its 387 tiles of 256 x 256 are 1.5 rounds of 256 CUs with one pixel range and 3.0 with two)
inline size_t wgrad_workspace_bytes(const WgradGeom& g) {
  size_t splits = 1024;
  while (splits > 3 && splits * g.per_split > ((size_t)128 << 20)) --splits;
  return splits * g.per_split;
}

// default when the shape was not autotuned: fill (not exceed) one round of 512 resident workgroups
inline int wgrad_default_splits(const WgradGeom& g) {
  int sp = 512 / (g.tiles > 1 ? g.tiles : 1);
  sp = sp < g.M / 2048 ? sp : g.M / 2048;      // (<= 512 < the 1024 of the candidate list)
  while (sp > 1 && !g.split_valid(sp)) --sp;
  return sp > 1 ? sp : 1;
}

// wgrad8_kernel: pieces of 4 pixels spanning at most two image rows, one wrap per 64-pixel advance, 31-bit byte offsets, at least one whole 256-wide
// tile in both directions (a narrower output would multiply zero fragments: the 128 x 128 kernel is the better tile there; the last co tile
// of a wide output may be partial - the 10 836 channels of the 1204-class cls_logits are 42.3 tiles)
inline bool wgrad_x_fits(const mi355det_conv_shape* s) { return ((long long)s->n * s->h * s->w + (long long)s->pad * (s->w + 1)) * s->in_ld * 2 < 0x7FFFFFF0ll; }
inline bool wgrad8_applicable(const mi355det_conv_shape* s) {
  if (s->wo < 4 || WGC_STEP / s->wo + 1 > s->ho || s->cout < 256 || (long long)s->ksize * s->ksize * s->cin < 256 || s->cin % 8 != 0) return false;
  return wgrad_x_fits(s);
}
// scalar pixel bookkeeping (both kernels): byte offsets into x and into one split's range of dy must fit 31 bits
inline bool wgrad_fits(const mi355det_conv_shape* s, int chunk) { return wgrad_x_fits(s) && (long long)chunk * s->out_ld * 2 < 0x7FFFFFF0ll; }

// The values the tuner times, in timing order: the split counts of the 128 x 128 kernel, then those of the phase-staggered 256 x 256 form
// (one or two whole rounds of one-workgroup-per-CU launches) with WG_FORM8 set.
inline std::vector<int> wgrad_candidates(const mi355det_conv_shape* s, const WgradGeom& g, size_t ws_bytes, bool allow8) {
  std::vector<int> out;
  auto small = [&](int sp) { return sp > 1 && (sp * g.per_split > ws_bytes || g.M / sp < 512); };
  for (int sp : WG_SPLITS)
    if (!small(sp) && !(sp > 1 && (size_t)sp * g.tiles > 4096) && g.split_valid(sp)) out.push_back(sp);
  if (!allow8 || !wgrad8_applicable(s)) return out;
  const int t8 = ((s->cout + WGC_TILE8 - 1) / WGC_TILE8) * ((g.NP + WGC_TILE8 - 1) / WGC_TILE8);
  const int c8[7] = {256 / t8, 512 / t8, 128 / t8, 768 / t8, 1, 2, 3};
  for (int a = 0; a < 7; ++a)      // (split_valid: >= 1)
    if (std::find(c8, c8 + a, c8[a]) == c8 + a && !small(c8[a]) && g.split_valid(c8[a])) out.push_back(c8[a] | WG_FORM8);
  return out;
}

// The tuner's pick from the times (ms) of wgrad_candidates; -1 when nothing was timed.
// Beside the data-gradient stream fewer, longer workgroups and less slab traffic win over the split count that is fastest alone (the step-level
// refinement of round 4 halved the split counts of the big layers: profiles/r04_ab_results.md 7): take the SMALLEST split count within 4 % of
// the fastest one.
inline int wgrad_pick(const int* vals, const float* ms, int n) {
  int best = -1, best8 = -1;
  float best_ms = 1e30f, best8_ms = 1e30f;
  for (int i = 0; i < n; ++i) {
    if (!(vals[i] & WG_FORM8) && ms[i] < best_ms) best_ms = ms[i], best = vals[i];
    if ((vals[i] & WG_FORM8) && ms[i] < best8_ms) best8_ms = ms[i], best8 = vals[i];
  }
  for (int i = n - 1; i >= 0; --i)
    if (!(vals[i] & WG_FORM8) && ms[i] <= best_ms * 1.04f) best = vals[i];
  return best8 > 0 && best8_ms < best_ms * 0.97f ? best8 : best;
}

struct WgradChoice { int splits; bool form8; int chunk; };      // form8 as chosen: the launch runs the 128 x 128 kernel where !wgrad_fits(s, chunk)
struct WgradResolved { int status; WgradChoice choice; char message[200]; };      // status 0: `choice` is launched; else an MI355DET_E* code and its text
inline WgradResolved wgrad_error(int status, const char* fmt, long long b = 0, long long c = 0) {
  WgradResolved r{};
  r.status = status;
  snprintf(r.message, sizeof(r.message), fmt, "conv_wgrad", b, c);
  return r;
}

// What mi355det_conv_wgrad launches: the default, overridden by the tune record (`recorded`, nullptr = none), overridden by debug key 7
// (`force`, 0 = none); strict mode (debug key 9): the forced value is launched as it is or not at all.
inline WgradResolved wgrad_resolve(const mi355det_conv_shape* s, const WgradGeom& g, const int* recorded, int force, bool strict, bool ws_present,
                                   size_t ws_bytes) {
  int splits = recorded ? *recorded & (WG_FORM8 - 1) : wgrad_default_splits(g);
  bool form8 = recorded && (*recorded & WG_FORM8);
  const int fsp = force & (WG_FORM8 - 1);
  if (strict && force > 0) {
    if (!g.split_valid(fsp)) return wgrad_error(MI355DET_EINVAL, "%s: forced split count %lld is not valid for %lld pixels (strict mode, debug key 9)", fsp, g.M);
    if (fsp > 1 && (!ws_present || fsp * g.per_split > ws_bytes))
      return wgrad_error(MI355DET_EINVAL, "%s: forced split count %lld needs %lld workspace bytes (strict mode, debug key 9)", fsp, (long long)(fsp * g.per_split));
  }
  if (force > 0 && g.split_valid(fsp)) {      // (not strict: an invalid forced value is ignored)
    splits = fsp;
    form8 = (force & WG_FORM8) != 0;
  }
  if (splits < 1) splits = 1;
  if ((force & WG_FORM8) && !(form8 && wgrad8_applicable(s)))      // the diagnostic switch must not fall back silently
    return wgrad_error(MI355DET_EINVAL, "%s: the phase-staggered kernel was forced (debug key 7) for a shape or split count it does not take");
  form8 = form8 && wgrad8_applicable(s);      // (a record written for another build: fall back to the 128 x 128 kernel, same split count)
  while (splits > 1 && (splits * g.per_split > ws_bytes || !g.split_valid(splits))) --splits;
  if (form8 && !wgrad_fits(s, g.chunk_of(splits)) && strict && (force & WG_FORM8))
    return wgrad_error(MI355DET_EINVAL, "%s: the forced phase-staggered kernel does not fit the 31-bit offsets of this shape (strict mode, debug key 9)");
  WgradResolved r{};
  r.choice = {splits, form8, g.chunk_of(splits)};
  return r;
}

}  // namespace mi355
