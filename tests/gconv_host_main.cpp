// Stand-alone host program for the argument checks, pack sizes and workspace arithmetic of the grouped-convolution entry points
// (csrc/gconv_kernels.hip).  It calls the size and refusal paths only: nothing is launched, no GPU is needed.  Meant for a sanitizer build
// of the host code, from the repository root:
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         -x hip object_detectors_amd/csrc/gconv_kernels.hip object_detectors_amd/csrc/lib.cpp tests/gconv_host_main.cpp -o gconv_host && ./gconv_host
//
// Exit status 0 and the line "gconv host checks ok" mean every expectation held; the sanitizers abort on their own findings.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/mi355det.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      printf("FAILED line %d: %s  [%s]\n", __LINE__, #cond, mi355det_last_error()); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

static mi355det_conv_shape shape(int n, int h, int w, int c, int cout, int k, int stride) {
  mi355det_conv_shape s;
  memset(&s, 0, sizeof(s));
  s.n = n, s.h = h, s.w = w, s.cin = c, s.cout = cout, s.ksize = k, s.stride = stride, s.pad = (k - 1) / 2;
  s.ho = (h + 2 * s.pad - k) / stride + 1, s.wo = (w + 2 * s.pad - k) / stride + 1;
  s.in_ld = c, s.out_ld = cout;
  return s;
}

int main(void) {
  char dummy[64];   // never dereferenced: every call below returns before a launch
  void* p = dummy;
  mi355det_conv_epilogue e;
  memset(&e, 0, sizeof(e));

  // ---- sizes: one operand image is [c / 32][9][kb / 32][2][64][8] bf16 with kb = max(32, channels per group)
  const int cpgs[5] = {4, 8, 16, 32, 64};
  for (int i = 0; i < 5; ++i)
    for (int stride = 1; stride <= 2; ++stride) {
      const int c = cpgs[i] * 32, kb = cpgs[i] == 64 ? 64 : 32;
      mi355det_conv_shape s = shape(2, 13, 19, c, c, 3, stride);
      EXPECT(mi355det_gconv_pack_elems(&s, 32) == (size_t)9 * kb * c);
      // workspace: splits * units * 9 * 32 * 32 floats, units = c / 32 (twice that at 64 channels per group), splits <= pixel tiles
      const size_t unit = (size_t)9 * 32 * 32 * 4, units = (size_t)(c / 32) * (cpgs[i] == 64 ? 2 : 1);
      const size_t tiles = (size_t)2 * ((s.ho + 7) / 8) * ((s.wo + 15) / 16);
      const size_t ws = mi355det_gconv_wgrad_workspace(&s, 32);
      EXPECT(ws > 0 && ws % (unit * units) == 0 && ws / (unit * units) <= tiles && ws / (unit * units) >= 1);
      s.in_ld = c + 3, s.out_ld = c + 5;   // any pitch above the channel count
      EXPECT(mi355det_gconv_pack_elems(&s, 32) == (size_t)9 * kb * c);
      // a workspace one byte short is refused before the launch (the pointers are never touched)
      EXPECT(mi355det_gconv_wgrad(&s, 32, p, p, (float*)p, p, ws - 1, NULL) == MI355DET_EWORKSPACE);
      EXPECT(mi355det_gconv_wgrad(&s, 32, p, p, (float*)p, NULL, 0, NULL) == MI355DET_EWORKSPACE);
    }
  {
    mi355det_conv_shape big = shape(64, 1600, 2688, 2048, 2048, 3, 1);   // workspace stays bounded: at most 1024 partial units (+ rounding)
    EXPECT(mi355det_gconv_wgrad_workspace(&big, 32) <= (size_t)2048 * 9 * 32 * 32 * 4);
  }

  // ---- refusals: MI355DET_EINVAL from every entry point, 0 from the size functions
  mi355det_conv_shape good = shape(1, 8, 8, 256, 256, 3, 1);
  struct {
    mi355det_conv_shape s;
    int groups;
  } bad[12];
  int nb = 0;
  bad[nb].s = good, bad[nb++].groups = 48;                                  // groups does not divide cin
  bad[nb].s = good, bad[nb++].groups = 128;                                 // 2 channels per group
  bad[nb].s = good, bad[nb++].groups = 2;                                   // 128 channels per group
  bad[nb].s = good, bad[nb++].groups = 0;
  bad[nb].s = good, bad[nb++].groups = -4;
  bad[nb].s = shape(1, 8, 8, 256, 256, 1, 1), bad[nb++].groups = 32;        // ksize 1
  bad[nb].s = shape(1, 8, 8, 256, 128, 3, 1), bad[nb++].groups = 32;        // cin != cout
  bad[nb].s = shape(1, 8, 8, 16, 16, 3, 1), bad[nb++].groups = 4;           // cin not a multiple of the 32-channel bundle
  bad[nb].s = good, bad[nb].s.stride = 3, bad[nb++].groups = 32;
  bad[nb].s = good, bad[nb].s.in_ld = 255, bad[nb++].groups = 32;           // pitch below the channel count
  bad[nb].s = good, bad[nb].s.ho = 7, bad[nb++].groups = 32;                // output size that does not match
  bad[nb].s = good, bad[nb].s.n = 0, bad[nb++].groups = 32;
  for (int i = 0; i < nb; ++i) {
    const mi355det_conv_shape* s = &bad[i].s;
    const int g = bad[i].groups;
    EXPECT(mi355det_gconv_pack_elems(s, g) == 0);
    EXPECT(mi355det_gconv_wgrad_workspace(s, g) == 0);
    EXPECT(mi355det_gconv_pack_weights(s, g, (const float*)p, 1, p, p, NULL) == MI355DET_EINVAL);
    EXPECT(mi355det_gconv_fwd_ex(s, g, p, p, &e, p, 0, NULL) == MI355DET_EINVAL);
    EXPECT(mi355det_gconv_dgrad(s, g, p, p, p, NULL) == MI355DET_EINVAL);
    EXPECT(mi355det_gconv_wgrad(s, g, p, p, (float*)p, p, (size_t)1 << 30, NULL) == MI355DET_EINVAL);
    EXPECT(strlen(mi355det_last_error()) > 0);
  }
  EXPECT(mi355det_gconv_pack_elems(NULL, 32) == 0);
  EXPECT(mi355det_gconv_fwd_ex(NULL, 32, p, p, &e, p, 0, NULL) == MI355DET_EINVAL);
  // epilogue forms conv2 of a bottleneck never has
  mi355det_conv_epilogue res = e;
  res.residual = p, res.residual_ld = 256;
  EXPECT(mi355det_gconv_fwd_ex(&good, 32, p, p, &res, p, 0, NULL) == MI355DET_EINVAL);
  EXPECT(mi355det_gconv_fwd_ex(&good, 32, p, p, &e, p, 1, NULL) == MI355DET_EINVAL);
  mi355det_conv_epilogue leaky = e;
  leaky.relu = 2;
  EXPECT(mi355det_gconv_fwd_ex(&good, 32, p, p, &leaky, p, 0, NULL) == MI355DET_EINVAL);
  // null pointers
  EXPECT(mi355det_gconv_fwd_ex(&good, 32, NULL, p, &e, p, 0, NULL) == MI355DET_EINVAL);
  EXPECT(mi355det_gconv_dgrad(&good, 32, p, NULL, p, NULL) == MI355DET_EINVAL);
  EXPECT(mi355det_gconv_pack_weights(&good, 32, (const float*)p, 1, NULL, NULL, NULL) == MI355DET_EINVAL);
  EXPECT(mi355det_gconv_wgrad(&good, 32, p, p, NULL, p, (size_t)1 << 30, NULL) == MI355DET_EINVAL);

  if (failures) {
    printf("%d gconv host check(s) failed\n", failures);
    return 1;
  }
  printf("gconv host checks ok\n");
  return 0;
}
