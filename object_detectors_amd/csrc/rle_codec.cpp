// pycocotools rleToString / rleFrString (include/mi355det.h): the compressed `counts` string of a COCO run-length encoding.  Host code only -
// no GPU call, no HIP header - so that it also builds on its own.
//
// Encode: x = counts[i], from the fourth count on minus counts[i-2] (signed); then 5 bits at a time, low group first: c = x & 0x1f,
// x >>= 5 (arithmetic), more = (c & 0x10) ? x != -1 : x != 0, bit 0x20 of c = more, character c + 48.  Decode is the inverse, with sign
// extension when the last group of a count has bit 0x10.
#include <stdint.h>
#include <stdio.h>

#include "../../include/mi355det.h"

namespace mi355 {
extern thread_local char g_err[512];
}

namespace {
int64_t codec_fail(const char* msg, long long a = 0, long long b = 0) {
  snprintf(mi355::g_err, sizeof(mi355::g_err), msg, a, b);
  return MI355DET_EINVAL;
}
}  // namespace

extern "C" {

int64_t mi355det_rle_to_string(const int32_t* counts, int64_t n, char* out, int64_t cap) {
  if (n < 0 || (n > 0 && !counts) || (out && cap < 0)) return codec_fail("rle_to_string: bad arguments");
  int64_t p = 0;
  for (int64_t i = 0; i < n; ++i) {
    long long x = counts[i];
    if (i > 2) x -= counts[i - 2];
    bool more = true;
    while (more) {
      int c = (int)(x & 0x1f);
      x >>= 5;
      more = (c & 0x10) ? x != -1 : x != 0;
      if (more) c |= 0x20;
      if (out) {
        if (p + 1 >= cap) return codec_fail("rle_to_string: cap %lld is too small", cap);      // room for this character and the NUL
        out[p] = (char)(c + 48);
      }
      ++p;
    }
  }
  if (out) {
    if (p >= cap) return codec_fail("rle_to_string: cap %lld is too small", cap);
    out[p] = 0;
  }
  return p;
}

int64_t mi355det_rle_from_string(const char* s, int32_t* counts, int64_t cap) {
  if (!s || (counts && cap < 0)) return codec_fail("rle_from_string: bad arguments");
  int64_t m = 0, p = 0;
  long long before1 = 0, before2 = 0;                 // the counts one and two before the current one
  while (s[p]) {
    long long x = 0;
    int k = 0;
    bool more = true;
    while (more) {
      const int c = (int)(unsigned char)s[p] - 48;
      if (c < 0 || c > 0x3f) return codec_fail("rle_from_string: character %lld at offset %lld is outside the alphabet", c + 48, p);
      if (k > 6) return codec_fail("rle_from_string: a count of more than 7 groups at offset %lld", p);
      x |= (long long)(c & 0x1f) << (5 * k);
      more = (c & 0x20) != 0;
      ++p;
      ++k;
      if (!more && (c & 0x10)) x |= (long long)(~0ull << (5 * k));
    }
    if (m > 2) x += before2;
    if (x < INT32_MIN || x > INT32_MAX) return codec_fail("rle_from_string: count %lld does not fit int32", m);
    if (counts) {
      if (m >= cap) return codec_fail("rle_from_string: cap %lld is too small", cap);
      counts[m] = (int32_t)x;
    }
    before2 = before1;
    before1 = x;
    ++m;
  }
  return m;
}

}  // extern "C"
