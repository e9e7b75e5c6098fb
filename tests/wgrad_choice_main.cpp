// Prints the weight gradient's host decisions (object_detectors_amd/csrc/wgrad_choice.h) for tests/test_wgrad_choice.py.  No GPU, no HIP.
//   T a0 .. a27 b0 .. b6                                   a set of times (ms): a_i for the i-th 128 x 128 candidate, b_i for the i-th 256 x 256 one
//   S n h w cin ho wo cout ksize stride pad in_ld out_ld   one JSON line: geometry, then per workspace the candidates, the pick per time set and the
//                                                          resolver's outcome for strict x record x debug key 7
//   R <shape> ws_bytes ws_present record force strict      one JSON string: a single outcome (record < 0: none)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../object_detectors_amd/csrc/wgrad_choice.h"

using namespace mi355;

static const int RECORDS[] = {-1, 1, 5, 5 | WG_FORM8, 1000}, FORCES[] = {0, 4, 10, 3 | WG_FORM8};

static std::string outcome(const mi355det_conv_shape* s, const WgradGeom& g, int record, int force, bool strict, bool ws_present, size_t ws_bytes) {
  const WgradResolved r = wgrad_resolve(s, g, record < 0 ? nullptr : &record, force, strict, ws_present, ws_bytes);
  char b[320];
  if (r.status) {
    snprintf(b, sizeof(b), "err %d %s", r.status, r.message);
  } else {      // what wgrad_launch runs: splits, chunk, kernel, the scalar pixel bookkeeping (x: the map is too narrow for it anyway), fold: 0 none, 1 wgrad_reduce_kernel, 2 wgrad_reduce8_kernel
    const WgradChoice& c = r.choice;
    const bool fits = wgrad_fits(s, c.chunk), k8 = c.form8 && fits;
    snprintf(b, sizeof(b), "ok %d %d k%d %s f%d", c.splits, c.chunk, k8 ? 256 : 128, k8 || (s->wo >= 4 && WGC_STEP / s->wo + 1 <= s->ho) ? (fits ? "1" : "0") : "x",
             c.splits == 1 ? 0 : (c.splits < 8 ? 1 : 2));
  }
  return b;
}

int main() {
  std::vector<std::vector<float>> times;
  char line[4096];
  while (fgets(line, sizeof(line), stdin)) {
    char* q = line + 1;
    if (line[0] == 'T') {
      times.emplace_back();
      for (int i = 0; i < 35; ++i) times.back().push_back(strtof(q, &q));
      continue;
    }
    if (line[0] != 'S' && line[0] != 'R') continue;
    int32_t v[12];
    for (int i = 0; i < 12; ++i) v[i] = (int32_t)strtol(q, &q, 10);
    const mi355det_conv_shape s = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]};
    const WgradGeom g(&s);
    if (line[0] == 'R') {
      const size_t ws = (size_t)strtoull(q, &q, 10);
      const long a[4] = {strtol(q, &q, 10), strtol(q, &q, 10), strtol(q, &q, 10), strtol(q, &q, 10)};
      printf("\"%s\"\n", outcome(&s, g, (int)a[1], (int)a[2], a[3] != 0, a[0] != 0, ws).c_str());
      continue;
    }
    printf("{\"geom\": [%d, %d, %d, %d, %d, %zu, %zu, %d, %d], \"valid\": [", g.M, g.NP, g.co_tiles, g.np_tiles, g.tiles, g.per_split, wgrad_workspace_bytes(g),
           wgrad_default_splits(g), (int)wgrad8_applicable(&s));
    const char* sep = "";
    for (int sp : WG_SPLITS)
      if (g.split_valid(sp)) printf("%s%d", sep, sp), sep = ", ";
    printf("], \"ws\": [");
    const size_t sizes[3] = {0, (size_t)1 << 20, wgrad_workspace_bytes(g)};
    for (int w = 0; w < 3; ++w) {
      printf("%s{\"bytes\": %zu, \"cands\": [", w ? ", " : "", sizes[w]);
      const std::vector<int> cands = wgrad_candidates(&s, g, sizes[w], true);
      for (size_t i = 0; i < cands.size(); ++i) printf("%s%d", i ? ", " : "", cands[i]);
      printf("], \"kernels\": [");      // a 256 x 256 candidate whose chunk does not fit the 31-bit offsets is timed as the 128 x 128 kernel
      for (size_t i = 0; i < cands.size(); ++i)
        printf("%s%d", i ? ", " : "", (cands[i] & WG_FORM8) && wgrad_fits(&s, g.chunk_of(cands[i] & (WG_FORM8 - 1))) ? 256 : 128);
      printf("], \"picks\": [");
      for (size_t t = 0; t < times.size(); ++t) {
        std::vector<float> ms;
        int n128 = 0, n8 = 0;
        for (int c : cands) ms.push_back(c & WG_FORM8 ? times[t][28 + n8++] : times[t][n128++]);
        printf("%s%d", t ? ", " : "", wgrad_pick(cands.data(), ms.data(), (int)cands.size()));
      }
      std::vector<std::string> seen;      // the distinct outcomes, and per (strict, record, key 7) an index into them
      std::string grid;
      for (int strict = 0; strict < 2; ++strict)
        for (int record : RECORDS)
          for (int force : FORCES) {
            const std::string o = outcome(&s, g, record, force, strict != 0, sizes[w] != 0, sizes[w]);
            size_t k = std::find(seen.begin(), seen.end(), o) - seen.begin();
            if (k == seen.size()) seen.push_back(o);
            grid += (grid.empty() ? "" : ", ") + std::to_string(k);
          }
      printf("], \"outcomes\": [");
      for (size_t i = 0; i < seen.size(); ++i) printf("%s\"%s\"", i ? ", " : "", seen[i].c_str());
      printf("], \"grid\": [%s]}", grid.c_str());
    }
    printf("]}\n");
  }
  return 0;
}
