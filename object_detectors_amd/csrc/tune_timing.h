// Timing helpers of the plan-time tuners (conv_kernels.hip: tile configurations and the stride-2 data-gradient form; wgrad_kernels.hip: split
// counts).  Includes the HIP runtime: not for lib.cpp (tune_record.h is the part it reads).
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

// a pair of timing events destroyed on every exit path (the tuning helpers return early on launch errors)
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool ok = false;
  EventPair() {
    if (hipEventCreate(&e0) != hipSuccess) { e0 = nullptr; return; }
    if (hipEventCreate(&e1) != hipSuccess) { e1 = nullptr; return; }
    ok = true;
  }
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
};

// Time `fn` for the tuning helpers: one warm-up launch, then the FASTER of two batches of three launches (a single batch of three let a
// neighbour's burst or a cold L2 decide: round 4 saw the tuner keep a 128 us configuration for 256->512 s2 @40 where the same kernel list
// held one of 106 us).  Returns milliseconds per batch, < 0 on a launch error (code in *err).
template <class F>
float time_candidate(F&& fn, hipEvent_t e0, hipEvent_t e1, hipStream_t st, int* err) {
  *err = fn();
  if (*err) return -1.f;
  float best = 1e30f;
  for (int b = 0; b < 2; ++b) {
    (void)hipEventRecord(e0, st);
    for (int r = 0; r < 3; ++r) (void)fn();
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  return best;
}

}  // namespace mi355
