// The host side of "count, one host read, emit" (include/mi355det.h): what every *_emit entry point of the run-length family checks of
// the numbers the caller read back from its count pass, before any launch.
#pragma once
#include "common.h"

namespace mi355 {

// `what` = the entry point.  The total must reach min_total, else the entry's own text `below` (format: what, total_runs): one count per
// mask or annotation for the encoders; 0 for the string decoder, where a refused mask owns no counts.  An empty total needs no counts.
inline int check_emit(const char* what, const char* below, long long min_total, long long total_runs, long long capacity,
                      const void* run_offsets, const void* counts) {
  if (total_runs < min_total) return fail(MI355DET_EINVAL, below, what, total_runs);
  if (capacity < total_runs) return fail(MI355DET_EINVAL, "%s: capacity %lld is smaller than the %lld counts", what, capacity, total_runs);
  if (!run_offsets || (total_runs > 0 && !counts)) return fail(MI355DET_EINVAL, "%s: missing operand", what);
  return MI355DET_OK;
}

}  // namespace mi355
