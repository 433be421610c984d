// ksim_desched_host.hpp -- the host arithmetic of a descheduling plan: where each replica's events sit in the
// per-event buffers, and how many pods a replica may evict.
//
// Host-only (no HIP type, no device call): the engine's plan driver (desched_plan in ksim_engine.hip) includes it,
// and so does the stand-alone check program tests/native_desched_host/desched_host_check.cpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ksim_ds_host {

// eoff[r] = the events of the replicas before r, eoff[R] = all of them.  Returns the largest stream length.
inline int event_offsets(const int* n_events, int R, std::vector<long long>& eoff) {
  int max_ev = 0;
  eoff.assign((size_t)R + 1, 0);
  for (int r = 0; r < R; ++r) {
    eoff[r + 1] = eoff[r] + n_events[r];
    max_ev = std::max(max_ev, n_events[r]);
  }
  return max_ev;
}

// deschedule.go:27 int(math.Ceil(ratio * float64(len(podMap)))), never more than the pods there are: defined for
// every ratio >= 0, +inf included, and every bound >= 0.  Without a bound pod it is 0 (inf * 0 is never formed);
// with one the product is not a NaN, and only a value below bound, so inside int32, is converted.
inline int32_t budget(double ratio, int32_t bound) {
  if (bound <= 0) return 0;
  const double want = std::ceil(ratio * (double)bound);
  return want < (double)bound ? (int32_t)want : bound;
}

}  // namespace ksim_ds_host
