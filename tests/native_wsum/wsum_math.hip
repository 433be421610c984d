// Host build of wsum_total (ksim_device.hpp): the normalise / range-check / weighted-sum arithmetic k_wsum runs per
// feasible node, behind a C entry point for tests/test_wsum_math_cpu.py (test infrastructure).
#include "ksim_device.hpp"

extern "C" {

// raw: [n][7] raw scores by plugin id, w: [7].  BestFit's and PWR's ranges are taken over the n nodes, as the kernel's
// block reduction takes them over the feasible nodes.  total: [n]; returns 1 when any node's score left 0..100.
int wm_totals(const int* raw, int n, const int* w, int* total) {
  using namespace ksim;
  int bf_lo = 0x7fffffff, bf_hi = (int)0x80000000, pw_lo = 0x7fffffff, pw_hi = (int)0x80000000;
  for (int i = 0; i < n; ++i) {
    bf_lo = raw[i * 7 + POL_BESTFIT] < bf_lo ? raw[i * 7 + POL_BESTFIT] : bf_lo;
    bf_hi = raw[i * 7 + POL_BESTFIT] > bf_hi ? raw[i * 7 + POL_BESTFIT] : bf_hi;
    pw_lo = raw[i * 7 + POL_PWR] < pw_lo ? raw[i * 7 + POL_PWR] : pw_lo;
    pw_hi = raw[i * 7 + POL_PWR] > pw_hi ? raw[i * 7 + POL_PWR] : pw_hi;
  }
  int ww[kNumPlugins];
  for (int p = 0; p < kNumPlugins; ++p) ww[p] = w[p];
  int any = 0;
  for (int i = 0; i < n; ++i) {
    int r[kNumPlugins];
    for (int p = 0; p < kNumPlugins; ++p) r[p] = raw[i * 7 + p];
    bool err = false;
    total[i] = wsum_total(r, bf_lo, bf_hi, pw_lo, pw_hi, ww, &err);
    any |= err ? 1 : 0;
  }
  return any;
}

int wm_num_plugins(void) { return ksim::kNumPlugins; }

}  // extern "C"
