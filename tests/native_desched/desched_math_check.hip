// Host-side harness for the descheduler's __host__ __device__ math (ksim_desched.hpp victim_eval,
// victim_score): the functions k_desched_eval and k_desched_select inline, run on the CPU so the CPU
// suite can compare them with the oracle without a GPU.  Test infrastructure only.
#include <cstring>

#include "ksim_desched.hpp"

using namespace ksim;

extern "C" {

long long dd_victim_score(double before, double after) { return ksim_ds::victim_score(before, after); }

// Add + F for a node state (cpu_left, gl[8], gpu count, type id, CPU capacity), a pod (cpu_nz, milli, num,
// GPU mask) and a typical table {cpu, milli, num_eff, mask} x T + freq[T] in the caller's order (split here
// as the engine's set_typical does: CPU-only entries first).  Returns 1 and *f_after when Add succeeds;
// *f_node is F of the state itself.
int dd_victim_eval(int cpu_left, const int* gl8, int gpu_cnt, int type_id, int cap, int cpu_nz, int milli, int num,
                   unsigned mask, int T, const int* tpi4, const double* tpf, double* f_node, double* f_after) {
  static TypDev tp[kMaxTypical];
  int nt = 0, ncpu = 0;
  bool typed = false;
  for (int pass = 0; pass < 2; ++pass) {
    for (int t = 0; t < T; ++t) {
      const bool cpu = tpi4[4 * t + 1] == 0;
      if ((pass == 0) != cpu) continue;
      TypDev d;
      std::memset(&d, 0, sizeof d);
      d.cpu = tpi4[4 * t];
      d.milli = tpi4[4 * t + 1];
      d.num_eff = tpi4[4 * t + 2];
      d.tmask = (uint32_t)tpi4[4 * t + 3];
      d.freq = tpf[t];
      if (!cpu && d.tmask != 0xFFFFFFFFu) typed = true;
      tp[nt++] = d;
    }
    if (pass == 0) ncpu = nt;
  }
  int gl[kMaxGpu];
  for (int g = 0; g < kMaxGpu; ++g) gl[g] = gl8[g];
  const uint32_t tb = 1u << type_id;
  if (typed) {
    *f_node = frag_F<true>(cpu_left, gl, tb, tp, ncpu, nt);
    return ksim_ds::victim_eval<true>(cpu_left, gl, gpu_cnt, tb, cap, cpu_nz, milli, num, mask, tp, ncpu, nt, f_after) ? 1 : 0;
  }
  *f_node = frag_F<false>(cpu_left, gl, tb, tp, ncpu, nt);
  return ksim_ds::victim_eval<false>(cpu_left, gl, gpu_cnt, tb, cap, cpu_nz, milli, num, mask, tp, ncpu, nt, f_after) ? 1 : 0;
}

}  // extern "C"
