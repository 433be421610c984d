// Host-side harness for the cosSim descheduler's __host__ __device__ math (ksim_desched.hpp cos_similarity,
// cos_elects, cos_bits): the functions k_cos_eval and k_cos_select inline, run on the CPU so the CPU suite can
// compare them with the restatement without a GPU.  Test infrastructure only.
#include "ksim_desched.hpp"

using namespace ksim;

extern "C" {

// Add + similarity for a node state (cpu_left, gl[8], gpu count, CPU capacity) and a pod (cpu_nz, milli, num,
// GPU mask): -1 for every case the reference skips.
double dc_cos_similarity(int cpu_left, const int* gl8, int gpu_cnt, int cap, int cpu_nz, int milli, int num,
                         unsigned mask) {
  int gl[kMaxGpu];
  for (int g = 0; g < kMaxGpu; ++g) gl[g] = gl8[g];
  return ksim_ds::cos_similarity(cpu_left, gl, gpu_cnt, cap, cpu_nz, milli, num, mask);
}

int dc_cos_elects(double s) { return ksim_ds::cos_elects(s) ? 1 : 0; }
unsigned long long dc_cos_bits(double s) { return ksim_ds::cos_bits(s); }

}  // extern "C"
