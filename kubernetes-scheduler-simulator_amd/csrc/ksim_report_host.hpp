// ksim_report_host.hpp -- the host side of the per-event cluster report: exact records to reports.
//
// Host-only (no HIP type, no device call): the engine includes it, and so does the stand-alone check program
// tests/native_report/report_merge_check.cpp.
//
// A ksim_report_part is the device's RepAcc byte for byte: 9 signed 128-bit sums with LSB 2^-80 (the 7 frag bins, the
// cluster's CPU and GPU watts) as {low, high} halves, then 8 64-bit counters.  The parts of the shards of one
// cluster are added as integers -- exact, in any order or grouping -- and each 128-bit sum becomes a double once:
// the correctly rounded exact sum, what an unsharded engine reports.  Rounding every part first and adding the
// doubles would not give it.
#pragma once

#include <cmath>
#include <cstdint>

#include "ksim_engine.h"

namespace ksim_rep_host {

constexpr int kFx = 9;   // 128-bit fields of a part
constexpr int kCnt = 8;  // counters
constexpr int kMaxWorld = 16;

static_assert(sizeof(ksim_report_part) == 208, "ksim_report_part must stay the device's 208-byte record");

inline __int128 fx_get(const ksim_report_part& p, int k) {
  return (__int128)(((unsigned __int128)(uint64_t)p.fx[k][1] << 64) | (uint64_t)p.fx[k][0]);
}
inline void fx_set(ksim_report_part& p, int k, __int128 v) {
  const unsigned __int128 u = (unsigned __int128)v;
  p.fx[k][0] = (int64_t)(uint64_t)u;
  p.fx[k][1] = (int64_t)(uint64_t)(u >> 64);
}

// acc += p, field by field (unsigned adds: two's complement sums, no signed overflow)
inline void part_add(ksim_report_part& acc, const ksim_report_part& p) {
  for (int k = 0; k < kFx; ++k)
    fx_set(acc, k, (__int128)((unsigned __int128)fx_get(acc, k) + (unsigned __int128)fx_get(p, k)));
  for (int k = 0; k < kCnt; ++k) acc.cnt[k] = (int64_t)((uint64_t)acc.cnt[k] + (uint64_t)p.cnt[k]);
}

// exact fixed-point sum -> nearest double (the int128 -> double conversion rounds to nearest even; the 2^-80
// scaling is exact)
inline double fx_round(const ksim_report_part& p, int k) { return std::ldexp((double)fx_get(p, k), -80); }

// One exact record as the reports the ABI hands out (either may be null).
inline void part_reports(const ksim_report_part& p, ksim_report* out, ksim_power_report* power_out) {
  if (out) {
    for (int k = 0; k < 7; ++k) out->frag_bins[k] = fx_round(p, k);
    out->used_nodes = p.cnt[0];
    out->used_gpus = p.cnt[1];
    out->used_gpu_milli = p.cnt[2];
    out->total_gpus = p.cnt[7];
    out->arrived_gpu_milli = p.cnt[4];
    out->used_cpu_milli = p.cnt[3];
    out->arrived_cpu_milli = p.cnt[5];
  }
  if (power_out) {
    power_out->cpu_w = fx_round(p, 7);
    power_out->gpu_w = fx_round(p, 8);
    power_out->cluster_w = power_out->cpu_w + power_out->gpu_w;  // analysis.go:54 powerCPUCluster + powerGPUCluster
    power_out->invalid_nodes = p.cnt[6];
  }
}

// ksim_report_merge: event i of the cluster = the sum of event i of every shard's parts.
inline int merge(const ksim_report_part* const* parts, int world, int n, ksim_report* out, ksim_power_report* power_out) {
  if (!parts || !out || world < 1 || world > kMaxWorld || n < 0) return KSIM_EINVAL;
  for (int k = 0; k < world; ++k)
    if (!parts[k]) return KSIM_EINVAL;
  for (int i = 0; i < n; ++i) {
    ksim_report_part acc = parts[0][i];
    for (int k = 1; k < world; ++k) part_add(acc, parts[k][i]);
    part_reports(acc, out + i, power_out ? power_out + i : nullptr);
  }
  return KSIM_OK;
}

}  // namespace ksim_rep_host
