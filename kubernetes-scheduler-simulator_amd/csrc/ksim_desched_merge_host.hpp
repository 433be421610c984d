// ksim_desched_merge_host.hpp -- the host merge of the descheduling plans of a node-sharded cluster's shards.
//
// Host-only (no HIP type, no device call): the engine includes it (ksim_desched_merge, ksim_cos_merge), and so does
// the stand-alone check program tests/native_desched_merge/desched_merge_check.cpp.
//
// Every shard plans the pods on its own nodes: a node's pops depend only on its own pods and its own priority
// history, and the nodes meet only in the visiting order and the budget.  So the cluster's victim list is the merge
// of the shards' lists by the key the select kernels walk in -- (frag_before descending, global rank ascending),
// for cosSim (gpu_left_milli descending, rank ascending) -- cut at budget(ratio, sum of the shards' bound pods).
// Each list is sorted by that key already and the key is unique (ranks are, and a node never pops twice at one
// priority), so a k-way merge that always takes the best head gives the order an unsharded engine plans in.  The
// device form is k_victim_merge (ksim_desched.hpp); both read the same key.
#pragma once

#include <cstdint>
#include <cstring>
#include <limits>

#include "ksim_desched_host.hpp"
#include "ksim_engine.h"

namespace ksim_ds_host {

constexpr int kMaxWorld = 16;

struct MergeKey {
  uint64_t prio;  // higher first
  uint32_t rank;  // then lower first
};
inline bool key_before(const MergeKey& x, const MergeKey& y) {
  return x.prio > y.prio || (x.prio == y.prio && x.rank < y.rank);
}
// frag_before is a non-negative double: its bits order as an integer (+ 0.0 folds a negative zero)
inline MergeKey merge_key(const ksim_victim& v) {
  const double f = v.frag_before + 0.0;
  uint64_t bits;
  std::memcpy(&bits, &f, sizeof bits);
  return MergeKey{bits, (uint32_t)v.node};
}
inline MergeKey merge_key(const ksim_cos_victim& v) { return MergeKey{(uint64_t)v.gpu_left_milli, (uint32_t)v.node}; }

// The validation both merges share, and the cluster's budget: KSIM_EINVAL for a null argument, world outside 1..16,
// a negative count (a null list is allowed only with count 0), a negative bound count or a sum past int32, a ratio
// that is negative or NaN, a negative cap.
template <class V>
inline int merge_check(const V* const* parts, const int* n, const int64_t* bound, int world, double ratio, int cap,
                       const int* n_out, int32_t* budget) {
  if (!parts || !n || !bound || !n_out || world < 1 || world > kMaxWorld || !(ratio >= 0.0) || cap < 0)
    return KSIM_EINVAL;
  int64_t sum = 0;
  for (int k = 0; k < world; ++k) {
    if (n[k] < 0 || (n[k] > 0 && !parts[k]) || bound[k] < 0) return KSIM_EINVAL;
    sum += bound[k];
    if (sum > (int64_t)std::numeric_limits<int32_t>::max()) return KSIM_EINVAL;
  }
  *budget = ksim_ds_host::budget(ratio, (int32_t)sum);
  return KSIM_OK;
}

// ksim_desched_merge / ksim_cos_merge: the first min(budget, sum of n) entries of the merged order into out[cap].
// *n_out is their number, set even when cap is too small (KSIM_ERANGE, nothing stored), *budget_out (nullable) the
// cluster's budget.  Inputs may be empty.
template <class V>
inline int merge(const V* const* parts, const int* n, const int64_t* bound, int world, double ratio, V* out, int cap,
                 int* n_out, int* budget_out) {
  int32_t budget = 0;
  if (int rc = merge_check(parts, n, bound, world, ratio, cap, n_out, &budget)) return rc;
  int64_t total = 0;
  for (int k = 0; k < world; ++k) total += n[k];
  const int take = (int)(total < (int64_t)budget ? total : (int64_t)budget);
  *n_out = take;
  if (budget_out) *budget_out = budget;
  if (cap < take) return KSIM_ERANGE;
  if (take > 0 && !out) return KSIM_EINVAL;
  int head[kMaxWorld] = {};
  for (int i = 0; i < take; ++i) {
    int best = -1;
    for (int k = 0; k < world; ++k)
      if (head[k] < n[k] && (best < 0 || key_before(merge_key(parts[k][head[k]]), merge_key(parts[best][head[best]]))))
        best = k;
    out[i] = parts[best][head[best]++];  // (best >= 0: i < take <= the entries left)
  }
  return KSIM_OK;
}

inline int merge_victims(const ksim_victim* const* parts, const int* n, const int64_t* bound, int world, double ratio,
                         ksim_victim* out, int cap, int* n_out, int* budget_out) {
  return merge<ksim_victim>(parts, n, bound, world, ratio, out, cap, n_out, budget_out);
}
inline int merge_cos_victims(const ksim_cos_victim* const* parts, const int* n, const int64_t* bound, int world,
                             double ratio, ksim_cos_victim* out, int cap, int* n_out, int* budget_out) {
  return merge<ksim_cos_victim>(parts, n, bound, world, ratio, out, cap, n_out, budget_out);
}

}  // namespace ksim_ds_host
