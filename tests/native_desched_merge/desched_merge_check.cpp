// desched_merge_check -- the host merge of the shards' descheduling plans (csrc/ksim_desched_merge_host.hpp) as a
// stand-alone program, built with -fsanitize=address,undefined (tests/test_desched_merge_cpu.py).  No GPU, no HIP.
//
// Synthetic lists for both record types: worlds 1, 2 and 16; priorities drawn from a few values, so that equal
// priorities meet across shards and the rank decides; shards without an entry, and every shard without one; ratios
// that give a budget of 0, one inside the list (the parts together, and single parts, are longer than it), one
// beyond the list, and +inf.  The expected output is a plain sort of the union by (priority descending, rank
// ascending), cut at budget(ratio, sum of the bound counts).  Then the argument errors.  Prints "cases=<n>", then
// "ok"; any broken expectation prints a line to stderr and exits 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ksim_desched_merge_host.hpp"

static void expect(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "desched_merge_check: %s\n", what);
  std::exit(1);
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) % n);
}

static void fill(ksim_victim& v, int event, int rank, int prio) {
  v = ksim_victim{};
  v.event = event, v.node = rank, v.gpu_mask = 1 + (int)rnd(255), v.score = 1 + (int64_t)rnd(1000);
  v.frag_before = 50.0 * prio + 0.25, v.frag_after = v.frag_before - (double)v.score;
}
static void fill(ksim_cos_victim& v, int event, int rank, int prio) {
  v = ksim_cos_victim{};
  v.event = event, v.node = rank, v.gpu_mask = 1 + (int)rnd(255);
  v.gpu_left_milli = 100 * prio, v.similarity = (double)rnd(1000) / 1000.0;
}
static bool same(const ksim_victim& x, const ksim_victim& y) {
  return x.event == y.event && x.node == y.node && x.gpu_mask == y.gpu_mask && x.score == y.score &&
         x.frag_before == y.frag_before && x.frag_after == y.frag_after;
}
static bool same(const ksim_cos_victim& x, const ksim_cos_victim& y) {
  return x.event == y.event && x.node == y.node && x.gpu_mask == y.gpu_mask && x.gpu_left_milli == y.gpu_left_milli &&
         x.similarity == y.similarity;
}

// One cluster of n_nodes ranks over `world` shards by rank range; each node gives 0..per_node entries of strictly
// falling priority (a node pops once per priority).  `hole`: the shards of that residue mod 3 get no entry;
// hole = -2: no shard gets one.
template <class V>
static long run_cluster(int world, int n_nodes, int per_node, int hole) {
  using namespace ksim_ds_host;
  std::vector<std::vector<V>> parts((size_t)world);
  std::vector<V> all;
  int event = 0;
  for (int rank = 0; rank < n_nodes; ++rank) {
    const int k = (int)((long long)rank * world / n_nodes);
    if (hole == -2 || (hole >= 0 && k % 3 == hole)) continue;
    int prio = 1 + (int)rnd(6) + per_node;
    const int cnt = (int)rnd((uint32_t)per_node + 1);
    for (int j = 0; j < cnt; ++j, --prio) {
      V v;
      fill(v, event++, rank, prio);
      parts[(size_t)k].push_back(v);
      all.push_back(v);
    }
  }
  const auto by_key = [](const V& x, const V& y) { return key_before(merge_key(x), merge_key(y)); };
  for (auto& p : parts) std::sort(p.begin(), p.end(), by_key);
  std::sort(all.begin(), all.end(), by_key);
  for (size_t i = 1; i < all.size(); ++i) expect(by_key(all[i - 1], all[i]), "the keys are unique");
  std::vector<const V*> ptr;
  std::vector<int> n;
  std::vector<int64_t> bound;
  int64_t bound_sum = 0;
  for (auto& p : parts) {
    ptr.push_back(p.empty() ? nullptr : p.data());  // an empty part may come as a null list
    n.push_back((int)p.size());
    bound.push_back((int64_t)p.size() + rnd(5));
    bound_sum += bound.back();
  }
  const double inf = std::numeric_limits<double>::infinity();
  const double ratios[] = {0.0, 1e-9, 0.01, 0.3, 0.5, 1.0, 7.0, inf};
  long cases = 0;
  for (const double q : ratios) {
    const int budget = ksim_ds_host::budget(q, (int32_t)bound_sum);
    const int want = (int)std::min<size_t>(all.size(), (size_t)budget);
    std::vector<V> out(all.size() + 1);
    int got = -1, b = -1;
    expect(merge<V>(ptr.data(), n.data(), bound.data(), world, q, out.data(), (int)all.size(), &got, &b) == KSIM_OK,
           "merge returns KSIM_OK");
    expect(got == want && b == budget, "the number merged and the budget");
    for (int i = 0; i < want; ++i) expect(same(out[(size_t)i], all[(size_t)i]), "the merged order is the sorted union, cut");
    if (want > 0) {  // a buffer one short: the count is still set, nothing is stored past it
      std::vector<V> small((size_t)want - 1 + 1);
      got = -1;
      expect(merge<V>(ptr.data(), n.data(), bound.data(), world, q, small.data(), want - 1, &got, nullptr) == KSIM_ERANGE,
             "a short buffer is KSIM_ERANGE");
      expect(got == want, "n_out is set with KSIM_ERANGE");
    }
    if (q == 0.0) expect(want == 0, "ratio 0 takes none");
    if (q >= 1.0) expect(want == (int)all.size(), "ratio >= 1 takes every entry");
    ++cases;
  }
  return cases;
}

template <class V>
static void argument_errors() {
  using namespace ksim_ds_host;
  V one[1] = {};
  const V* ptr[17];
  int n[17];
  int64_t bound[17];
  for (int k = 0; k < 17; ++k) ptr[k] = one, n[k] = 1, bound[k] = 1;
  V out[17];
  int got = 0, b = 0;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  expect(merge<V>(nullptr, n, bound, 1, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "null parts");
  expect(merge<V>(ptr, nullptr, bound, 1, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "null counts");
  expect(merge<V>(ptr, n, nullptr, 1, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "null bounds");
  expect(merge<V>(ptr, n, bound, 1, 1.0, out, 17, nullptr, &b) == KSIM_EINVAL, "null n_out");
  expect(merge<V>(ptr, n, bound, 1, 1.0, nullptr, 17, &got, &b) == KSIM_EINVAL, "null out with entries to store");
  expect(merge<V>(ptr, n, bound, 0, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "world 0");
  expect(merge<V>(ptr, n, bound, 17, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "world 17");
  expect(merge<V>(ptr, n, bound, 1, -0.5, out, 17, &got, &b) == KSIM_EINVAL, "negative ratio");
  expect(merge<V>(ptr, n, bound, 1, nan, out, 17, &got, &b) == KSIM_EINVAL, "NaN ratio");
  expect(merge<V>(ptr, n, bound, 1, 1.0, out, -1, &got, &b) == KSIM_EINVAL, "negative cap");
  n[1] = -1;
  expect(merge<V>(ptr, n, bound, 2, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "negative count");
  n[1] = 1, bound[1] = -1;
  expect(merge<V>(ptr, n, bound, 2, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "negative bound");
  bound[1] = std::numeric_limits<int32_t>::max();
  expect(merge<V>(ptr, n, bound, 2, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "bound counts past int32");
  bound[1] = 1, ptr[1] = nullptr;
  expect(merge<V>(ptr, n, bound, 2, 1.0, out, 17, &got, &b) == KSIM_EINVAL, "null list with a count");
  ptr[1] = one;
  expect(merge<V>(ptr, n, bound, 16, 1.0, out, 17, &got, nullptr) == KSIM_OK && got == 16, "world 16, no budget_out");
}

int main() {
  long cases = 0;
  for (const int world : {1, 2, 16})
    for (const int n_nodes : {16, 97, 513})
      for (const int per_node : {1, 3})
        for (const int hole : {-1, 0, 1, -2}) {
          cases += run_cluster<ksim_victim>(world, n_nodes, per_node, hole);
          cases += run_cluster<ksim_cos_victim>(world, n_nodes, 1, hole);
        }
  argument_errors<ksim_victim>();
  argument_errors<ksim_cos_victim>();
  std::printf("cases=%ld\nok\n", cases);
  return 0;
}
