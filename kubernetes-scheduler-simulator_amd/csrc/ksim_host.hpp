// Host-side plumbing of the engine that knows nothing of the engine itself: the growable device buffer and the
// environment knobs.  Host code only.  Included by ksim_engine.hip below KSIM_HIP; DevBuf calls hipMalloc / hipFree /
// hipMemcpyAsync as the includer declares them (a host check of its grow / upload / release logic supplies
// malloc-backed ones).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

// A device buffer that grows on demand: the pointer and its capacity in one owning object.
template <typename T>
struct DevBuf {
  T* p = nullptr;   // kernels take it by name: args.keys = e->d_h_keys.p
  size_t cap = 0;   // elements asked for by the ensure() that allocated p

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;  // one owner: the engine
  DevBuf& operator=(const DevBuf&) = delete;

  // Room for n elements.  Reallocates when n exceeds the capacity or nothing is allocated yet; the old
  // contents are then gone (*grew, if given, says so: a caller whose contents carry state re-initialises them).
  int ensure(size_t n, bool* grew = nullptr) {
    if (grew) *grew = false;
    if (n <= cap && p) return KSIM_OK;
    if (p) KSIM_HIP(hipFree(p));
    p = nullptr;
    cap = 0;
    KSIM_HIP(hipMalloc(&p, sizeof(T) * std::max(n, (size_t)1)));
    cap = n;
    if (grew) *grew = true;
    return KSIM_OK;
  }

  // ensure(v.size()), then v copied in on stream st (v is pageable: the caller synchronises before v goes away).
  int upload(const std::vector<T>& v, hipStream_t st) {
    const int rc = ensure(v.size());
    if (rc) return rc;
    KSIM_HIP(hipMemcpyAsync(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st));
    return KSIM_OK;
  }

  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Plain device pointers and DevBufs freed through one list, in the order given (ksim_engine_destroy).
static inline void release_one(void* p) { (void)hipFree(p); }
template <typename T>
static void release_one(DevBuf<T>& b) { b.release(); }
template <typename... B>
static void release_all(B&... b) { (release_one(b), ...); }

// Environment knobs.  Besides the five plain ones (KSIM_PROFILE, KSIM_COOP, KSIM_CUS,
// KSIM_SIDE_STREAMS, KSIM_GROUP_TIMES), two comma-separated key=value lists: KSIM_VARIANT selects the measured
// alternative forms of the kernels and plans (A/B runs; the defaults are what the bench and the tests measure),
// KSIM_TEST the test-only settings (wrap points, stress delays, forced misses).
static long knob(const char* var, const char* key, long dflt) {
  const char* v = std::getenv(var);
  if (!v) return dflt;
  const size_t kl = std::strlen(key);
  for (const char* p = v; *p;) {
    const char* q = std::strchr(p, ',');
    const size_t len = q ? (size_t)(q - p) : std::strlen(p);
    if (len > kl && std::strncmp(p, key, kl) == 0 && p[kl] == '=') return std::strtol(p + kl + 1, nullptr, 0);
    if (!q) break;
    p = q + 1;
  }
  return dflt;
}
static long variant(const char* key, long dflt) { return knob("KSIM_VARIANT", key, dflt); }
static long test_knob(const char* key, long dflt) { return knob("KSIM_TEST", key, dflt); }

constexpr int kSideStreams = 6;  // the most side streams a concurrent run uses (ksim_engine::side)

// The knobs a run reads, read once at its top (ksim_engine_run, ksim_shard_group_run): per run, not per process --
// a caller may change the variables between two runs.
struct RunEnv {
  int profile = 0;           // KSIM_PROFILE: 0 off (unset or "0"), 1 phase timers, 2 k_memo's step trace, 3 anything else
  bool group_times = false;  // KSIM_GROUP_TIMES=1
  int side_streams = 4;      // of a concurrent run: GPU_MAX_HW_QUEUES, KSIM_SIDE_STREAMS over it, 1..kSideStreams
  bool skip = true, gate = true, scan1_mix = true, report_overlap = true, pf_memo = true;  // KSIM_VARIANT
  bool force_report_overlap = false;                                                       // KSIM_TEST report_overlap
  long pf_memo_ver0 = 0;                                                                   // KSIM_TEST
  bool pf_guess = true;
  int hdelay = 0;  // KSIM_TEST hdelay=<mask>: the memoised kernels' hand-over stress delays (ksim_memo.hpp hdelay; the
                   // bits are per kernel); a nonzero mask selects the instantiations that carry them
  bool timers() const { return profile == 1; }
};

static RunEnv read_env() {
  RunEnv v;
  if (const char* pe = std::getenv("KSIM_PROFILE")) v.profile = pe[0] == '0' ? 0 : pe[0] == '1' ? 1 : pe[0] == '2' ? 2 : 3;
  const char* gt = std::getenv("KSIM_GROUP_TIMES");
  v.group_times = gt && gt[0] == '1';
  if (const char* q = std::getenv("GPU_MAX_HW_QUEUES")) v.side_streams = std::atoi(q) > 0 ? std::atoi(q) : v.side_streams;
  if (const char* q = std::getenv("KSIM_SIDE_STREAMS")) v.side_streams = std::atoi(q) > 0 ? std::atoi(q) : v.side_streams;
  v.side_streams = std::max(1, std::min(v.side_streams, kSideStreams));
  v.skip = variant("skip", 1) != 0;
  v.gate = variant("gate", 1) != 0;
  v.scan1_mix = variant("scan1_mix", 1) != 0;
  v.report_overlap = variant("report_overlap", 1) != 0;
  v.pf_memo = variant("pf_memo", 1) != 0;
  v.force_report_overlap = test_knob("report_overlap", 0) != 0;
  v.pf_memo_ver0 = test_knob("pf_memo_ver0", 0);
  v.pf_guess = test_knob("pf_guess", 1) != 0;
  v.hdelay = (int)(test_knob("hdelay", 0) & 0xff);
  return v;
}
