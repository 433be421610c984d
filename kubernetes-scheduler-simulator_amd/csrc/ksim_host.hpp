// Host-side plumbing of the engine that knows nothing of the engine itself: the owning handles of its device
// resources and the environment knobs.  Host code only.  Included by ksim_engine.hip below KSIM_HIP; the handles call
// the HIP functions as the includer declares them (tests/native_host supplies malloc-backed ones and checks the
// grow / upload / move / release logic on the CPU).  Every handle frees what it holds in its destructor, on the
// device that is current then: the owner sets it first.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

// A device buffer: the pointer and its capacity in one owning, movable object.
template <typename T>
struct DevBuf {
  T* p = nullptr;   // kernels take it by name: args.keys = e->hmemo.keys.p
  size_t cap = 0;   // elements asked for by the alloc() / ensure() that allocated p

  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}  // one owner: no copies
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }

  // Exactly n elements (one when n is 0), allocated afresh: what was held is freed first, and on failure the
  // buffer is left empty.  ext_flags: hipExtMallocWithFlags flags (hipDeviceMallocUncached), 0 for a plain hipMalloc.
  int alloc(size_t n, unsigned ext_flags = 0) {
    release();
    const size_t bytes = sizeof(T) * std::max(n, (size_t)1);
    KSIM_HIP(ext_flags ? hipExtMallocWithFlags((void**)&p, bytes, ext_flags) : hipMalloc((void**)&p, bytes));
    cap = n;
    return KSIM_OK;
  }

  // Room for n elements.  Reallocates when n exceeds the capacity or nothing is allocated yet; the old
  // contents are then gone (*grew, if given, says so: a caller whose contents carry state re-initialises them).
  int ensure(size_t n, bool* grew = nullptr) {
    const bool grow = n > cap || !p;
    const int rc = grow ? alloc(n) : KSIM_OK;
    if (grew) *grew = grow && !rc;
    return rc;
  }

  // ensure(v.size()), then v copied in on stream st (v is pageable: the caller synchronises before v goes away).
  int upload(const std::vector<T>& v, hipStream_t st) {
    const int rc = ensure(v.size());
    if (rc) return rc;
    KSIM_HIP(hipMemcpyAsync(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st));
    return KSIM_OK;
  }

  int fill(int byte, hipStream_t st) {  // every byte of the cap elements, on stream st
    if (cap) KSIM_HIP(hipMemsetAsync(p, byte, sizeof(T) * cap, st));
    return KSIM_OK;
  }
  int zero(hipStream_t st) { return fill(0, st); }

  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// An owned HIP object (event, stream, instantiated graph): movable, reads as the handle it holds; reset() destroys
// what is held and takes another.  Destroying a stream does not wait for its work: the owner drains it first.
template <typename H, hipError_t (*Destroy)(H)>
struct DevHandle {
  H h = nullptr;

  DevHandle() = default;
  DevHandle(DevHandle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}  // one owner: no copies
  ~DevHandle() { reset(); }
  operator H() const { return h; }
  void reset(H next = nullptr) {
    if (h) (void)Destroy(h);
    h = next;
  }
};
using GraphExec = DevHandle<hipGraphExec_t, hipGraphExecDestroy>;
// (The node-sharded mode's communicator is one more DevHandle: its Destroy goes through the dlopen'd RCCL, in
// ksim_engine.hip; like every handle it leaves a null one alone.)

// Created on first use: an event (hipEventDefault: a timing event, as hipEventCreate makes) and a non-blocking stream.
struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy> {
  int ensure(unsigned flags = hipEventDefault) {
    if (!h) KSIM_HIP(hipEventCreateWithFlags(&h, flags));
    return KSIM_OK;
  }
};
struct DevStream : DevHandle<hipStream_t, hipStreamDestroy> {
  int ensure() {
    if (!h) KSIM_HIP(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
    return KSIM_OK;
  }
};

// Host-mapped coherent int flags the device stores and the host polls: host pointer, device address, capacity.
struct MappedFlags {
  int* h = nullptr;
  int* d = nullptr;
  size_t cap = 0;

  MappedFlags() = default;
  MappedFlags(const MappedFlags&) = delete;
  MappedFlags& operator=(const MappedFlags&) = delete;
  ~MappedFlags() { release(); }

  int ensure(size_t n) {  // room for n flags; a larger block replaces the old one (freed first) and starts zeroed
    if (n <= cap && h) return KSIM_OK;
    release();
    KSIM_HIP(hipHostMalloc((void**)&h, sizeof(int) * std::max(n, (size_t)1), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h, 0, sizeof(int) * n);
    if (hipHostGetDevicePointer((void**)&d, h, 0) != hipSuccess) return release(), KSIM_EHIP;
    cap = n;
    return KSIM_OK;
  }
  void release() {
    if (h) (void)hipHostFree(h);
    h = d = nullptr;
    cap = 0;
  }
};

// The exchange buffers of a world of shard processes as this rank sees them: ptr[q] is rank q's buffer, the peers'
// opened by IPC, the own slot this rank's own allocation (never opened here, never closed).  Every other rank is
// mapped or none is.
struct PeerMap {
  std::vector<unsigned long long*> ptr;  // empty: nothing mapped
  int self = -1;

  PeerMap() = default;
  PeerMap(PeerMap&& o) noexcept : ptr(std::move(o.ptr)), self(o.self) { o.ptr.clear(); }  // one owner: no copies
  ~PeerMap() { close(); }
  bool mapped() const { return !ptr.empty(); }

  // handles: `world` records of `stride` bytes, each beginning with a hipIpcMemHandle_t.  On a failed open the ranks
  // opened so far are closed again, the map stays empty, and *bad / *why (nullable) name the rank and the error.
  int open(const uint8_t* handles, size_t stride, int world, int rank, unsigned long long* own, int* bad = nullptr,
           hipError_t* why = nullptr) {
    close();
    ptr.assign((size_t)world, nullptr);
    self = rank;
    ptr[rank] = own;
    for (int q = 0; q < world; ++q) {
      if (q == rank) continue;
      hipIpcMemHandle_t h;
      std::memcpy(&h, handles + (size_t)q * stride, sizeof h);
      void* p = nullptr;
      const hipError_t r = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
      if (r != hipSuccess) {
        if (bad) *bad = q;
        if (why) *why = r;
        close();  // (the ranks past q are still null)
        return KSIM_EHIP;
      }
      ptr[q] = reinterpret_cast<unsigned long long*>(p);
    }
    return KSIM_OK;
  }
  void close() {
    for (int q = 0; q < (int)ptr.size(); ++q)
      if (q != self && ptr[q]) (void)hipIpcCloseMemHandle(ptr[q]);
    ptr.clear();
  }
};

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
  // KSIM_VARIANT, the memoised FGD replays (ksim_plan.hpp; the first three take effect when a plan is made)
  bool memo_decider = false;  // run_mode 0 plans k_memo's decider form
  bool hl2 = false;           // k_hmemo at one workgroup per replica keeps the second maxima beside L1
  bool hmodel = true;         // k_hmemo's per-model tables of typed replicas (0: the whole table for every model)
  int hpf = 1;                // k_hmemo, one workgroup per replica: 1 = wave 0 lists the next refresh (the default since r04:
                              // C4 190.7 -> 178-185 ms, C2 run_mode 5 50.3 -> 47.7 ms, profiles/r04/memo/ab_runs.txt),
                              // 2 = touches its flagged rows, 0 = off (4: the wide form lists on wave 0 too)
  int hprune = 64;            // k_hmemo (A/B): the F list's group pruning for replicas with more than this many typical
                              // pods (-1: every replica; default 64: the large typed tables, where the F rounds bound the step)
  bool shard_hmemo = true;    // an in-process shard group of FGD replicas on k_hmemo_group (0: the per-pod k_step path)
  bool force_report_overlap = false;                                                       // KSIM_TEST report_overlap
  long pf_memo_ver0 = 0;                                                                   // KSIM_TEST
  bool pf_guess = true;
  int group_k = 0;  // KSIM_TEST group_k=<K>: the in-process k_replay shard group at K slices per shard (replay_group_slices)
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
  v.memo_decider = variant("memo_decider", 0) == 1;
  v.hl2 = variant("hl2", 0) == 1;
  v.hmodel = variant("hmodel", 1) != 0;
  v.hpf = (int)variant("hpf", 1) & 7;
  v.hprune = (int)variant("hprune", 64);
  v.shard_hmemo = variant("shard_hmemo", 1) != 0;
  v.force_report_overlap = test_knob("report_overlap", 0) != 0;
  v.pf_memo_ver0 = test_knob("pf_memo_ver0", 0);
  v.pf_guess = test_knob("pf_guess", 1) != 0;
  v.group_k = (int)std::max(0l, std::min(test_knob("group_k", 0), 256l));
  v.hdelay = (int)(test_knob("hdelay", 0) & 0xff);
  return v;
}
