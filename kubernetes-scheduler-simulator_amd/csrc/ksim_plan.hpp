// ksim_plan.hpp -- host-side planning: the memoised FGD replays (k_memo, ksim_memo.hpp; k_hmemo, ksim_hmemo.hpp), the
// run plan of the persistent path (make_run_plan: which kernel every replica runs on, in which order, on which stream,
// at what width) and the slices of the node-sharded runs.
//
// Everything here is arithmetic over vectors: which workgroup owns which pod class, how wide a launch is, how its LDS
// is carved, which instantiation of a kernel a run takes.  No HIP call and no environment read: the engine
// (ksim_engine.hip) fills a PlanInput / RunPlanInput from its own state, the knobs it read (RunEnv) and a residency
// query bound to the kernel, so the same code runs in a CPU-only test (tests/native_host/plan_check.cpp).  The LDS
// layouts are host-and-device functions: k_hmemo, k_replay and k_scan1 carve their dynamic LDS with the function the
// planner sizes it with; k_memo's carving is written out at the top of the kernel (its register allocation is
// sensitive to it) and held to memo_layout by that test.
#pragma once
#include <algorithm>
#include <array>
#include <cstring>
#include <functional>
#include <map>
#include <numeric>
#include <utility>
#include <vector>

#include "ksim_device.hpp"
#include "ksim_engine.h"

namespace ksim_plan {

using namespace ksim;

constexpr size_t kLdsMax = 160 * 1024;  // LDS of one CU (gfx950)

// Slices of a node-sharded launch: K workgroups per shard, S nodes (k_hmemo: ranks) each; !ok: the group does not fit.
struct ShardSlices {
  int K, S;
  bool ok;
};

// ---- k_memo: limits and LDS layout (ksim_memo.hpp takes them from here) ----
namespace memo {
constexpr int kMaxCw = 64;         // class slots per workgroup (one wave-0 lane each)
constexpr int kFoldRows = 6;       // Q1, Q2 (+Q3 frag), Q4, XL, XR, NA
// fold-buffer rows 66 doubles apart: lanes 0-5 fold rows 0-5 with ds_read_b128, whose bank is
// (a/4) % 64; a 64-double (2 x 256 B) stride put all six rows on the same banks (6-way conflict),
// 66 puts row b on banks 4b..4b+3
constexpr int kFoldStride = 66;
constexpr int kFoldBuf = kFoldRows * kFoldStride;  // doubles per evaluating wave
constexpr int kMemoMaxRank = 0xFFF;  // ranks are a 12-bit field of the packed key (pack_key32)
// sizeof(MemoShared), sizeof(DeciderScratch): the structs stay beside the kernel, which asserts both
constexpr size_t kSharedBytes = 25088, kDeciderBytes = 5328;

// Dynamic LDS of k_memo: MemoShared | NodeRec nodes[N] | keys[Cw][N] (or the decider's scratch; none with the keys in
// HBM) | the F waves' fold buffers (start-up: two words per node) | int last[N].
struct MemoLayout {
  size_t nodes, keys, fold, last, total;
};
KSIM_HD MemoLayout memo_layout(int N, int Cw, int nfw, bool hkeys) {
  const size_t keys = (size_t)Cw * N * 4 > kDeciderBytes ? (size_t)Cw * N * 4 : kDeciderBytes;
  const size_t fold = (size_t)nfw * kFoldBuf * 8, two = ((size_t)N * 8 + 15) & ~(size_t)15;
  MemoLayout L;
  L.nodes = kSharedBytes;
  L.keys = L.nodes + (size_t)N * sizeof(NodeRec);
  L.fold = L.keys + (hkeys ? 0 : (keys + 15) & ~(size_t)15);
  L.last = L.fold + (fold > two ? fold : two);
  L.total = L.last + (size_t)N * 4;
  return L;
}
}  // namespace memo

// ---- k_hmemo: limits and LDS layout (ksim_hmemo.hpp takes them from here) ----
namespace hmemo {
constexpr int kFan = 64;              // keys per L1 block (one wave / one quarter-wave dwordx4 row)
constexpr int kMaxNb = 64;            // L1 blocks per class (N <= 4096)
constexpr int kMaxClasses = 1024;     // one class-pass thread each
constexpr int kMaxGroups = 128;
constexpr int kMaxItems = 1 + 8 * kMaxGroups;
constexpr int kHRankMax = (1 << 20) - 1;
constexpr uint32_t kMtPresent = 1u << 31;
constexpr size_t kSharedBytes = 14080;  // sizeof(HShared): the struct stays beside the kernel, which asserts it

// Dynamic LDS after HShared (16-B aligned regions).
struct HLayout {
  size_t cls, gpod, F, l1, l2, nodes, last, cnt, bx, bx2, cgrp, flist, code, igrp, fnew, fold, gbase, gkey, ctp, mto, total;
};
KSIM_HD size_t halign(size_t x) { return (x + 15) & ~(size_t)15; }
KSIM_HD HLayout hmemo_layout(int N, int Cmax, int Gmax, int nb, bool l2, int Mtab) {
  HLayout L;
  size_t o = kSharedBytes;
  L.cls = o;   o = halign(o + (size_t)Cmax * sizeof(PodDev));
  L.gpod = o;  o = halign(o + (size_t)Gmax * sizeof(PodDev));
  L.F = o;     o = halign(o + (size_t)kMaxItems * sizeof(double));
  L.l1 = o;    o = halign(o + (size_t)Cmax * nb * 4);
  L.l2 = o;    o = halign(o + (l2 ? (size_t)Cmax * nb * 4 : 0));
  L.nodes = o; o = halign(o + (size_t)N * sizeof(NodeRec));
  L.last = o;  o = halign(o + (size_t)N * 4);
  L.cnt = o;   o = halign(o + (size_t)Cmax * 4);
  L.bx = o;    o = halign(o + (size_t)Cmax * 4);
  L.bx2 = o;   o = halign(o + (l2 ? (size_t)Cmax * 4 : 0));
  L.cgrp = o;  o = halign(o + (size_t)Cmax * 2);
  L.flist = o; o = halign(o + (size_t)Cmax * 2);
  L.code = o;  o = halign(o + (size_t)2 * kMaxItems);  // the F list, double-buffered like d's records
  L.igrp = o;  o = halign(o + (size_t)2 * kMaxItems);
  L.fnew = o;  o = halign(o + (size_t)Cmax);
  L.fold = o;  o = halign(o + (size_t)Cmax);
  L.gbase = o; o = halign(o + (size_t)Gmax * 2 * 2);
  L.gkey = o;  o = halign(o + (size_t)Gmax * 2 * 4);  // every score group's key on d, double-buffered like the list
  L.ctp = o;   o = halign(o + (size_t)Mtab * sizeof(TypDev));  // the per-model tables (typed replicas)
  L.mto = o;   o = halign(o + (Mtab > 0 ? (size_t)KSIM_MAX_TYPES * 4 : 0));
  L.total = o;
  return L;
}

// Slices of a wide or node-sharded k_hmemo launch over n ranks: S ranks per workgroup (a multiple of kFan, so no L1
// block straddles two workgroups) for about `want` workgroups, K workgroups.  What the three callers differ in:
//   kNoClamp    the unsharded wide form (hmemo_plan): the caller refuses an S past one L1 level;
//   kClamp      the in-process shard group: S cut to one L1 level, K from S;
//   kClampKeepK one shard per process: K stays `want` on every rank (ranks differ in their node counts, never in K)
//               unless S had to be cut.
enum SliceClamp { kNoClamp, kClamp, kClampKeepK };
struct HSlices {
  int S, K;
};
inline HSlices hmemo_slices(int n, int want, SliceClamp clamp) {
  int S = std::max(kFan, (n + want - 1) / want + kFan - 1) / kFan * kFan;
  const bool cut = clamp != kNoClamp && S > kMaxNb * kFan;
  if (cut) S = kMaxNb * kFan;
  return {S, clamp == kClampKeepK && !cut ? want : (n + S - 1) / S};
}
// One shard per process (ksim_engine_run of a shard with peers): the same K and S on every rank, from n_global and
// world only; refused when the exchange would pass 256 columns or this shard's N nodes pass its slices.
inline ShardSlices hmemo_peer_slices(int n_global, int world, int N) {
  const HSlices sl = hmemo_slices((n_global + world - 1) / world, std::max(1, 64 / world), kClampKeepK);
  return {sl.K, sl.S, world * sl.K <= 256 && N <= sl.K * sl.S};
}
// The in-process shard group over shards of at most nmax nodes.
inline ShardSlices hmemo_group_slices(int nmax, int world, int cus) {
  const HSlices sl = hmemo_slices(nmax, std::max(1, std::min(64, cus / world)), kClamp);
  return {sl.K, sl.S, sl.K >= 1 && world * sl.K <= 256 && sl.K * sl.S >= nmax};
}
}  // namespace hmemo

// ---- k_replay: limits and LDS layout (ksim_replay.hpp takes them from here) ----
namespace replay {
constexpr int kMaxK = 256;     // workgroups per replica (<= 64: one granule column per polling lane)
constexpr int kPfGuess = 256;  // PWR+FGD: entries of the guessed-range table (class id mod 256)
constexpr int kTagStride = 16;  // u16 tag counts per node
// sizeof(ReplayShared), sizeof(ReplayFgd): the structs stay beside the kernel, which asserts both
constexpr size_t kSharedBytes = 5248, kFgdBytes = 20864;

// The dynamic LDS layout of one k_replay workgroup (host and device).
struct RLayout {
  size_t fgd, nodes, tags, F0, E0, pe, last, praw, pinf, gtab, pver, pm, total;
};
// pm_c > 0 (PWR+FGD): u32 pver[S+1] (each slot's state version) and uint2 pm[pm_c][S] (every class's
// memoised Filter + Score of every real slot, valid while its version matches; pf_memo_* in ksim_replay.hpp)
__host__ __device__ inline RLayout replay_layout(int S, int pol, bool general, int pm_c = 0) {
  const bool tags = pol == POL_CLUSTERING, fgd = pol == POL_FGD || pol == POL_PWR_FGD;
  const bool pwr = pol == POL_PWR || pol == POL_PWR_FGD, pf = pol == POL_PWR_FGD;
  const size_t S1 = (size_t)S + 1;
  RLayout L;
  size_t o = kSharedBytes;
  L.fgd = o;   o += fgd ? kFgdBytes : 0;
  L.nodes = o; o += S1 * sizeof(NodeRec);
  L.tags = o;  o += tags ? S1 * kTagStride * sizeof(uint16_t) : 0;
  L.F0 = o;    o += fgd ? S1 * sizeof(double) : 0;
  L.E0 = o;    o += pwr ? S1 * sizeof(double) : 0;
  L.pe = o;    o += pwr ? S1 * sizeof(int2) : 0;
  L.last = o;  o += general ? S1 * sizeof(int) : 0;
  L.praw = o;  o += pf ? 2 * S1 * sizeof(int) : 0;  // by step parity: the pending step's stays intact
  L.pinf = o;  o += pf ? 2 * S1 * sizeof(int) : 0;
  o = (o + 15) / 16 * 16;
  L.gtab = o;  o += pf ? kPfGuess * sizeof(int4) : 0;
  L.pver = o;  o += (pf && pm_c > 0) ? (S1 * sizeof(unsigned) + 15) / 16 * 16 : 0;
  L.pm = o;    o += (pf && pm_c > 0) ? (size_t)pm_c * S * sizeof(uint2) : 0;
  L.total = o;
  return L;
}
inline size_t replay_lds(int S, int pol, bool general) {  // S real slots + the virtual node
  return replay_layout(S, pol, general).total;
}
}  // namespace replay

// ---- k_scan1: limits and LDS size (ksim_scan1.hpp takes them from here) ----
namespace scan1 {
constexpr int kBlock = 256;
constexpr int kRegSlots = 5;  // kReg: node slots per thread held in VGPRs (N <= 1280, the openb clusters)
constexpr int kPolMix = 65;   // scan1_lds's policy id of a k_scan1_mix launch (the presence bits always present)
constexpr size_t kSharedBytes = 4864;  // sizeof(Scan1Shared): the struct stays beside the kernel, which asserts it
// k_scan1 has an instantiation for these policies (the engine's scan1_fn names them; launch_scan1 refuses a null)
inline bool scan1_serves(int pol) { return pol >= POL_BESTFIT && pol <= POL_RANDOM; }

// Dynamic LDS: Scan1Shared | NodeRec nodes[N] (not with kReg) | u16 tag presence[N] rounded up to 16 B
// (GpuClustering, and every k_scan1_mix launch) | i32 last[N] (report)
__host__ __device__ inline size_t scan1_tm_bytes(int N) { return ((size_t)N * sizeof(uint16_t) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t scan1_lds(int N, int pol, bool report, bool reg = false) {
  return kSharedBytes + (reg ? 0 : (size_t)N * sizeof(NodeRec)) +
         (pol == POL_CLUSTERING || pol == kPolMix ? scan1_tm_bytes(N) : 0) + (report ? (size_t)N * 4 : 0);
}
}  // namespace scan1

// ---- k_wsum: limits and LDS layout (ksim_wsum.hpp takes them from here) ----
namespace wsum {
constexpr int kBlock = 1024;           // thread t owns the node slots t, t + kBlock, ...
constexpr size_t kSharedBytes = 5328;  // sizeof(WsumShared): the struct stays beside the kernel, which asserts it
constexpr int kMaxNodes = kMaxSlice + 1;  // the packed key's slot field (one workgroup holds the whole cluster)
// the plugins of a weight vector as a mask (bit p: w[p] > 0)
inline unsigned plugin_mask(const int32_t* w) {
  unsigned m = 0u;
  for (int p = 0; p < kNumPlugins; ++p) m |= w[p] > 0 ? 1u << p : 0u;
  return m;
}
// Dynamic LDS after WsumShared (16-B aligned regions): NodeRec nodes[N] | int4 sc[N] (the step's raw scores of every
// slot, kept between the scan and the decision) | u16 tags[N][16] (GpuClustering in the mask: the tag counts) |
// double F0[N] (FGD in the mask: cached F of the current state, < 0 = stale) | i32 last[N] (general: the report's
// previous event per node).
struct WLayout {
  size_t nodes, sc, tags, F0, last, total;
};
__host__ __device__ inline WLayout wsum_layout(int N, unsigned mask, bool general) {
  const size_t n = (size_t)N;
  WLayout L;
  size_t o = kSharedBytes;
  L.nodes = o; o += n * sizeof(NodeRec);
  L.sc = o;    o += n * 16;
  L.tags = o;  o += ((mask >> POL_CLUSTERING) & 1u) ? n * replay::kTagStride * sizeof(uint16_t) : 0;
  L.F0 = o;    o += ((mask >> POL_FGD) & 1u) ? n * sizeof(double) : 0;
  L.last = o;  o += general ? (n * sizeof(int) + 15) / 16 * 16 : 0;
  L.total = o;
  return L;
}
inline size_t wsum_lds(int N, unsigned mask, bool general) { return wsum_layout(N, mask, general).total; }
inline bool wsum_fits(int N, unsigned mask, bool general) {
  return N >= 1 && N <= kMaxNodes && wsum_lds(N, mask, general) <= kLdsMax;
}
}  // namespace wsum

// ---- which instantiation a launch takes ----
// The engine maps a form's code() to a function pointer in one switch over the enumerators below (no default: a form
// without an instantiation does not compile clean); tests/native_host/plan_check.cpp enumerates every input.
struct MemoForm {
  bool decider, general, stress, report, hkeys;  // k_memo's template arguments, in order
  constexpr int code() const { return decider | general << 1 | stress << 2 | report << 3 | hkeys << 4; }
};
enum MemoFormCode : int {
  kMemoLean = 0, kMemoDecider = 1 | 2, kMemoGeneral = 2, kMemoStress = 4, kMemoReport = 8,
  kMemoHKeysLean = 16, kMemoHKeysGeneral = 16 | 2, kMemoHKeysReport = 16 | 8,
};
// general: the instantiation with the profile hooks, the trace, deletes and the sigmoid expression for a missing
// score table; else a lean one, with the report's stores when the report is on.
inline MemoForm memo_form(bool decider, bool hkeys, bool profile, bool tracing, bool table, bool any_delete, bool report,
                          int hdelay) {
  const bool general = profile || tracing || !table || any_delete;
  if (decider) return {true, true, false, false, false};
  if (hkeys) return {false, general, false, !general && report, true};  // (no stress form: hdelay reaches only the general one)
  if (general) return {false, true, false, false, false};
  // the hdelay test knob: the lean kernel with the stress delays compiled in.  With the report on this row wins over
  // the next, and the stress form has none of the report's stores: kept as it is here.
  if (hdelay) return {false, false, true, false, false};
  return {false, false, false, report, false};
}

struct HMemoForm {
  int sub;     // the exchange: 0 one workgroup per replica, 1 up to 64 granule columns, 4 up to 256
  bool prof;   // the general instantiation: timers, stress delays
  bool model;  // the large-table instantiation (per-model tables, F-list pruning; one workgroup per replica only)
  bool group;  // k_hmemo_group: an in-process shard group's launch
  constexpr int code() const { return sub | prof << 3 | model << 4 | group << 5; }
};
enum HMemoFormCode : int {
  kHMemoOne = 0, kHMemoOneProf = 8, kHMemoOneModel = 16, kHMemoOneProfModel = 24,
  kHMemoWide = 1, kHMemoWideProf = 9, kHMemoWide4 = 4, kHMemoWide4Prof = 12,
  kHMemoGroup = 33, kHMemoGroupProf = 41, kHMemoGroup4 = 36, kHMemoGroup4Prof = 44,
};
enum HMemoWhere { kHLocal, kHPeer, kHGroup };  // an unsharded launch, one shard per process, an in-process shard group
// Ktot: the granule columns of the exchange (an unsharded launch: its workgroups per replica).  A sharded launch never
// takes the one-workgroup form, and has no profile buffer: only the stress delays make it general.
inline HMemoForm hmemo_form(HMemoWhere where, int Ktot, bool profile, int hdelay, bool model) {
  const bool gen = (where == kHLocal && profile) || hdelay != 0;
  if (where == kHLocal && Ktot == 1) return {0, gen, model, false};
  return {Ktot <= 64 ? 1 : 4, gen, false, where == kHGroup};
}

// ---- what the planners read ----
struct ReplicaView {  // one replica of the plan
  const std::vector<PodDev>* cls;   // its pod classes (classify_events)
  const std::vector<int>* ev_cls;   // class of each event, -1 delete
  const std::vector<NodeRec>* rec;  // its initial node records
  const std::vector<TypDev>* tp;    // its typical table as uploaded
  int typed, ncpu, nt;              // ReplicaDev's
};
struct PlanInput {
  std::vector<ReplicaView> reps;  // in launch order
  int N = 0, node_off = 0, cus = 0, wgs_req = 0, run_mode = 0;
  bool decider = false;      // k_memo's decider form
  bool hl2 = false;          // KSIM_VARIANT hl2: k_hmemo's second maxima (one workgroup per replica, when they fit)
  bool hmodel = true;        // KSIM_VARIANT hmodel: k_hmemo's per-model tables
  bool score_table = false;  // the FGD score steps exist (k_hmemo needs them)
  // workgroups of k_memo (1024 threads, that much dynamic LDS) resident at once on the usable CUs
  std::function<int(size_t lds)> resident;
};

// ---- pod requests and classes ----
inline int to_pod_dev(const ksim_pod& s, PodDev* d) {
  if (s.gpu_milli < 0 || s.gpu_milli > kMilli || s.gpu_count < 0 || s.gpu_count > kMaxGpu) return KSIM_ERANGE;
  if (s.cpu_milli < 0 || s.cpu_milli > 0x3fffffff || s.cpu_nz_milli < 0 || s.cpu_nz_milli > 0x3fffffff ||
      s.mem_mib < 0 || s.mem_mib > 0x3fffffff)
    return KSIM_ERANGE;
  std::memset(d, 0, sizeof *d);
  d->cpu_req = (int32_t)s.cpu_milli;
  d->cpu_nz = (int32_t)s.cpu_nz_milli;
  d->mem = (int32_t)s.mem_mib;
  d->milli = (int16_t)s.gpu_milli;
  d->num = (int8_t)s.gpu_count;
  // GetGpuAffinityFromPodAnnotation (open-gpu-share/utils/pod.go:111-123)
  if (s.gpu_count == 0) d->tag = -1;
  else if (s.gpu_count == 1 && s.gpu_milli < kMilli) d->tag = 0;
  else if (s.gpu_milli == kMilli) d->tag = (int8_t)s.gpu_count;
  else d->tag = -2;
  d->tmask = s.type_mask;
  d->ref = s.ref;
  d->flags = s.is_delete ? kPodDelete : 0u;
  return KSIM_OK;
}

// Pod classes of one event stream: the distinct Filter + Score requests of its creation events, in order of first
// appearance (cls[id].pad = id), how many events each has, and the class of every event (-1 delete), which is also
// written to the event's own pad: the kernels read it there.
inline void classify_events(std::vector<PodDev>& ev, std::vector<PodDev>& cls, std::vector<int>& cn, std::vector<int>& ev_cls) {
  const int n = (int)ev.size();
  cls.clear();
  cn.clear();
  std::vector<std::pair<std::vector<int32_t>, int>> seen;  // small: linear probe by sorted insert
  auto key_of = [](const PodDev& q) {
    return std::vector<int32_t>{q.cpu_req, q.cpu_nz, q.mem, q.milli, q.num, (int32_t)q.tmask};
  };
  for (int i = 0; i < n; ++i) {
    if (ev[i].flags & kPodDelete) { ev[i].pad = -1; continue; }
    const std::vector<int32_t> k = key_of(ev[i]);
    auto it = std::lower_bound(seen.begin(), seen.end(), k,
                               [](const std::pair<std::vector<int32_t>, int>& a, const std::vector<int32_t>& b) {
                                 return a.first < b;
                               });
    int id;
    if (it != seen.end() && it->first == k) {
      id = it->second;
    } else {
      id = (int)cls.size();
      seen.insert(it, {k, id});
      cls.push_back(ev[i]);
      cls.back().pad = id;
      cn.push_back(0);
    }
    ev[i].pad = id;
    ++cn[id];
  }
  ev_cls.resize(n);
  for (int i = 0; i < n; ++i) ev_cls[i] = ev[i].pad;
}

// ---- k_memo planning (memoised FGD replay, ksim_memo.hpp) ----
struct MemoPlan {
  int K = 0, Cw = 0, nfw = 0, Cmax = 1;  // K: the most workgroups of a replica
  int nwg = 0;                            // workgroups of the launch (Σ Kr)
  std::vector<int> Kr, wgoff;             // [Rg] each replica's workgroups (r06: per replica), its first block
  bool decider = false;  // workgroup 0 decides, 1..K-1 own the classes
  bool hkeys = false;    // the keys in HBM (k_memo<..., kHKeys>): classes whose keys do not fit in LDS
  size_t lds = 0;
  std::vector<PodDev> pod;                  // [Rg][Cmax]
  std::vector<int> owner;                   // [Rg][Cmax]
  std::vector<int> wgcls, wgref;            // [nwg][Cw] (block wgoff[i] + w)
  std::vector<unsigned long long> wggrp;    // [nwg][Cw]
};

// Classes of one replica onto K workgroups, at most Cw slots each.  Classes with the same score
// request (cpu_nz, milli, num) stay in one workgroup (their candidate states are the same, so one
// refresh evaluates them once); groups go largest first to the workgroup with the fewest groups.
// split: a group that fits no workgroup whole is spread over the workgroups with the most free slots
// (each part's workgroup evaluates the group's candidate states for its own classes: the same keys,
// the states evaluated once per part) -- the typed gpuspec traces hold groups of up to 60 classes.
inline bool memo_assign(const std::vector<PodDev>& cls, int K, int Cw, std::vector<int>& slot_cls, std::vector<int>& owner,
                        bool split = false) {
  std::vector<std::pair<std::vector<int32_t>, std::vector<int>>> groups;
  for (int c = 0; c < (int)cls.size(); ++c) {
    const std::vector<int32_t> k{cls[c].cpu_nz, cls[c].milli, cls[c].num};
    auto it = std::find_if(groups.begin(), groups.end(), [&](const auto& g) { return g.first == k; });
    if (it == groups.end()) groups.push_back({k, {c}});
    else it->second.push_back(c);
  }
  std::stable_sort(groups.begin(), groups.end(),
                   [](const auto& a, const auto& b) { return a.second.size() > b.second.size(); });
  std::vector<int> used(K, 0), ng(K, 0);
  slot_cls.assign((size_t)K * Cw, -1);
  owner.assign(cls.size(), -1);
  for (const auto& g : groups) {
    const int sz = (int)g.second.size();
    int best = -1;
    for (int w = 0; w < K; ++w)
      if (used[w] + sz <= Cw && (best < 0 || ng[w] < ng[best] || (ng[w] == ng[best] && used[w] < used[best]))) best = w;
    if (best < 0 && !split) return false;
    for (size_t k = 0; k < g.second.size();) {
      if (best < 0 || used[best] >= Cw) {  // split: the workgroup with the most free slots
        best = 0;
        for (int w = 1; w < K; ++w)
          if (used[w] < used[best]) best = w;
        if (used[best] >= Cw) return false;
        ++ng[best];
      } else if (k == 0) {
        ++ng[best];
      }
      const int c = g.second[k++];
      slot_cls[(size_t)best * Cw + used[best]] = c;
      owner[c] = (best << 8) | used[best];
      ++used[best];
    }
  }
  return true;
}

// forceK > 0: exactly that many workgroups per replica (a wide-hinted group, ksim_engine_set_replica_wgs);
// forceKr: that many for each replica (r06: the hints differ); hkeys_ok: when no K fits the keys in LDS, the keys
// may go to HBM (k_memo<..., kHKeys>, classes split over the workgroups as evenly as the slots allow).
inline bool memo_plan(const PlanInput& in, MemoPlan& pl, int forceK = 0, bool hkeys_ok = false,
                      const std::vector<int>* forceKr = nullptr) {
  using namespace memo;
  const int Rg = (int)in.reps.size();
  if (Rg == 0 || in.N > kMemoMaxRank + 1) return false;
  pl.decider = in.decider;
  pl.Cmax = 1;
  for (const ReplicaView& v : in.reps) pl.Cmax = std::max(pl.Cmax, (int)v.cls->size());
  const int K0 = forceK > 0 ? forceK : in.wgs_req > 0 ? in.wgs_req : std::min(64, in.cus / Rg);
  std::vector<int> Kr(Rg, K0);
  if (forceKr) Kr = *forceKr;
  if ((int)Kr.size() != Rg) return false;
  auto total = [&]() { int t = 0; for (int k : Kr) t += k; return t; };
  auto kmax = [&]() { return *std::max_element(Kr.begin(), Kr.end()); };
  if (*std::min_element(Kr.begin(), Kr.end()) < 1 || kmax() > 64 || total() > in.cus) return false;
  const bool forced = forceK > 0 || forceKr != nullptr;
  const int d0 = pl.decider ? 1 : 0;  // decider mode: classes on workgroups 1..K-1
  std::vector<std::vector<int>> sc(Rg), ow(Rg);
  // the smallest Cw >= Cw0 every replica's classes pack into (split: parts of a group on several workgroups)
  auto pack = [&](int Cw0, bool split) {
    for (int Cw = Cw0; Cw <= kMaxCw; ++Cw) {
      bool ok = true;
      for (int i = 0; ok && i < Rg; ++i) {
        const int K = Kr[i];
        std::vector<int> s1;
        ok = K > d0 && memo_assign(*in.reps[i].cls, K - d0, Cw, s1, ow[i], split);
        if (!ok) break;
        sc[i].assign((size_t)K * Cw, -1);
        std::copy(s1.begin(), s1.end(), sc[i].begin() + (size_t)d0 * Cw);
        for (int& o : ow[i]) o += d0 << 8;
      }
      if (ok) return Cw;
    }
    return 0;
  };
  auto cw0 = [&](int dd) {  // the fewest slots per workgroup that can hold every replica's classes
    int c = 1;
    for (int i = 0; i < Rg; ++i) c = std::max(c, ((int)in.reps[i].cls->size() + Kr[i] - 1 - dd) / std::max(1, Kr[i] - dd));
    return c;
  };
  auto fold_waves = [&](int Cw, bool hk) {  // waves 1..9 need fold buffers on the critical path
    for (int f : {16, 12})
      if (memo_layout(in.N, Cw, f, hk).total <= kLdsMax) return f;
    return 0;
  };
  int Cw = 0, nfw = 0;
  bool hk = false;
  for (;;) {
    Cw = pack(cw0(d0), false);
    nfw = Cw > 0 ? fold_waves(Cw, false) : 0;
    // every workgroup of the launch must be resident (they exchange granules every step)
    if (nfw > 0 && kmax() > 1 && total() > in.resident(memo_layout(in.N, Cw, nfw, false).total)) return false;
    if (nfw > 0) break;
    if (hkeys_ok && !pl.decider) {  // the keys in HBM: LDS holds the cluster and the fold buffers only
      Cw = pack(cw0(0), true);
      nfw = Cw > 0 ? fold_waves(Cw, true) : 0;
      if (nfw > 0 && kmax() > 1 && total() > in.resident(memo_layout(in.N, Cw, nfw, true).total)) return false;
      if (nfw > 0) {
        hk = true;
        break;
      }
    }
    const int K = Kr[0];
    if (forced || in.wgs_req > 0 || K >= 64 || Rg * (K + 1) > in.cus) return false;
    std::fill(Kr.begin(), Kr.end(), K + 1);
  }
  pl.K = kmax();
  pl.nwg = total();
  pl.Kr = Kr;
  pl.wgoff.assign(Rg, 0);
  for (int i = 1; i < Rg; ++i) pl.wgoff[i] = pl.wgoff[i - 1] + Kr[i - 1];
  pl.Cw = Cw;
  pl.nfw = nfw;
  pl.hkeys = hk;
  pl.lds = memo_layout(in.N, Cw, nfw, hk).total;
  pl.pod.assign((size_t)Rg * pl.Cmax, PodDev{});
  pl.owner.assign((size_t)Rg * pl.Cmax, -1);
  pl.wgcls.assign((size_t)pl.nwg * Cw, -1);
  pl.wgref.assign((size_t)pl.nwg * Cw, 0);
  pl.wggrp.assign((size_t)pl.nwg * Cw, 0ull);
  for (int i = 0; i < Rg; ++i) {
    const std::vector<PodDev>& cls = *in.reps[i].cls;
    for (size_t c = 0; c < cls.size(); ++c) {
      pl.pod[(size_t)i * pl.Cmax + c] = cls[c];
      pl.owner[(size_t)i * pl.Cmax + c] = ow[i][c];
    }
    for (int w = 0; w < Kr[i]; ++w) {
      const size_t o = ((size_t)pl.wgoff[i] + w) * Cw;
      for (int j = 0; j < Cw; ++j) {
        const int c = sc[i][(size_t)w * Cw + j];
        pl.wgcls[o + j] = c;
        pl.wgref[o + j] = j;
        if (c < 0) continue;
        for (int j2 = 0; j2 < j; ++j2) {  // first slot with the same score request
          const int c2 = sc[i][(size_t)w * Cw + j2];
          if (c2 >= 0 && cls[c2].cpu_nz == cls[c].cpu_nz && cls[c2].milli == cls[c].milli && cls[c2].num == cls[c].num) {
            pl.wgref[o + j] = j2;
            break;
          }
        }
        pl.wggrp[o + pl.wgref[o + j]] |= 1ull << j;
      }
    }
  }
  return true;
}

// The per-event and per-block tables of a k_memo launch, at `stride` events per replica.
struct MemoEvents {
  std::vector<int> evo;    // [Rg][stride] owner code of every event: workgroup << 16 | first slot of its score group << 8
                           // | slot; -1 delete
  std::vector<int> evcls;  // [Rg][stride] class of every event, -1 delete (decider mode)
  std::vector<int> wgmap;  // [nwg] each block's replica position << 8 | workgroup (MemoArgs::wg_map)
};
inline MemoEvents memo_events(const PlanInput& in, const MemoPlan& pl, int stride) {
  const int Rg = (int)in.reps.size();
  MemoEvents t;
  t.evcls.assign((size_t)Rg * stride, -1);
  t.evo.assign((size_t)Rg * stride, -1);
  for (int gi = 0; gi < Rg; ++gi) {
    const std::vector<int>& ec = *in.reps[gi].ev_cls;
    for (size_t i = 0; i < ec.size(); ++i) {
      t.evcls[(size_t)gi * stride + i] = ec[i];
      if (ec[i] < 0) continue;
      const int o = pl.owner[(size_t)gi * pl.Cmax + ec[i]];
      const int w = o >> 8, slot = o & 0xff;
      const int ref = pl.wgref[((size_t)pl.wgoff[gi] + w) * pl.Cw + slot];
      t.evo[(size_t)gi * stride + i] = (w << 16) | (ref << 8) | slot;
    }
  }
  t.wgmap.resize((size_t)pl.nwg);
  for (int gi = 0; gi < Rg; ++gi)
    for (int w = 0; w < pl.Kr[gi]; ++w) t.wgmap[(size_t)pl.wgoff[gi] + w] = (gi << 8) | w;
  return t;
}

// ---- k_hmemo planning (memoised FGD replay with the keys in HBM, ksim_hmemo.hpp) ----
struct HPlan {
  int Cmax = 1, Gmax = 1, Smax = 1, Npad = 0, nb = 0;
  int K = 1, S = 0, nbw = 0;      // workgroups per replica, ranks per workgroup, L1 blocks per workgroup
  bool l2 = false;                // the second maxima beside L1 (the wide form, when they fit in LDS; KSIM_VARIANT hl2)
  size_t lds = 0;
  std::vector<int> cg;            // [Rg][2] classes, groups
  std::vector<PodDev> cls, gpod;  // [Rg][Cmax] (sorted by group), [Rg][Gmax]
  std::vector<uint16_t> cgrp;     // [Rg][Cmax]
  std::vector<int> evc;           // [Rg][stride] class slot of each event, -1 delete
  std::vector<NodeRec> st;        // [Rg][Smax] distinct initial node states
  std::vector<int> ns;            // [Rg]
  std::vector<int> nstate;        // [Rg][Npad] state of each rank, -1 padding
  // Typed replicas (a GPU typical pod names models): per GPU model of the cluster, the typical table cut to
  // the CPU-only pods and the GPU pods that accept the model (ksim_hmemo.hpp, "per-model tables")
  int Mtab = 0, Mslots = 0;       // longest replica's concatenated tables, most models of one replica
  std::vector<int> mtoff;         // [Rg][KSIM_MAX_TYPES] kMtPresent | slot << 21 | entries << 12 | offset
  std::vector<uint8_t> mtab;      // [Rg][Mtab] typical-table index of each entry
};

// Classes of each replica grouped by score request (cpu_nz, milli, num: the candidate states of
// fgd_score.go:99-149 depend on nothing else), and the distinct initial node states (the keys
// before the first event depend on the state, the class and the rank only).
inline bool hmemo_plan(const PlanInput& in, int stride, HPlan& pl, int forceK = 0, int forceS = 0) {
  using namespace hmemo;
  const int Rg = (int)in.reps.size();
  if (Rg == 0 || in.N > kHRankMax || !in.score_table) return false;
  pl.Npad = (in.N + kFan - 1) / kFan * kFan;
  pl.nb = pl.Npad / kFan;
  // one workgroup per replica while one L1 level covers the cluster; wider clusters are sliced over
  // K co-resident workgroups (at most 64: one granule column per polling lane), S a multiple of 64
  // (run_mode 5 with wgs_per_replica > 1 asks for the wide form on a small cluster too; when the
  // wide grid would not fit the usable CUs a small cluster keeps one workgroup per replica)
  const bool small = in.N <= kMaxNb * kFan;
  pl.K = 1;
  pl.S = in.N;
  pl.nbw = pl.nb;
  if (forceK > 0) {  // a node-sharded group: every shard's slices alike (the caller checked S, K)
    pl.S = forceS;
    pl.K = forceK;
    pl.nbw = forceS / kFan;
  } else if (!small || (in.run_mode == 5 && in.wgs_req > 1)) {
    const HSlices sl = hmemo_slices(in.N, in.wgs_req > 1 ? in.wgs_req : 64, kNoClamp);
    if (sl.S <= kMaxNb * kFan && (size_t)Rg * sl.K <= (size_t)in.cus) {
      pl.S = sl.S;
      pl.K = sl.K;
      pl.nbw = sl.S / kFan;
    } else if (!small) {
      return false;
    }
  }
  std::vector<std::vector<int>> ord(Rg), gof(Rg), slot(Rg), gfirst(Rg), sof(Rg);
  std::vector<std::vector<NodeRec>> sts(Rg);
  pl.Cmax = pl.Gmax = pl.Smax = 1;
  for (int i = 0; i < Rg; ++i) {
    const std::vector<PodDev>& cls = *in.reps[i].cls;
    const std::vector<NodeRec>& rec = *in.reps[i].rec;
    std::vector<std::array<int, 3>> gk;
    gof[i].resize(cls.size());
    for (size_t c = 0; c < cls.size(); ++c) {
      const std::array<int, 3> k{cls[c].cpu_nz, cls[c].milli, cls[c].num};
      const auto it = std::find(gk.begin(), gk.end(), k);
      gof[i][c] = (int)(it - gk.begin());
      if (it == gk.end()) { gk.push_back(k); gfirst[i].push_back((int)c); }
    }
    if ((int)cls.size() > kMaxClasses || (int)gk.size() > kMaxGroups) return false;
    ord[i].resize(cls.size());
    std::iota(ord[i].begin(), ord[i].end(), 0);
    std::stable_sort(ord[i].begin(), ord[i].end(), [&](int a, int b) { return gof[i][a] < gof[i][b]; });
    slot[i].assign(cls.size(), -1);
    for (size_t k = 0; k < ord[i].size(); ++k) slot[i][ord[i][k]] = (int)k;
    pl.Cmax = std::max(pl.Cmax, (int)cls.size());
    pl.Gmax = std::max(pl.Gmax, (int)gk.size());
    // distinct initial states (every field but the rank)
    if (rec.size() != (size_t)in.N) return false;
    std::map<std::array<uint32_t, 7>, int> sid;
    sof[i].assign(pl.Npad, -1);
    for (int j = 0; j < in.N; ++j) {
      const NodeRec& n = rec[j];
      std::array<uint32_t, 7> k;
      std::memcpy(k.data(), &n, sizeof k);
      auto it = sid.find(k);
      if (it == sid.end()) {
        it = sid.emplace(k, (int)sts[i].size()).first;
        sts[i].push_back(n);
      }
      sof[i][(int)(n.name_rank - (uint32_t)in.node_off)] = it->second;
    }
    pl.Smax = std::max(pl.Smax, (int)sts[i].size());
  }
  {
    // L2 spares the flagged blocks' key reloads.  They bound the wide form's class waves (C5: 100k nodes, the
    // keys far beyond L2, 55 flagged rows per refresh from HBM), while one workgroup over an openb cluster
    // keeps its keys in L2 and is bound by F: there L2 only adds update work (profiles/r04/hmemo/).
    // Off by default since r05: in the wide form its code alone cost C5 4.09 -> 4.22 s, and it is compiled only into
    // the one-workgroup instantiations; KSIM_VARIANT=hl2=1 turns it on there.
    const bool want = in.hl2 && pl.K == 1;
    pl.l2 = want && hmemo_layout(pl.S, pl.Cmax, pl.Gmax, pl.nbw, true, 0).total <= kLdsMax;
  }
  {  // per-model tables of the typed replicas (KSIM_VARIANT=hmodel=0: the whole table for every model, as before r05)
    pl.Mtab = pl.Mslots = 0;
    pl.mtoff.assign((size_t)Rg * KSIM_MAX_TYPES, 0);
    std::vector<std::vector<uint8_t>> mt(Rg);
    for (int i = 0; in.hmodel && pl.K == 1 && i < Rg; ++i) {  // (the wide form evaluates the whole table)
      const ReplicaView& v = in.reps[i];
      if (!v.typed || v.tp->size() != (size_t)v.nt) continue;
      const std::vector<TypDev>& tpv = *v.tp;
      uint32_t models = 0u;
      for (const NodeRec& n : *v.rec) models |= 1u << n.gpu_type;
      int slot = 0;
      for (int m = 0; m < KSIM_MAX_TYPES; ++m) {
        if (!((models >> m) & 1u)) continue;
        const int off = (int)mt[i].size();
        for (int t = 0; t < v.nt; ++t)
          if (t < v.ncpu || (tpv[t].tmask >> m) & 1u) mt[i].push_back((uint8_t)t);
        const int len = (int)mt[i].size() - off;
        pl.mtoff[(size_t)i * KSIM_MAX_TYPES + m] = (int)(kMtPresent | (uint32_t)slot << 21 | (uint32_t)len << 12 | (uint32_t)off);
        ++slot;
      }
      pl.Mtab = std::max(pl.Mtab, (int)mt[i].size());
      pl.Mslots = std::max(pl.Mslots, slot);
    }
    // tables that do not fit (a 12-bit offset, or the LDS beside the keys' L1 level): the whole-table form
    // (KSIM_VARIANT hmodel=0), which evaluates the same bits, rather than no k_hmemo at all
    if (pl.Mtab > 4095 || hmemo_layout(pl.S, pl.Cmax, pl.Gmax, pl.nbw, pl.l2, pl.Mtab).total > kLdsMax) {
      pl.Mtab = pl.Mslots = 0;
      std::fill(pl.mtoff.begin(), pl.mtoff.end(), 0);
      for (auto& v : mt) v.clear();
    }
    pl.mtab.assign((size_t)Rg * std::max(pl.Mtab, 1), 0);
    for (int i = 0; i < Rg; ++i) std::copy(mt[i].begin(), mt[i].end(), pl.mtab.begin() + (size_t)i * std::max(pl.Mtab, 1));
  }
  pl.lds = hmemo_layout(pl.S, pl.Cmax, pl.Gmax, pl.nbw, pl.l2, pl.Mtab).total;
  if (pl.lds > kLdsMax) return false;
  pl.cg.assign((size_t)Rg * 2, 0);
  pl.cls.assign((size_t)Rg * pl.Cmax, PodDev{});
  pl.cgrp.assign((size_t)Rg * pl.Cmax, 0);
  pl.gpod.assign((size_t)Rg * pl.Gmax, PodDev{});
  pl.evc.assign((size_t)Rg * stride, -1);
  pl.st.assign((size_t)Rg * pl.Smax, NodeRec{});
  pl.ns.assign(Rg, 0);
  pl.nstate.assign((size_t)Rg * pl.Npad, -1);
  for (int i = 0; i < Rg; ++i) {
    const std::vector<PodDev>& cls = *in.reps[i].cls;
    pl.cg[2 * i] = (int)cls.size();
    pl.cg[2 * i + 1] = (int)gfirst[i].size();
    for (size_t k = 0; k < ord[i].size(); ++k) {
      pl.cls[(size_t)i * pl.Cmax + k] = cls[ord[i][k]];
      pl.cgrp[(size_t)i * pl.Cmax + k] = (uint16_t)gof[i][ord[i][k]];
    }
    // a group's request: its first class's (the score part, fgd_score.go:99-149, is the group's), with the
    // least demanding Filter part of every class of the group -- min CPU, min memory, every accepted GPU
    // model -- so that Filter of it on a node fails only when every class of the group fails (the group
    // pruning of k_hmemo's F list; nothing else reads these fields of a group's request)
    for (size_t g = 0; g < gfirst[i].size(); ++g) pl.gpod[(size_t)i * pl.Gmax + g] = cls[gfirst[i][g]];
    for (size_t c = 0; c < cls.size(); ++c) {
      PodDev& gp = pl.gpod[(size_t)i * pl.Gmax + gof[i][c]];
      gp.cpu_req = std::min(gp.cpu_req, cls[c].cpu_req);
      gp.mem = std::min(gp.mem, cls[c].mem);
      gp.tmask |= cls[c].tmask;
    }
    const std::vector<int>& ec = *in.reps[i].ev_cls;
    for (size_t k = 0; k < ec.size(); ++k) pl.evc[(size_t)i * stride + k] = ec[k] < 0 ? -1 : slot[i][ec[k]];
    std::copy(sts[i].begin(), sts[i].end(), pl.st.begin() + (size_t)i * pl.Smax);
    pl.ns[i] = (int)sts[i].size();
    std::copy(sof[i].begin(), sof[i].end(), pl.nstate.begin() + (size_t)i * pl.Npad);
  }
  return true;
}

// ---- the run plan: everything a persistent run decides, before it launches anything ----
// Which kernel every replica runs on, in which order, on which stream, at what width.  The engine fills a RunPlanInput
// (run_plan_input) once prepare_memo has made the FGD plans, and launches what the plan says.
struct RunReplica {
  int policy = 0;
  bool go_random = false;  // Random on Go's math/rand stream (k_random_go)
  int n_events = 0;
  bool has_delete = false;
  int dpcfg = 0;  // DotProduct: dimExtMethod | normMethod << 4
  unsigned wmask = 0u;  // POL_WEIGHTED: the plugins with a positive weight (wsum::plugin_mask)
};
struct RunPlanInput {
  std::vector<RunReplica> reps;
  int N = 0, cus = 0, wgs_req = 0, run_mode = 0;
  bool report = false;
  int scan1 = 0;  // 0: no k_scan1, 1: the node records in LDS, 2: in VGPRs where they fit
  // the FGD plans of the run (prepare_memo): split: the wide-hinted replicas on k_memo, the others on k_hmemo
  bool split_fgd = false, memo_ok = false, hmemo_ok = false;
  int memo_nwg = 0, hmemo_K = 1;            // k_memo's workgroups in all, k_hmemo's per replica
  std::vector<int> memo_reps, hmemo_reps;   // the replicas of each plan, in its order
  // the run's knobs (RunEnv)
  bool timers = false, scan1_mix = true;
  int side_streams = 4;
};

// Group kinds of a run beside the policies themselves (and scan1::kPolMix)
constexpr int kPolRandomGo = 64;  // the k_random_go replicas
constexpr int kPolFgdH = 66;      // the one-workgroup FGD replicas on k_hmemo beside wide ones on k_memo (split_fgd)

enum GroupKernel { kRunRandomGo, kRunScan1, kRunMemo, kRunHmemo, kRunReplay, kRunNone, kRunWsum };

struct PlanGroup {
  int kind = 0;              // a policy, kPolFgdH, scan1::kPolMix or kPolRandomGo
  int first = 0, count = 0;  // its replicas: RunPlan::order[first .. first + count)
  GroupKernel kernel = kRunReplay;  // (kRunNone: an FGD group the required memoised kernel has no plan for)
  int side = -1;             // its side stream's index; -1: the engine stream
  int K = 1, S = 0;          // k_replay and k_scan1 groups: workgroups per replica, nodes per slice, dynamic LDS bytes
  size_t lds = 0;            // (k_replay: a co-resident grid the device cannot hold is narrowed at launch)
  unsigned wmask = 0u;       // a k_wsum group: the union of its replicas' plugin masks (the launch's LDS layout)
};

struct RunPlan {
  std::vector<int> order;  // the replicas in launch order (uploaded as d_replist)
  std::vector<PlanGroup> groups;
  bool any_delete = false, general = false;  // general: k_replay's instantiation with timers, report stores, deletes
  bool concurrent = false;                   // the groups on side streams, else back to back on the engine stream
  bool reg1 = false;                         // k_scan1 keeps the node records in VGPRs
  int fgd_cus = 0;                           // CUs the FGD groups hold (a k_memo / k_hmemo workgroup fills a CU's registers)
};

// Workgroups per replica for k_replay: every workgroup of a launch must be
// co-resident (they exchange granules every step), so R*K never exceeds one
// workgroup per CU; K = 1 needs no co-residency at all.
inline int choose_wgs(int cus, int N, int wgs_req, int R) {
  // auto: one workgroup per CU up to 64 per replica; large clusters (C5: 100k nodes) go wider
  // so that a slice stays near 384 nodes (one to two FGD evaluation rounds per step)
  int K = wgs_req;
  if (K <= 0) {
    K = std::min(cus / R, 64);
    K = std::max(K, std::min(cus / R, (N + 383) / 384));
  }
  K = std::max(1, std::min(K, replay::kMaxK));
  K = std::min(K, N);
  if (R * K > cus) K = 1;
  return K;
}

// K, S and LDS bytes of a k_replay group: choose_wgs, then narrower slices until the layout fits in LDS (or cannot
// be narrowed further: the launcher refuses a layout that still does not fit).  Returns choose_wgs' own K.
inline int replay_fit(const RunPlanInput& in, bool general, PlanGroup& g) {
  const int K0 = g.K = choose_wgs(in.cus, in.N, in.wgs_req, g.count);
  g.S = (in.N + g.K - 1) / g.K;
  while (replay::replay_lds(g.S, g.kind, general) > kLdsMax && g.K < replay::kMaxK && g.count * (g.K + 1) <= in.cus) {
    ++g.K;
    g.S = (in.N + g.K - 1) / g.K;
  }
  g.lds = replay::replay_lds(g.S, g.kind, general);
  return K0;
}

// The launcher's narrowing of a K > 1 k_replay grid against `cap`, the workgroups the occupancy query says can be
// resident at once: fewer, larger slices when it is short.  lds: the layout's bytes at a slice size.
enum NarrowRefusal { kNarrowOk, kNarrowAsked, kNarrowLds };  // kNarrowAsked: the run's own width holds no replica each
struct ReplayNarrow {
  int K, S;
  NarrowRefusal refused;
};
inline ReplayNarrow replay_narrow(int K, int cap, int Rg, int N, int wgs_req, const std::function<size_t(int S)>& lds) {
  const int S = (N + K - 1) / K;
  if (Rg * K <= cap) return {K, S, kNarrowOk};
  if (wgs_req > 0 && cap < Rg) return {K, S, kNarrowAsked};
  const int K2 = std::max(1, std::min(K, cap / Rg)), S2 = (N + K2 - 1) / K2;
  return {K2, S2, lds(S2) > kLdsMax ? kNarrowLds : kNarrowOk};
}

// Slices of the in-process k_replay shard group (lean cheap policies) over shards of at most nmax nodes: about 384
// nodes each (choose_wgs), at most 256 columns over the world, widened until the layout fits in LDS; not ok when the
// layout does not fit or the exchange would have a single column.  k_req > 0 (KSIM_TEST group_k: the tests' way to a
// wide exchange on a small cluster): that many slices per shard instead of the 384-node rule, under the same clamps.
inline ShardSlices replay_group_slices(int nmax, int world, int cus, int pol, int k_req = 0) {
  int K = std::max(1, std::min(256 / world, k_req > 0 ? k_req : (nmax + 383) / 384));
  K = std::min(K, std::max(1, cus / world));
  K = std::min(K, std::max(1, nmax));  // (the 384-node rule never asks for more slices than nodes; a k_req may)
  int S = (nmax + K - 1) / K;
  while (replay::replay_lds(S, pol, false) > kLdsMax && (K + 1) * world <= std::min(256, cus)) {
    ++K;
    S = (nmax + K - 1) / K;
  }
  return {K, S, world * K >= 2 && replay::replay_lds(S, pol, false) <= kLdsMax};
}

// The replicas ordered into groups: a split FGD run's two plans first, then one group per policy present, the
// Random replicas on Go's stream last (one k_random_go workgroup each).
inline void plan_order(const RunPlanInput& in, RunPlan& pl) {
  const int R = (int)in.reps.size();
  auto add = [&](int kind, int count) {
    PlanGroup g;
    g.kind = kind;
    g.count = count;
    if (count) pl.groups.push_back(g);
  };
  if (in.split_fgd) {  // the wide FGD replicas (k_memo) first, then the one-workgroup ones (k_hmemo): the plans' orders
    pl.order = in.memo_reps;
    pl.order.insert(pl.order.end(), in.hmemo_reps.begin(), in.hmemo_reps.end());
    add(POL_FGD, (int)in.memo_reps.size());
    add(kPolFgdH, (int)in.hmemo_reps.size());
  }
  for (int pol = in.split_fgd ? POL_BESTFIT : POL_FGD; pol <= POL_PWR_FGD; ++pol) {
    int c = 0;
    for (int r = 0; r < R; ++r)
      if (in.reps[r].policy == pol && !in.reps[r].go_random) { pl.order.push_back(r); ++c; }
    add(pol, c);
  }
  {  // the weighted combinations (k_wsum), after the policies' groups and before Go's Random
    int c = 0;
    for (int r = 0; r < R; ++r)
      if (in.reps[r].policy == POL_WEIGHTED) { pl.order.push_back(r); ++c; }
    add(POL_WEIGHTED, c);
  }
  int c = 0;
  for (int r = 0; r < R; ++r)
    if (in.reps[r].go_random) { pl.order.push_back(r); ++c; }
  add(kPolRandomGo, c);
}

// Each group's kernel (with the k_replay fit of those that have no other), and whether the groups run concurrently on
// side streams: when every group is at ONE workgroup per replica (no cross-workgroup exchange, so no co-residency
// needed; a paper-sweep group fills 170 of 256 CUs, the next group's workgroups take the rest).  A group needing K > 1,
// a k_memo launch outside a split FGD run or the profile timers keep the launches back to back on the engine stream.
inline void plan_kernels(const RunPlanInput& in, RunPlan& pl) {
  pl.concurrent = !in.timers && pl.groups.size() >= 2;
  int first = 0;  // (make_run_plan sets g.first afterwards; plan_mix leaves a k_wsum group where it is)
  for (PlanGroup& g : pl.groups) {
    const int g_first = first;
    first += g.count;
    const bool fgd = g.kind == POL_FGD && in.run_mode != 2;
    if (g.kind == kPolRandomGo) {  // one workgroup per replica
      g.kernel = kRunRandomGo;
    } else if (g.kind == POL_WEIGHTED) {  // k_wsum: one workgroup per replica over the whole cluster, no exchange
      g.kernel = kRunWsum;
      g.K = 1;
      g.S = in.N;
      for (int j = g_first; j < g_first + g.count; ++j) g.wmask |= in.reps[pl.order[j]].wmask;
      g.lds = wsum::wsum_lds(in.N, g.wmask, pl.general);  // (the launcher refuses a cluster that does not fit)
    } else if (fgd && in.memo_ok) {  // (a split FGD run's wide group is launched first, behind its gate)
      g.kernel = kRunMemo;
      pl.concurrent = pl.concurrent && in.split_fgd;
    } else if ((fgd || g.kind == kPolFgdH) && in.hmemo_ok) {  // concurrent at one workgroup per replica
      g.kernel = kRunHmemo;
      pl.concurrent = pl.concurrent && (g.kind == kPolFgdH || in.hmemo_K == 1);
    } else {
      const int K0 = replay_fit(in, pl.general, g);
      if (g.kind != kPolFgdH) pl.concurrent = pl.concurrent && g.K == 1;
      // one workgroup per replica, create-only, a cheap policy: the 256-thread k_scan1 (ksim_scan1.hpp)
      const bool one = K0 == 1 && !in.timers && !pl.any_delete && in.scan1 && in.N <= kMaxSlice &&
                       scan1::scan1_serves(g.kind) && scan1::scan1_lds(in.N, g.kind, in.report, pl.reg1) <= kLdsMax;
      if ((fgd || g.kind == kPolFgdH) && in.run_mode >= 3 && in.run_mode <= 5) {
        g.kernel = kRunNone;
      } else if (one) {
        g.kernel = kRunScan1;
        g.K = 1;
        g.S = in.N;
        g.lds = scan1::scan1_lds(in.N, g.kind, in.report, pl.reg1);
      }
    }
  }
}

// The cheap-policy groups a concurrent run would give one k_scan1 launch each become ONE k_scan1_mix launch (policy
// per workgroup), its replicas longest stream first, where the first of them stood: the run then needs one side
// stream beside the FGD group's, whatever the hardware-queue mapping of the process.
inline void plan_mix(const RunPlanInput& in, RunPlan& pl) {
  if (!(pl.concurrent && !pl.any_delete && in.scan1 && in.N <= kMaxSlice && in.scan1_mix &&
        scan1::scan1_lds(in.N, scan1::kPolMix, in.report, pl.reg1) <= kLdsMax))
    return;
  std::vector<int> mix, norder;
  std::vector<PlanGroup> ngroups;
  int f = 0, at = -1, nmix = 0;
  for (const PlanGroup& g : pl.groups) {
    bool m = g.kind >= POL_BESTFIT && g.kind <= POL_RANDOM;
    for (int j = f; m && j < f + g.count; ++j)
      m = g.kind != POL_DOTPROD || in.reps[pl.order[j]].dpcfg == (DIM_MERGE | NORM_MAX << 4);
    if (m) {
      mix.insert(mix.end(), pl.order.begin() + f, pl.order.begin() + f + g.count);
      if (at < 0) at = (int)ngroups.size();
      ++nmix;
    } else {
      ngroups.push_back(g);
      norder.insert(norder.end(), pl.order.begin() + f, pl.order.begin() + f + g.count);
    }
    f += g.count;
  }
  if (nmix < 2) return;
  std::stable_sort(mix.begin(), mix.end(), [&](int x, int y) { return in.reps[x].n_events > in.reps[y].n_events; });
  int off = 0;
  for (int g = 0; g < at; ++g) off += ngroups[g].count;
  norder.insert(norder.begin() + off, mix.begin(), mix.end());
  PlanGroup mg;
  mg.kind = scan1::kPolMix;
  mg.count = (int)mix.size();
  mg.kernel = kRunScan1;
  mg.K = 1;
  mg.S = in.N;
  mg.lds = scan1::scan1_lds(in.N, scan1::kPolMix, in.report, pl.reg1);
  ngroups.insert(ngroups.begin() + at, mg);
  pl.order.swap(norder);
  pl.groups.swap(ngroups);
}

// What a run launches, in which order, on which streams.
inline RunPlan make_run_plan(const RunPlanInput& in) {
  RunPlan pl;
  for (const RunReplica& r : in.reps) pl.any_delete = pl.any_delete || r.has_delete;
  pl.general = in.timers || in.report || pl.any_delete;
  pl.reg1 = in.scan1 == 2 && in.N <= scan1::kBlock * scan1::kRegSlots;
  plan_order(in, pl);
  plan_kernels(in, pl);
  plan_mix(in, pl);
  // The side streams share the process's hardware queues (GPU_MAX_HW_QUEUES, HIP's default 4), and two streams on one
  // queue run their kernels one after the other.  So no more side streams than queues (side_streams): the first
  // group (FGD on k_hmemo, the longest in a paper sweep) gets one to itself, the others take the rest round robin.  A
  // split FGD run's wide k_memo group runs on the engine stream itself, which otherwise only waits: three groups then
  // need two side streams (with three, two groups shared a queue: 64 -> 133 ms for a C4 share, profiles/r06/c4_wide/).
  const int nq = in.side_streams, g_off = in.split_fgd ? 1 : 0;
  int first = 0;
  for (int gi = 0; gi < (int)pl.groups.size(); ++gi) {
    PlanGroup& g = pl.groups[gi];
    g.first = first;
    first += g.count;
    const int j = gi - g_off;
    g.side = !pl.concurrent || j < 0 ? -1 : (j == 0 || nq == 1) ? 0 : 1 + (j - 1) % (nq - 1);
    if (g.kind == kPolFgdH) pl.fgd_cus += g.count;
    else if (g.kind == POL_FGD && in.run_mode != 2)
      pl.fgd_cus += in.memo_ok ? in.memo_nwg : g.count * (in.hmemo_ok ? in.hmemo_K : 1);
  }
  return pl;
}

}  // namespace ksim_plan
