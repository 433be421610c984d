// ksim_desched.hpp -- fragmentation-aware descheduling on the device (planning only).
//
// After a trace has been scheduled the reference can evict the pods that cause the most GPU
// fragmentation and schedule them again (pkg/simulator/deschedule.go:20-47 DescheduleCluster with the
// policies fragOnePod :94-119 and fragMultiPod :121-178; the victim of one node is
// findVictimPodOnNodeFragAware, deschedule_utils.go:73-106).  Here the plan -- which pods, in which
// order -- is made on the device from the last run's results and final node records:
//   k_desched_mark    one thread per event: a delete event that took effect marks its creation event;
//   k_desched_eval    one thread per event: for a pod still bound, F(node) and F(node + pod)
//                     (NodeResource.Add, pkg/type/resource.go:482-512), and the bound-pod count;
//   k_desched_select  one workgroup per replica: the pop / pick / re-key loop of the policy over those
//                     values, victims in eviction order.
// The cosSim policy (:49-92; the victim of one node: findVictimPodOnCosSim, deschedule_utils.go:15-45) shares
// k_desched_mark and has k_cos_eval and k_cos_select of its own, after the frag kernels.  On a node-sharded engine
// the same kernels plan the pods on the shard's own nodes (the ownership rule, eval_bound_node), and k_victim_merge,
// at the end of this file, merges the shards' lists into the cluster's plan.  The host side is one
// driver for all policies: desched_plan in ksim_engine.hip, its arithmetic in ksim_desched_host.hpp.
// The rescheduling itself is the ordinary replay of the extended event stream (ksim/desched.py).
// No kernel here waits for another workgroup, and nothing is on the per-pod path.
//
// fragMultiPod passes the node state built BEFORE its loop on every pop (deschedule.go:124, :156:
// nodeResMap is never updated), so the candidate states of a later pop of the same node are still
// "the original node + one pod"; only the left-hand side of the score moves (the priority stored at
// the previous eviction, :162-163).  F(original node + pod) is therefore computed once per bound pod
// and the loop is pure selection.  Order contract (the reference's is a Go map's and an unstable
// sort's): pods of a node in ascending creation-event index, nodes of equal priority by name rank.
#pragma once

#include "ksim_device.hpp"
#include "ksim_engine.h"

namespace ksim_ds {

using namespace ksim;

// NodeResource.Add(podRes, gpu ids) (resource.go:482-512) on a node state: the verdict, and on success the
// state after it.  CPU left grows by PodResource.MilliCpu (cpu_nz); a pod with GPUs adds its per-GPU milli to
// every device named in `mask`.  False (the reference skips the pod) when the CPU left would exceed the
// capacity, a named device does not exist or a device would exceed 1000 milli left.
KSIM_HD bool node_add(int cpuL, const int (&gl)[kMaxGpu], int gpu_cnt, int cap, int cpu_nz, int milli, int num,
                      unsigned mask, long long* cpu_after, int (&g2)[kMaxGpu]) {
  const long long cpu_new = (long long)cpuL + cpu_nz;
  if (cpu_new > (long long)cap) return false;
  bool ok = true;
#pragma unroll
  for (int g = 0; g < kMaxGpu; ++g) {
    const bool named = num > 0 && ((mask >> g) & 1u);
    const int v = gl[g] + (named ? milli : 0);
    ok = ok && !(named && (g >= gpu_cnt || v > kMilli));
    g2[g] = v;
  }
  if (num > 0 && (mask >> kMaxGpu) != 0u) ok = false;
  *cpu_after = cpu_new;
  return ok;
}

// Add, then F of the result.  *f_after is written only on success.  frag_F is used unchanged: same per-bin
// order, no fused multiply-add.
template <bool kTyped>
KSIM_HD bool victim_eval(int cpuL, const int (&gl)[kMaxGpu], int gpu_cnt, uint32_t typebit, int cap, int cpu_nz,
                         int milli, int num, unsigned mask, const TypDev* __restrict__ tp, int ncpu, int nt,
                         double* f_after) {
  long long cpu_new;
  int g2[kMaxGpu];
  if (!node_add(cpuL, gl, gpu_cnt, cap, cpu_nz, milli, num, mask, &cpu_new, g2)) return false;
  *f_after = frag_F<kTyped>((int)cpu_new, g2, typebit, tp, ncpu, nt);
  return true;
}

// cosSim (deschedule_utils.go:15-45 findVictimPodOnCosSim): the cosine of [CPU left, total milli-GPU left] of
// the node after Add and [MilliCpu, MilliGpu x GpuNumber] of the pod, as CalculateVectorCosineSimilarity
// (pkg/utils/utils.go:1196-1218) writes it: three running sums over the two components, sqrt of the two
// magnitudes, inner / (m1 * m2).  Every component is an integer far below 2^26, so the sums are exact; only the
// two roots, their product and the quotient round, each correctly (no fused multiply-add, no fast math).
// -1 (the reference skips the pod) when Add fails, a magnitude is zero or the value leaves
// [-1e-3, 1 + 1e-3] (GetResourceSimilarity, utils.go:1181-1193).
KSIM_HD double cos_similarity(int cpuL, const int (&gl)[kMaxGpu], int gpu_cnt, int cap, int cpu_nz, int milli, int num,
                              unsigned mask) {
  long long cpu_new;
  int g2[kMaxGpu];
  if (!node_add(cpuL, gl, gpu_cnt, cap, cpu_nz, milli, num, mask, &cpu_new, g2)) return -1.0;
  int tot = 0;
#pragma unroll
  for (int g = 0; g < kMaxGpu; ++g) tot += g2[g];
  const double n0 = (double)cpu_new, n1 = (double)tot;
  const double p0 = (double)cpu_nz, p1 = (double)((long long)milli * (long long)num);
  double m1 = 0.0, m2 = 0.0, inner = 0.0;
  m1 += n0 * n0;
  m2 += p0 * p0;
  inner += n0 * p0;
  m1 += n1 * n1;
  m2 += p1 * p1;
  inner += n1 * p1;
  m1 = __builtin_sqrt(m1);
  m2 = __builtin_sqrt(m2);
  if (m1 == 0.0 || m2 == 0.0) return -1.0;
  const double s = inner / (m1 * m2);
  const double delta = 1e-3;
  if (s < 0.0 - delta || s > 1.0 + delta) return -1.0;
  return s;
}

// What k_desched_eval leaves per event (32 B).  node < 0: not a candidate (a delete event, a pod that
// is not bound any more, or a record that does not validate).
struct __align__(16) EvalRec {
  double f_node;    // F(final state of the node)
  double f_after;   // F(node + pod), valid when ok
  int32_t node;     // local index
  int32_t gpu_mask;
  int32_t ok;       // Add succeeded
  int32_t pad;
};
static_assert(sizeof(EvalRec) == 32, "EvalRec layout");
static_assert(sizeof(ksim_victim) == 40, "ksim_victim layout");

constexpr int kEvalBlock = 256;
constexpr int kSelBlock = 256;
constexpr int kSelNodeBytes = 20;          // per-node tables of k_desched_select: key 8, rank 4, start 4, end 4
constexpr int kSelLdsBytes = 60 * 1024;    // a select kernel's tables sit in LDS up to this size, in HBM beyond
// one replica's tables in HBM: 16-byte aligned, so the 8-byte keys at its start are aligned for any N
KSIM_HD size_t tab_stride(int N, int node_bytes) { return ((size_t)N * node_bytes + 15) & ~(size_t)15; }

struct PlanArgs {          // what the kernels of every policy take
  const ReplicaDev* reps;
  const long long* eoff;   // [R + 1] first event slot of each replica in the per-event buffers
  uint8_t* gone;           // [Σ E] creation events whose delete took effect (k_desched_mark)
  int32_t* bound;          // [R] pods still bound
  const int32_t* budget;   // [R]
  int32_t* n_vict;         // [R]
  uint8_t* tab;            // [R][tab_stride(N, its bytes per node)] the select kernel's tables beyond LDS, else null
  int N;
  int node_off;            // a node-sharded engine: the global rank of its local node 0 (else 0) ...
  int sharded;             // ... and 1: results carry global ranks, and only the owner of a node plans its pods
};

struct DsArgs : PlanArgs {
  EvalRec* eval;           // [Σ E]
  int32_t* plist;          // [Σ E] k_desched_select: candidate events grouped by node
  ksim_victim* vict;       // [Σ E]
  int policy;              // ksim_desched_policy
};

// grid (ceil(E_max / kEvalBlock), R): gone[ref] = 1 for every delete event that took effect.
__global__ __launch_bounds__(kEvalBlock) void k_desched_mark(PlanArgs a) {
  const int r = (int)blockIdx.y;
  const ReplicaDev rp = a.reps[r];
  const int e = (int)blockIdx.x * kEvalBlock + (int)threadIdx.x;
  if (e >= rp.n_events) return;
  const PodDev p = rp.ev[e];
  if (!(p.flags & kPodDelete) || rp.res[e].status != ST_DELETED) return;
  if (p.ref >= 0 && p.ref < e) a.gone[a.eoff[r] + p.ref] = 1;
}

// The opening of both eval kernels, for event e (< n_events) of replica r: returns whether its pod is still bound
// and, when the result record validates, calls body(local index, node, its GPU-left array) inside the two tests, as the
// kernels had it inline (the compiler's output is the same).  The record is validated before it indexes anything:
// the node index before the node is loaded, the mask against the node's GPU count before anything uses it.
// The ownership rule of a node-sharded engine (report_delta_event's): results carry global ranks, local = rank -
// node_off indexes rp.nodes, rp.cap and the select kernels' tables, and a pod counts as bound, and is a candidate,
// only where 0 <= local < N -- the other shards hold a provisional record of that step.  Unsharded, node_off is 0
// and every pod that passes the three tests is bound, as it always was.  body(local, node, GPU-left array).
template <class F>
__device__ __forceinline__ bool eval_bound_node(const PlanArgs& a, const ReplicaDev& rp, int r, int e, const PodDev& p,
                                                const ResultDev& res, F&& body) {
  const int local = res.node >= 0 ? res.node - a.node_off : -1;
  const bool owned = local >= 0 && local < a.N;
  const bool bound = !(p.flags & kPodDelete) && res.status == ST_OK && !a.gone[a.eoff[r] + e] && (owned || !a.sharded);
  if (bound && owned && res.gpu_mask >= 0) {
    const NodeV n = load_node(rp.nodes + local);
    const int cnt = n.gpu_cnt();
    if (cnt <= kMaxGpu && ((unsigned)res.gpu_mask >> cnt) == 0u) {
      int gl[kMaxGpu];
      unpack_gl(n, gl);
      body(local, n, gl);
    }
  }
  return bound;
}

// Their tail, reached by every thread of the block: the pods in the API are every bound pod, candidate or not
// (deschedule.go:21, :27).
__device__ __forceinline__ void count_bound(const PlanArgs& a, int r, bool bound) {
  const unsigned long long m = __ballot(bound);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.bound + r, (int)__popcll(m));
}

// grid (ceil(E_max / kEvalBlock), R), the replica's typical table staged in LDS: the candidate record
// of every event and the replica's bound-pod count.
__global__ __launch_bounds__(kEvalBlock) void k_desched_eval(DsArgs a, const TypDev* __restrict__ tp_all) {
  const int r = (int)blockIdx.y;
  const ReplicaDev rp = a.reps[r];
  __shared__ TypDev s_tp[kMaxTypical];
  {
    const TypDev* tp = tp_all + (size_t)r * kMaxTypical;
    for (int i = (int)threadIdx.x; i < rp.nt * 2; i += kEvalBlock)
      reinterpret_cast<uint4*>(s_tp)[i] = reinterpret_cast<const uint4*>(tp)[i];
    __syncthreads();
  }
  const int e = (int)blockIdx.x * kEvalBlock + (int)threadIdx.x;
  bool bound = false;
  if (e < rp.n_events) {
    EvalRec out;
    out.f_node = 0.0;
    out.f_after = 0.0;
    out.node = -1;
    out.gpu_mask = 0;
    out.ok = 0;
    out.pad = 0;
    const PodDev p = rp.ev[e];
    const ResultDev res = rp.res[e];
    bound = eval_bound_node(a, rp, r, e, p, res, [&](int local, const NodeV& n, const int (&gl)[kMaxGpu]) {
      const int cnt = n.gpu_cnt();
      const uint32_t tb = 1u << n.gpu_type();
      const int cap = rp.cap[local];
      out.node = local;
      out.gpu_mask = res.gpu_mask;
      if (rp.typed) {
        out.f_node = frag_F<true>(n.cpu_left, gl, tb, s_tp, rp.ncpu, rp.nt);
        out.ok = victim_eval<true>(n.cpu_left, gl, cnt, tb, cap, p.cpu_nz, p.milli, p.num, (unsigned)res.gpu_mask,
                                   s_tp, rp.ncpu, rp.nt, &out.f_after) ? 1 : 0;
      } else {
        out.f_node = frag_F<false>(n.cpu_left, gl, tb, s_tp, rp.ncpu, rp.nt);
        out.ok = victim_eval<false>(n.cpu_left, gl, cnt, tb, cap, p.cpu_nz, p.milli, p.num, (unsigned)res.gpu_mask,
                                    s_tp, rp.ncpu, rp.nt, &out.f_after) ? 1 : 0;
      }
    });
    a.eval[a.eoff[r] + e] = out;
  }
  count_bound(a, r, bound);
}

// int64(frag_before - frag_after): fp64 subtraction, truncation toward zero (deschedule_utils.go:92).
// Both are sums of at most 256 terms freq x milli <= 8000, so the difference is far inside int64.
KSIM_HD long long victim_score(double before, double after) { return (long long)(before - after); }

// A node's queue key: the bits of its priority (a non-negative double: monotone as an integer) + 1; 0 = not queued.
KSIM_HD unsigned long long prio_key(double f) { return __builtin_bit_cast(unsigned long long, f) + 1ull; }
KSIM_HD double key_prio(unsigned long long k) { return __builtin_bit_cast(double, k - 1ull); }

struct NodePick {
  unsigned long long key;
  unsigned rank;
  int idx;
};
// (priority desc, name rank asc)
__device__ __forceinline__ bool better(const NodePick& x, const NodePick& y) {
  return x.key > y.key || (x.key == y.key && x.key != 0ull && x.rank < y.rank);
}
__device__ __forceinline__ NodePick wave_best(NodePick v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    NodePick w;
    w.key = __shfl_xor(v.key, o, 64);
    w.rank = __shfl_xor(v.rank, o, 64);
    w.idx = __shfl_xor(v.idx, o, 64);
    if (better(w, v)) v = w;
  }
  return v;
}

// One workgroup per replica.  Setup: the candidates that can ever be a victim (Add succeeded and the score
// against the node's own F is positive: a node's priority only falls, so a score that is not positive now never
// will be) grouped by node -- count, block scan, fill -- and every node with such a candidate queued at F(node).
// Loop, at most once per queued node plus once per unit of budget: pop the node of the highest priority, pick
// its pod of the highest score (ties: the lowest event), emit it and re-key the node with F(node + pod)
// (fragMultiPod) or drop it (fragOnePod: one visit per node); a node without a victim is dropped.
__global__ __launch_bounds__(kSelBlock) void k_desched_select(DsArgs a) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ NodePick s_pick[kSelBlock / 64];
  __shared__ unsigned long long s_pod[kSelBlock / 64];
  __shared__ int s_pj[kSelBlock / 64];
  __shared__ int s_scan[kSelBlock / 64];
  const int r = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  const ReplicaDev rp = a.reps[r];
  const int N = a.N, E = rp.n_events;
  const EvalRec* ev = a.eval + a.eoff[r];
  int32_t* plist = a.plist + a.eoff[r];
  ksim_victim* vict = a.vict + a.eoff[r];
  uint8_t* base = a.tab ? a.tab + (size_t)r * tab_stride(N, kSelNodeBytes) : s_dyn;
  unsigned long long* nkey = reinterpret_cast<unsigned long long*>(base);
  unsigned* nrank = reinterpret_cast<unsigned*>(base + (size_t)N * 8);
  int* nstart = reinterpret_cast<int*>(base + (size_t)N * 12);
  int* nend = reinterpret_cast<int*>(base + (size_t)N * 16);

  for (int i = tid; i < N; i += kSelBlock) {
    nkey[i] = 0ull;
    nrank[i] = rp.nodes[i].name_rank;
    nend[i] = 0;
  }
  __syncthreads();
  for (int e = tid; e < E; e += kSelBlock) {
    const EvalRec c = ev[e];
    if (c.node >= 0 && c.ok && victim_score(c.f_node, c.f_after) > 0) {
      atomicAdd(&nend[c.node], 1);
      nkey[c.node] = prio_key(c.f_node);  // (every candidate of a node stores the same value)
    }
  }
  __syncthreads();
  {  // exclusive scan of the counts: a contiguous chunk per thread, the wave sums by shuffles, the waves through LDS
    const int per = (N + kSelBlock - 1) / kSelBlock;
    const int lo = min(N, tid * per), hi = min(N, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += nend[i];
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_up(incl, o, 64);
      if (lane >= o) incl += x;
    }
    if (lane == 63) s_scan[w] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int i = 0; i < w; ++i) run += s_scan[i];
    for (int i = lo; i < hi; ++i) {
      const int c = nend[i];
      nstart[i] = run;
      nend[i] = run;
      run += c;
    }
  }
  __syncthreads();
  for (int e = tid; e < E; e += kSelBlock) {
    const EvalRec c = ev[e];
    if (c.node >= 0 && c.ok && victim_score(c.f_node, c.f_after) > 0) plist[atomicAdd(&nend[c.node], 1)] = e;
  }
  __syncthreads();

  int left = a.budget[r], nv = 0;
  for (int it = 0; left > 0 && it < N + a.budget[r]; ++it) {
    NodePick best;
    best.key = 0ull;
    best.rank = 0u;
    best.idx = -1;
    for (int i = tid; i < N; i += kSelBlock) {
      NodePick c;
      c.key = nkey[i];
      c.rank = nrank[i];
      c.idx = i;
      if (better(c, best)) best = c;
    }
    best = wave_best(best);
    if (lane == 0) s_pick[w] = best;
    __syncthreads();
    best = s_pick[0];
#pragma unroll
    for (int i = 1; i < kSelBlock / 64; ++i)
      if (better(s_pick[i], best)) best = s_pick[i];
    if (best.key == 0ull) break;  // the queue is empty (uniform: every thread read the same s_pick)
    const double prio = key_prio(best.key);
    // the node's pod of the highest score: key = score << 32 | ~event (score < 2^22: the bound above)
    unsigned long long pk = 0ull;
    int pj = -1;
    for (int j = nstart[best.idx] + tid; j < nend[best.idx]; j += kSelBlock) {
      const int e = plist[j];
      if (e < 0) continue;  // evicted on an earlier pop
      const long long s = victim_score(prio, ev[e].f_after);
      if (s <= 0) continue;
      const unsigned long long k = ((unsigned long long)s << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)e);
      if (k > pk) {
        pk = k;
        pj = j;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long k2 = __shfl_xor(pk, o, 64);
      const int j2 = __shfl_xor(pj, o, 64);
      if (k2 > pk) {
        pk = k2;
        pj = j2;
      }
    }
    if (lane == 0) {
      s_pod[w] = pk;
      s_pj[w] = pj;
    }
    __syncthreads();
    pk = s_pod[0];
    pj = s_pj[0];
#pragma unroll
    for (int i = 1; i < kSelBlock / 64; ++i)
      if (s_pod[i] > pk) {
        pk = s_pod[i];
        pj = s_pj[i];
      }
    if (pk != 0ull) {
      if (tid == 0) {
        const int e = plist[pj];
        const EvalRec c = ev[e];
        ksim_victim v;
        v.event = e;
        v.node = c.node + a.node_off;  // the global rank, as a shard's results carry it
        v.gpu_mask = c.gpu_mask;
        v.reserved = 0;
        v.score = (long long)(pk >> 32);
        v.frag_before = prio;
        v.frag_after = c.f_after;
        vict[nv] = v;
        plist[pj] = -1;
        nkey[best.idx] = a.policy == KSIM_DESCHED_FRAG_MULTI_POD ? prio_key(c.f_after) : 0ull;
      }
      ++nv;
      --left;
    } else if (tid == 0) {
      nkey[best.idx] = 0ull;
    }
    __syncthreads();  // the re-key and the eviction mark before the next pop; s_pick / s_pod free again
  }
  if (tid == 0) a.n_vict[r] = nv;
}

// ---- cosSim (deschedule.go:49-92 descheduleClusterOnCosSim) ----------------------------------------------------
// The node state is the plan-time state for every pod and every node, a node gives one victim at most and the
// walk only counts them, so the plan is: per bound pod its similarity (k_cos_eval), per node the arg-min of
// (similarity, event) over the pods that can be elected, the nodes that pass both bars and have such a pod in
// the order of sortNodeStatusByResource, cut at the budget (k_cos_select).

// What k_cos_eval leaves per event (16 B).  node < 0: not a bound pod, or a record that does not validate.
struct __align__(16) CosRec {
  double sim;  // cos_similarity: -1 when the reference skips the pod
  int32_t node;  // local index
  int32_t gpu_mask;
};
static_assert(sizeof(CosRec) == 16, "CosRec layout");
static_assert(sizeof(ksim_cos_victim) == 32, "ksim_cos_victim layout");

// per-node tables of k_cos_select: the least similarity's bits 8, sort key 8, its pod 4, node index 4
constexpr int kCosNodeBytes = 24;

struct CosArgs : PlanArgs {
  CosRec* rec;             // [Σ E]
  ksim_cos_victim* vict;   // [Σ E]
  long long cpu_bar;       // milliCpuBar: a node at or above it is skipped
  long long gpu_bar;       // milliGpuBar: some device of the node must have more than it left
};

// A pod is elected only with 0 <= similarity < 1 (deschedule_utils.go:34, victimPodSimilarity starts at 1).
// Such doubles are non-negative, so their bit patterns order as integers; + 0.0 folds a negative zero.
KSIM_HD bool cos_elects(double s) { return s >= 0.0 && s < 1.0; }
KSIM_HD unsigned long long cos_bits(double s) { return __builtin_bit_cast(unsigned long long, s + 0.0); }

// grid (ceil(E_max / kEvalBlock), R): the candidate record of every event and the replica's bound-pod count.
__global__ __launch_bounds__(kEvalBlock) void k_cos_eval(CosArgs a) {
  const int r = (int)blockIdx.y;
  const ReplicaDev rp = a.reps[r];
  const int e = (int)blockIdx.x * kEvalBlock + (int)threadIdx.x;
  bool bound = false;
  if (e < rp.n_events) {
    CosRec out;
    out.sim = -1.0;
    out.node = -1;
    out.gpu_mask = 0;
    const PodDev p = rp.ev[e];
    const ResultDev res = rp.res[e];
    bound = eval_bound_node(a, rp, r, e, p, res, [&](int local, const NodeV& n, const int (&gl)[kMaxGpu]) {
      out.node = local;
      out.gpu_mask = res.gpu_mask;
      out.sim = cos_similarity(n.cpu_left, gl, n.gpu_cnt(), rp.cap[local], p.cpu_nz, p.milli, p.num,
                               (unsigned)res.gpu_mask);
    });
    a.rec[a.eoff[r] + e] = out;
  }
  count_bound(a, r, bound);
}

// One workgroup per replica.  The arg-min in two passes over the events (the 64-bit similarity and the event do
// not fit one atomic): the least bits per node, then the least event among the pods that have them.  The nodes
// that pass both bars and have a victim are compacted (in any order: the sort decides) with the key
// (8000 - total milli-GPU left) << 32 | name_rank, sorted ascending by a bitonic network over exactly M entries
// (every exchange moves the smaller key down, so the entries a power of two would add above M, all +inf, never
// move and are never stored), and the first min(M, budget) are written out.  Ties of the key (name ranks that
// are not unique) fall back on the node index, so the plan is the same on every run.
__global__ __launch_bounds__(kSelBlock) void k_cos_select(CosArgs a) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ int s_m;
  const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
  const ReplicaDev rp = a.reps[r];
  const int N = a.N, E = rp.n_events;
  const CosRec* rec = a.rec + a.eoff[r];
  ksim_cos_victim* vict = a.vict + a.eoff[r];
  uint8_t* base = a.tab ? a.tab + (size_t)r * tab_stride(N, kCosNodeBytes) : s_dyn;
  unsigned long long* nbits = reinterpret_cast<unsigned long long*>(base);
  unsigned long long* skey = reinterpret_cast<unsigned long long*>(base + (size_t)N * 8);
  unsigned* nev = reinterpret_cast<unsigned*>(base + (size_t)N * 16);
  int* sidx = reinterpret_cast<int*>(base + (size_t)N * 20);
  constexpr unsigned kNone = 0xFFFFFFFFu;

  if (tid == 0) s_m = 0;
  for (int i = tid; i < N; i += kSelBlock) {
    nbits[i] = ~0ull;
    nev[i] = kNone;
  }
  __syncthreads();
  for (int e = tid; e < E; e += kSelBlock) {
    const CosRec c = rec[e];
    if (c.node >= 0 && c.node < N && cos_elects(c.sim)) atomicMin(&nbits[c.node], cos_bits(c.sim));
  }
  __syncthreads();
  for (int e = tid; e < E; e += kSelBlock) {
    const CosRec c = rec[e];
    if (c.node >= 0 && c.node < N && cos_elects(c.sim) && cos_bits(c.sim) == nbits[c.node])
      atomicMin(&nev[c.node], (unsigned)e);
  }
  __syncthreads();
  for (int i = tid; i < N; i += kSelBlock) {
    if (nev[i] == kNone) continue;
    const NodeV n = load_node(rp.nodes + i);
    if ((long long)n.cpu_left >= a.cpu_bar) continue;
    const int cnt = min(n.gpu_cnt(), kMaxGpu);
    int gl[kMaxGpu];
    unpack_gl(n, gl);
    bool pass = false;
    int tot = 0;
#pragma unroll
    for (int g = 0; g < kMaxGpu; ++g) {
      pass = pass || (g < cnt && (long long)gl[g] > a.gpu_bar);
      tot += gl[g];
    }
    if (!pass) continue;
    const int slot = atomicAdd(&s_m, 1);  // < N: one slot per node at most
    skey[slot] = ((unsigned long long)(unsigned)(kMaxGpu * kMilli - min(tot, kMaxGpu * kMilli)) << 32) |
                 (unsigned long long)n.name_rank;
    sidx[slot] = i;
  }
  __syncthreads();
  const int M = s_m;
  for (unsigned long long k = 2; (k >> 1) < (unsigned long long)M; k <<= 1) {
    for (unsigned long long j = k >> 1; j > 0; j >>= 1) {
      const bool flip = j == (k >> 1);  // the first step of a stage pairs i with its mirror in the block of k
      for (unsigned long long t = (unsigned long long)tid; t < (k >> 1) * ((unsigned long long)M / k + 1);
           t += kSelBlock) {
        const unsigned long long i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const unsigned long long l = flip ? (i ^ (k - 1)) : (i | j);
        if (l >= (unsigned long long)M) continue;  // (i < l)
        const unsigned long long ki = skey[i], kl = skey[l];
        const int xi = sidx[i], xl = sidx[l];
        if (ki > kl || (ki == kl && xi > xl)) {
          skey[i] = kl;
          skey[l] = ki;
          sidx[i] = xl;
          sidx[l] = xi;
        }
      }
      __syncthreads();
    }
  }
  const int nv = min(M, a.budget[r]);
  for (int k = tid; k < nv; k += kSelBlock) {
    const int i = sidx[k];
    const int e = (int)nev[i];
    const CosRec c = rec[e];
    ksim_cos_victim v;
    v.event = e;
    v.node = i + a.node_off;
    v.gpu_mask = c.gpu_mask;
    v.reserved = 0;
    v.gpu_left_milli = (long long)(kMaxGpu * kMilli) - (long long)(skey[k] >> 32);
    v.similarity = c.sim;
    vict[k] = v;
  }
  if (tid == 0) a.n_vict[r] = nv;
}

// ---- the merge of the shards' plans (node-sharded cluster) -------------------------------------------------------
// A node's pops depend only on its own pods and its own priority history, so the cluster's victim list is the merge of
// the shards' lists by the key the select kernels walk in -- (frag_before descending, global rank ascending), for
// cosSim (gpu_left_milli descending, rank ascending) -- cut at the cluster's budget.  Every shard's list is sorted by
// that key and the key is unique (DESIGN.md "Descheduling on shards").

struct MergeKey {
  unsigned long long prio;  // higher first
  unsigned rank;            // then lower first
};
__host__ __device__ inline bool key_before(const MergeKey& x, const MergeKey& y) {
  return x.prio > y.prio || (x.prio == y.prio && x.rank < y.rank);
}
// frag_before is a non-negative double (its bits order as an integer, + 0.0 folds a negative zero); gpu_left_milli is
// at most 8000 and never negative.
__host__ __device__ inline MergeKey merge_key(const ksim_victim& v) {
  return MergeKey{__builtin_bit_cast(unsigned long long, v.frag_before + 0.0), (unsigned)v.node};
}
__host__ __device__ inline MergeKey merge_key(const ksim_cos_victim& v) {
  return MergeKey{(unsigned long long)v.gpu_left_milli, (unsigned)v.node};
}

constexpr int kMergeWorld = 16;
constexpr int kMergeBlock = 256;

template <class V>
struct MergeArgs {
  const V* part[kMergeWorld];  // each shard's list, sorted by the key
  int n[kMergeWorld];          // its length, clamped to its buffer on the host and here to >= 0
  int world;
  int budget;                  // the cluster's
  V* out;                      // [out_cap] the merged list
  int out_cap;
  int32_t* n_out;              // min(budget, sum of n), at most out_cap
};

// grid ceil(sum n / kMergeBlock): one thread per input entry.  The entry at position i of shard k counts, in every
// other shard's list, the entries with a strictly better key (a binary search: the lists are sorted and the keys
// unique); i plus those counts is its place in the merged order, and it stores its record there when that is inside
// the budget.  Plain stores to distinct places; no workgroup waits for another; every loop is bounded (world <= 16,
// a search halves an int range: <= 32 steps).
// The arguments sit in device memory (a table indexed by the shard: plain loads, no copy of it per thread).
template <class V>
__global__ __launch_bounds__(kMergeBlock) void k_victim_merge(const MergeArgs<V>* __restrict__ ap) {
  const MergeArgs<V>& a = *ap;
  const int world = min(max(a.world, 0), kMergeWorld);
  long long t = (long long)blockIdx.x * kMergeBlock + (long long)threadIdx.x;
  long long total = 0;
  int k = -1, i = 0;
  for (int j = 0; j < world; ++j) {
    const int nj = max(a.n[j], 0);
    if (k < 0 && t >= total && t < total + nj) {
      k = j;
      i = (int)(t - total);
    }
    total += nj;
  }
  const long long cut = min(min((long long)max(a.budget, 0), total), (long long)max(a.out_cap, 0));
  if (t == 0) *a.n_out = (int32_t)cut;
  if (k < 0) return;
  const V mine = a.part[k][i];
  const MergeKey key = merge_key(mine);
  long long pos = i;
  for (int j = 0; j < world; ++j) {
    if (j == k) continue;
    int lo = 0, hi = max(a.n[j], 0);  // the first entry of list j that is not before `mine`
    for (int s = 0; s < 32 && lo < hi; ++s) {
      const int mid = lo + ((hi - lo) >> 1);
      if (key_before(merge_key(a.part[j][mid]), key)) lo = mid + 1;
      else hi = mid;
    }
    pos += lo;
  }
  if (pos < cut) a.out[pos] = mine;
}

}  // namespace ksim_ds
