// ksim_engine.hip -- MI355X (gfx950) scoring engine for the simulator's per-pod
// Filter+Score pass, behind the C ABI of include/ksim_engine.h.
//
// Device layout (HBM, struct-of-records, replica-major):
//   NodeRec  nodes[R][N]   32 B: cpu/mem left, 8 x u16 milli-GPU left, pods left,
//                          gpu count, model id, name rank
//   uint16   tags[R][N][16] GpuClustering affinity counts
//   PodDev   ev_r[E_r]      32 B per event, per replica
//   TypDev   tp[R][256]     typical-pod table (staged into LDS per workgroup)
//   ResultDev res_r[E_r]    24 B per event
//
// One pod step of every replica is ONE kernel launch (k_step):
//   workgroup (256 threads) = one replica x `nodes_per_block` nodes
//   phase 1  one thread per node: Filter; cheap policies score here
//   phase 2  FGD only: the (node, candidate placement) pairs of the workgroup
//            are compacted into an LDS work list and every thread evaluates
//            F = NodeGpuShareFragAmountScore of one candidate state against the
//            LDS-staged typical table (sequential fp64 bins, bit-exact)
//   phase 3  per node: score = int64(sigmoid((F0-Fk)/1000)*100), packed
//            argmax key (score | ~name_rank | gpu), workgroup max-reduce
//   commit   relaxed agent-scope atomics into the replica's Accum; the
//            workgroup that takes the last ticket reads the winner, runs
//            Reserve's GPU selector on it and scatters the Bind update.
// Steps are captured K at a time into a hipGraph (kernel i reads step = base+i;
// a one-thread kernel advances base) so a whole trace replays with no host
// round trip per pod.
#include <dlfcn.h>
#include <unistd.h>
#include <string>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <map>
#include <numeric>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>
#include <chrono>
#include <thread>

#include "ksim_device.hpp"
#include "ksim_engine.h"
#include "ksim_plan.hpp"

using namespace ksim;
using namespace ksim_plan;

namespace {

constexpr int kBlock = 256;
constexpr int kNBMax = 64;
constexpr int kMaxCand = 9;
constexpr int kTagStride = ksim_plan::replay::kTagStride;

struct StepArgs {
  ReplicaDev* reps;
  Accum* acc;
  int N;
  int NB;
  int bpr;        // workgroups per replica
  int rep_first;  // first replica of this launch
  const int* base;
  int step_off;
  const PodDev* pod_override;  // single-pod calls
  ResultDev* res_override;
  int mode;  // 0: commit (Reserve+Bind), 1: Filter+Score outputs only, 2: shard totals -> send
  unsigned long long* send;        // mode 2: this shard's {best key, nfeas, err, lo | hi << 32}
  const unsigned long long* recv;  // k_shard_commit: the `world` gathered shard records
  int world;
  uint8_t* out_feas;
  int32_t* out_score;
  int32_t* out_gpu;
};

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// allocateGpuId (open_gpu_share.go:252-283) on one node: the replica's gpuSelMethod.
// fgd_gpu: the FGD selector's device for share pods (first max-score index), -1 if none.
// Returns the GPU mask, 0 for pods without GPU milli, -1 where the reference panics / returns "".
// fgd_gpu: the FGD / PWR selectors' GPU index; for SEL_DOTPROD the best match group's GPU mask
// (dotprod_cfg_score, 0 = "": Reserve fails).
__device__ int select_gpus(const NodeV& n, const PodDev& p, int gpusel, int fgd_gpu, uint64_t seed, int step) {
  if (p.milli <= 0) return 0;                                         // open_gpu_share.go:185-187
  if (p.milli < kMilli && p.num > 1) return -1;                       // :266-268 panic
  if (gpusel == SEL_DOTPROD) return fgd_gpu <= 0 ? -1 : fgd_gpu;      // dot_product_score.go:102-107
  if (!is_share_pod(p)) return exclusive_gpu_mask(n, p);              // exclusive branch of every selector
  switch (gpusel) {
    case SEL_FGD:                                                     // fgd_score.go:153-156
    case SEL_PWR:                                                     // pwr_score.go:214-219
      return fgd_gpu < 0 ? -1 : (1 << fgd_gpu);
    case SEL_RANDOM: {                                                // :325-343 (Random contract)
      const uint64_t nk = rand_node_key(seed, step, n.name_rank);
      int pick = -1;
      uint64_t best = 0;
      for (int g = 0; g < kMaxGpu; ++g) {
        if (g < n.gpu_cnt() && n.gl(g) >= p.milli) {
          const uint64_t k = rand_gpu_key(nk, g);
          if (pick < 0 || k > best) { best = k; pick = g; }
        }
      }
      return pick < 0 ? -1 : (1 << pick);
    }
    case SEL_WORST: {                                                 // :305-323
      int c = -1, cv = 0;
#pragma unroll
      for (int g = 0; g < kMaxGpu; ++g) {
        const int v = n.gl(g);
        if (g < n.gpu_cnt() && v >= p.milli && (c < 0 || v > cv)) { c = g; cv = v; }
      }
      return c < 0 ? -1 : (1 << c);
    }
    default: {                                                        // best fit, :285-303
      int c = -1, cv = 0;
#pragma unroll
      for (int g = 0; g < kMaxGpu; ++g) {
        const int v = n.gl(g);
        if (g < n.gpu_cnt() && v >= p.milli && (c < 0 || v < cv)) { c = g; cv = v; }
      }
      return c < 0 ? -1 : (1 << c);
    }
  }
}

// Bind on a register image (see apply_bind).
__device__ __forceinline__ void bind_node(NodeV& n, const PodDev& p, int mask, int sign) {
  n.cpu_left -= sign * p.cpu_req;
  n.mem_left -= sign * p.mem;
  const int pods = n.pods_left() - sign;
  n.meta = (n.meta & 0xffff0000u) | ((uint32_t)pods & 0xffffu);
  const uint32_t d = (uint32_t)(sign * (int)p.milli) & 0xffffu;
#pragma unroll
  for (int g = 0; g < kMaxGpu; ++g) {
    // u16 lanes never borrow across halves: 0 <= left - milli and left + milli <= 1000
    if ((mask >> g) & 1) n.g[g >> 1] = (g & 1) ? n.g[g >> 1] - (d << 16) : ((n.g[g >> 1] & 0xffff0000u) | ((n.g[g >> 1] - d) & 0xffffu));
  }
}

// Bind: scheduler cache assume (Requested += pod), open-gpu-share cache
// AddOrUpdatePod (devices += milli), NodeInfo.Pods += pod (affinity tags).
__device__ void apply_bind(NodeRec* nr, uint16_t* tags, const PodDev& p, int mask, int sign) {
  NodeV n = load_node(nr);
  n.cpu_left -= sign * p.cpu_req;
  n.mem_left -= sign * p.mem;
  const int pods = n.pods_left() - sign;
  n.meta = (n.meta & 0xffff0000u) | ((uint32_t)pods & 0xffffu);
  const uint32_t d = (uint32_t)(sign * (int)p.milli) & 0xffffu;
#pragma unroll
  for (int g = 0; g < kMaxGpu; ++g) {
    // u16 lanes never borrow across halves: 0 <= left - milli and left + milli <= 1000
    if ((mask >> g) & 1) n.g[g >> 1] = (g & 1) ? n.g[g >> 1] - (d << 16) : ((n.g[g >> 1] & 0xffff0000u) | ((n.g[g >> 1] - d) & 0xffffu));
  }
  store_node(nr, n);
  if (p.tag >= 0) tags[p.tag] = (uint16_t)((int)tags[p.tag] + sign);
}

// Cluster report bookkeeping of k_step: the state event `step` left on `node` and the previous
// event that changed it (k_replay keeps the same per-node record in LDS).
__device__ __forceinline__ void note_change(const ReplicaDev& rp, int node, int step) {
  store_node(rp.snap + step, load_node(rp.nodes + node));
  rp.prev[step] = rp.last[node];
  rp.last[node] = step;
}

// Bit g set iff GPU g fits `milli` and no lower-index fitting GPU has the same milli left.
__device__ __forceinline__ unsigned first_of_class(const NodeV& n, int milli) {
  unsigned fm = 0u;
  const int cnt = n.gpu_cnt();
#pragma unroll
  for (int g = 0; g < kMaxGpu; ++g) {
    const int v = n.gl(g);
    bool first = g < cnt && v >= milli;
#pragma unroll
    for (int h = 0; h < g; ++h) first = first && !(n.gl(h) == v);
    fm |= first ? (1u << g) : 0u;
  }
  return fm;
}

// ---------------------------------------------------------------------------
// Per-node pieces shared by k_step (one launch per pod) and k_replay (persistent).
// ---------------------------------------------------------------------------

// The selector argument of select_gpus for a winner `n` (global node index `node`): the FGD / PWR
// GPU index from the key, or DotProduct's best-group mask recomputed on the node.
// kDp = false: a kernel specialised on a policy other than DotProduct (no DotProduct selector there).
template <bool kDp = true>
__device__ __forceinline__ int sel_arg(const ReplicaDev& rp, const NodeV& n, const PodDev& p, int node, int key_gpu) {
  if (!kDp || rp.gpusel != SEL_DOTPROD) return key_gpu;
  int gid = 0;
  (void)dotprod_cfg_score(n, p, dp_norm(rp.dpcfg) == NORM_NODE ? rp.cap[node] : 0, rp.dpcfg, &gid);
  return gid;
}

// Raw score of a feasible node under a non-FGD policy (compile-time policy, used by
// k_replay); *err on a Score error.  Same functions and semantics as node_phase1.
// `cap`: the node's MilliCpuCapacity (DotProduct's normMethod "node").
template <int kPol>
__device__ __forceinline__ int cheap_score(const NodeV& n, const PodDev& p, uint64_t seed, const uint16_t* tags,
                                           int step, bool* err, int dpcfg = 0, int cap = 0) {
  *err = false;
  if constexpr (kPol == POL_BESTFIT) {
    const int r = bestfit_score(n, p, n.total());
    if (r == -1) { *err = true; return kBfKeyBias; }
    return r + kBfKeyBias;  // biased (kBfKeyBias)
  } else if constexpr (kPol == POL_DOTPROD) {
    int gid = 0;
    // uniform per replica
    const int r = dpcfg == (DIM_MERGE | NORM_MAX << 4) ? dotprod_merge_max(n, p) : dotprod_cfg_score(n, p, cap, dpcfg, &gid);
    *err = r < 0 || r > 100;  // no NormalizeScore: the framework's range check (framework.go:686-704)
    return r;
  } else if constexpr (kPol == POL_PACKING) {
    bool perr = false;
    const int r = p.milli <= 0 ? 0 : packing_score(n, p, &perr);
    *err = perr;
    return r;
  } else if constexpr (kPol == POL_CLUSTERING) {
    if (p.tag == -2) { *err = true; return 0; }
    return clustering_score(tags, p.tag, n.total());
  } else {
    return (int)(rand_node_key(seed, step, n.name_rank) >> 40);
  }
}

// Filter, then the cheap scores; for FGD only the candidate count.  `tags` may
// point at global memory (k_step) or LDS (k_replay).
__device__ __forceinline__ bool node_phase1(const NodeV& n, const PodDev& p, const ReplicaDev& rp,
                                            const uint16_t* tags, int step, bool share, int* raw, int* nc,
                                            bool* err, int node = 0, int* pgpu = nullptr) {
  *raw = 0;
  *nc = 0;
  *err = false;
  if (!filter_node(n, p)) return false;
  const int total = n.total();
  switch (rp.policy) {
    case POL_FGD:
      // one candidate per DISTINCT milli-left value among the fitting GPUs: placing the pod on
      // any GPU of a value class yields the same multiset of GPU states, hence the same F
      // (frag.go depends on the multiset only) and the same score.
      *nc = share ? 1 + __builtin_popcount(first_of_class(n, p.milli)) : 2;
      break;
    case POL_BESTFIT:
      *raw = bestfit_score(n, p, total);
      *err = *raw == -1;
      *raw = (*err ? 0 : *raw) + kBfKeyBias;  // biased (kBfKeyBias)
      break;
    case POL_DOTPROD: {  // any dimExtMethod / normMethod; *pgpu: the best group's GPU mask
      int gid = 0;
      *raw = dotprod_cfg_score(n, p, rp.cap[node], rp.dpcfg, &gid);
      *err = *raw < 0 || *raw > 100;  // no NormalizeScore: the framework's range check
      if (pgpu) *pgpu = gid;
      break;
    }
    case POL_PACKING: {
      bool perr = false;
      *raw = p.milli <= 0 ? 0 : packing_score(n, p, &perr);
      *err = perr;
      break;
    }
    case POL_CLUSTERING:
      if (p.tag == -2) *err = true;
      else *raw = clustering_score(tags, p.tag, total);
      break;
    case POL_PWR:
    case POL_PWR_FGD: {  // pwr_score.go:48-91 (+ FGD's candidates for the weighted combination)
      int g = -1;
      bool perr = false;
      *raw = pwr_score(n, p, rp.cap[node], rp.cpum[node], *rp.pw, &g, &perr);
      *err = perr;
      if (pgpu) *pgpu = g;
      if (rp.policy == POL_PWR_FGD) *nc = share ? 1 + __builtin_popcount(first_of_class(n, p.milli)) : 2;
      break;
    }
    default:  // POL_RANDOM: RandomScorePlugin.PreScore pick, as a 24-bit hash key
      *raw = (int)(rand_node_key(rp.seed, step, n.name_rank) >> 40);
      break;
  }
  return true;
}

// FGD work list of one node: current state, then one candidate per GPU value class
// (share pod) or the NodeResource.Sub state.
__device__ __forceinline__ void emit_fgd_items(const NodeV& n, const PodDev& p, bool share, int local, int o,
                                               uint8_t* item_node, uint8_t* item_code) {
  item_node[o] = (uint8_t)local;
  item_code[o] = 0;  // current state
  ++o;
  if (share) {
    const unsigned fm = first_of_class(n, p.milli);
#pragma unroll
    for (int g = 0; g < kMaxGpu; ++g) {
      if ((fm >> g) & 1u) {
        item_node[o] = (uint8_t)local;
        item_code[o] = (uint8_t)(1 + g);  // fgd_score.go:111-118 candidate on GPU g
        ++o;
      }
    }
  } else {
    item_node[o] = (uint8_t)local;
    item_code[o] = 9;  // fgd_score.go:137-141 NodeResource.Sub
  }
}

// F of one candidate state.
__device__ __forceinline__ double eval_fgd_item(const NodeV& m, int code, const PodDev& p, const ReplicaDev& rp,
                                                const TypDev* __restrict__ tp) {
  int gl[kMaxGpu];
  unpack_gl(m, gl);
  int cpuL = m.cpu_left;
  if (code >= 1 && code <= 8) {
    cpuL -= p.cpu_nz;
#pragma unroll
    for (int g = 0; g < kMaxGpu; ++g) gl[g] -= (g == code - 1) ? (int)p.milli : 0;
  } else if (code == 9) {
    bool ok = false;
    const unsigned sm = sub_gpu_mask(gl, m.gpu_cnt(), cpuL, p, &ok);
    if (ok) {
      cpuL -= p.cpu_nz;
#pragma unroll
      for (int g = 0; g < kMaxGpu; ++g)
        if ((sm >> g) & 1u) gl[g] -= p.milli;
    }
  }
  return rp.typed ? frag_F<true>(cpuL, gl, 1u << m.gpu_type(), tp, rp.ncpu, rp.nt)
                  : frag_F<false>(cpuL, gl, 1u << m.gpu_type(), tp, rp.ncpu, rp.nt);
}

// Node score from its candidates' F values; *gpu = lowest GPU index reaching the max (share pods).
__device__ __forceinline__ void finalize_fgd(const double* F, const uint8_t* code, int o, int nc, bool share,
                                             int* raw, int* gpu) {
  const double F0 = F[o];
  *gpu = -1;
  if (share) {
    // candidates are in increasing first-index order: the first max is the lowest GPU index
    // reaching the max, as fgd_score.go:128 picks it
    int best = -1, bs = 0;
    for (int k = 1; k < nc; ++k) {
      const int fs = fgd_frag_score(F0, F[o + k]);
      if (best < 0 || fs > bs) { bs = fs; best = code[o + k] - 1; }
    }
    *raw = bs;
    *gpu = best;
  } else {
    *raw = fgd_frag_score(F0, F[o + 1]);
  }
}

// Winning total weighted score as the reference reports it (0 on the single-feasible shortcut).
__device__ __forceinline__ long long result_score(const ReplicaDev& rp, int nfeas, int wscore, int lo, int hi) {
  if (nfeas <= 1) return 0;
  if (rp.policy == POL_BESTFIT) return (hi > lo ? 100 : 0) * 1000LL;  // NormalizeScore (plugin_utils.go:48-74)
  if (rp.policy == POL_RANDOM) return 100 * 1000LL;
  if (rp.policy == POL_PWR_FGD) return (long long)wscore;  // already w_pwr * PWR + w_fgd * FGD
  // PWRScorePlugin.NormalizeScore maps the max raw score to 100 (and all-equal scores to 100), and
  // the winner holds the max raw score
  if (rp.policy == POL_PWR) return 100 * 1000LL;
  return (long long)wscore * 1000LL;
}


// The end of a scheduling cycle once the cluster-wide best key and counts are known: the result,
// Reserve's GPU selector and the Bind scatter (scheduler.go:509-554).  `node` is the local index
// of the winning node, or -1 when another shard owns it (sharded mode: the result then carries the
// winner's global rank and a provisional status; the owner's record is authoritative).
__device__ void finish_cycle(const StepArgs& a, const ReplicaDev& rp, const PodDev& p, int step, ResultDev* res_slot,
                             unsigned long long best, int nfeas, int anyerr, int glo, int ghi, int node) {
  ResultDev out{-1, 0, 0, nfeas, ST_UNSCHED};
  if (nfeas > 0) {
    out.status = (nfeas > 1 && anyerr) ? ST_ERROR : ST_OK;  // framework.go:650-656: a Score error aborts
    if (out.status == ST_OK) {
      out.score = result_score(rp, nfeas, key_score(best), glo, ghi);
      if (node < 0) {
        out.node = (int)key_rank(best);  // another shard binds
      } else {
        NodeRec* nr = rp.nodes + node;
        const NodeV wn = load_node(nr);
        const int mask = select_gpus(wn, p, rp.gpusel, sel_arg(rp, wn, p, node, key_gpu(best)), rp.seed, step);
        if (mask < 0) {
          out.status = ST_ERROR;  // Reserve failed: allocateGpuId returned "" / panicked
          out.score = 0;
        } else {
          apply_bind(nr, rp.tags + (size_t)node * kTagStride, p, mask, +1);
          if (rp.snap && !a.pod_override) note_change(rp, node, step);
          out.node = rp.node_off + node;
          out.gpu_mask = mask;
        }
      }
    }
  }
  *res_slot = out;
}

// PWR raw scores are energy deltas old - new <= 0 W (pwr_score.go:167,200); biased into the
// non-negative range of the Accum min / max.
constexpr int kPwrBias = 1 << 30;

__global__ __launch_bounds__(kBlock) void k_step(StepArgs a, const TypDev* __restrict__ tp_all) {
  const int r = a.rep_first + (int)blockIdx.x / a.bpr;
  const int b = (int)blockIdx.x % a.bpr;
  const int tid = (int)threadIdx.x;
  const ReplicaDev rp = a.reps[r];
  const TypDev* __restrict__ tp = tp_all + (size_t)r * kMaxTypical;
  const int step = (a.base ? *a.base : 0) + a.step_off;
  if (!a.pod_override && step >= rp.n_events) return;
  const PodDev p = a.pod_override ? *a.pod_override : rp.ev[step];
  ResultDev* res_slot = a.res_override ? a.res_override : (rp.res + step);

  if (p.flags & kPodDelete) {
    // simulator.go:416-422 deletePod -> informer DeleteFunc -> GpuSharePlugin.removePod
    if ((a.mode == 0 || a.mode == 2) && b == 0 && tid == 0) {
      ResultDev out{-1, 0, 0, 0, ST_DELETED};
      if (p.ref >= 0 && p.ref < step) {
        const ResultDev c = rp.res[p.ref];
        const int local = c.node - rp.node_off;  // sharded: only the owner of the node undoes the bind
        if (c.node >= 0 && c.status == ST_OK && local >= 0 && local < a.N) {
          const PodDev cp = rp.ev[p.ref];
          apply_bind(rp.nodes + local, rp.tags + (size_t)local * kTagStride, cp, c.gpu_mask, -1);
          if (rp.snap && !a.pod_override) note_change(rp, local, step);
        }
        if (c.node >= 0 && c.status == ST_OK) {
          out.node = c.node;
          out.gpu_mask = c.gpu_mask;
        }
      }
      *res_slot = out;
    }
    return;
  }

  __shared__ NodeRec s_node[kNBMax];
  __shared__ int s_off[kNBMax + 1];
  __shared__ uint8_t s_item_node[kNBMax * kMaxCand];
  __shared__ uint8_t s_item_code[kNBMax * kMaxCand];
  __shared__ double s_F[kNBMax * kMaxCand];
  __shared__ unsigned long long s_rkey[kBlock / 64];
  __shared__ int s_rcnt[kBlock / 64], s_rerr[kBlock / 64], s_rlo[kBlock / 64], s_rhi[kBlock / 64];

  const int n0 = b * a.NB;
  const int nb = max(0, min(a.NB, a.N - n0));
  const bool fgd = rp.policy == POL_FGD || rp.policy == POL_PWR_FGD;
  const bool pwr = is_pwr_policy(rp.policy);
  const bool share = is_share_pod(p);

  // ---- phase 1: Filter (+ cheap scores; PWR's raw score) ----
  bool feas = false, err = false;
  int raw = 0, nc = 0, gpu = -1, pgpu = -1;
  NodeV n{};
  if (tid < nb) {
    n = load_node(rp.nodes + n0 + tid);
    store_node(&s_node[tid], n);
    feas = node_phase1(n, p, rp, rp.tags + (size_t)(n0 + tid) * kTagStride, step, share, &raw, &nc, &err, n0 + tid,
                       &pgpu);
  }
  const int praw = raw;  // PWR policies: the PWR score before NormalizeScore

  // ---- phase 2: FGD candidate evaluation over a compacted work list ----
  if (fgd) {
    if (tid < 64) {  // wave 0: exclusive scan of candidate counts
      int v = tid < nb ? nc : 0;
      int incl = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        int w = __shfl_up(incl, o, 64);
        if (tid >= o) incl += w;
      }
      s_off[tid] = incl - v;
      if (tid == 63) s_off[64] = incl;
    }
    __syncthreads();
    if (tid < nb && nc > 0) emit_fgd_items(n, p, share, tid, s_off[tid], s_item_node, s_item_code);
    __syncthreads();
    const int items = s_off[64];
    for (int j = tid; j < items; j += kBlock)
      s_F[j] = eval_fgd_item(load_node(&s_node[s_item_node[j]]), s_item_code[j], p, rp, tp);
    __syncthreads();
    if (tid < nb && feas) finalize_fgd(s_F, s_item_code, s_off[tid], nc, share, &raw, &gpu);
  }

  if (a.mode == 1) {
    if (tid < nb) {
      a.out_feas[n0 + tid] = feas ? 1 : 0;
      a.out_score[n0 + tid] = feas ? (pwr ? praw : raw) : 0;
      a.out_gpu[n0 + tid] =
          feas ? select_gpus(n, p, rp.gpusel, (rp.gpusel == SEL_PWR || rp.gpusel == SEL_DOTPROD) ? pgpu : gpu, rp.seed, step)
               : 0;
    }
    return;
  }
  if (pwr && tid < nb) {
    // phase A of a PWR cycle: PWRScorePlugin.NormalizeScore needs the min / max raw score over the
    // feasible nodes first, so the per-node scores wait in HBM for k_step_pwr (same step, next launch)
    const int fgpu = rp.policy == POL_PWR_FGD ? gpu : -1;
    rp.pws[n0 + tid] = make_int2(feas ? praw : INT_MIN,
                                 (rp.policy == POL_PWR_FGD ? (raw & 0xff) : 0) | ((pgpu + 1) & 0xf) << 8 |
                                     ((fgpu + 1) & 0xf) << 12);
  }
  if (pwr) raw = praw + kPwrBias;  // the min / max accumulators start at -1 (raw PWR scores are <= 0)

  // ---- phase 3: workgroup reduction of the packed argmax key ----
  unsigned long long key = (feas && !pwr) ? pack_key((unsigned)raw, n.name_rank, gpu) : 0ull;
  int cnt = feas ? 1 : 0;
  int lo = feas ? raw : 0x7fffffff, hi = feas ? raw : -1;
  key = wave_max_u64(key);
  cnt = wave_sum_i(cnt);
  const int e = wave_max_i(err ? 1 : 0);
  lo = wave_min_i(lo);
  hi = wave_max_i(hi);
  const int w = tid >> 6;
  if ((tid & 63) == 0) { s_rkey[w] = key; s_rcnt[w] = cnt; s_rerr[w] = e; s_rlo[w] = lo; s_rhi[w] = hi; }
  __syncthreads();
  if (tid != 0) return;
  for (int i = 1; i < kBlock / 64; ++i) {
    key = s_rkey[i] > key ? s_rkey[i] : key;
    cnt += s_rcnt[i];
    lo = min(lo, s_rlo[i]);
    hi = max(hi, s_rhi[i]);
  }
  int errb = s_rerr[0] | s_rerr[1] | s_rerr[2] | s_rerr[3];

  // ---- commit: last workgroup of the replica finishes the cycle ----
  Accum* ac = a.acc + r;
  if (cnt > 0) {
    __hip_atomic_fetch_max(&ac->best, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&ac->nfeas, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(&ac->lo, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&ac->hi, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (errb) __hip_atomic_fetch_or(&ac->err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (pwr && a.mode != 2) return;  // k_step_pwr finishes the cycle
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every contribution performed before the ticket
  const unsigned t = __hip_atomic_fetch_add(&ac->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t != (unsigned)(a.bpr - 1)) return;
  if (pwr) {
    // round A of a sharded PWR cycle: the shard's raw score range goes to the exchange, so that k_step_pwr
    // normalizes with the cluster's.  The totals stay in the Accum for k_step_pwr (round B), which resets them.
    a.send[0] = 0ull;
    a.send[1] = (unsigned long long)__hip_atomic_load(&ac->nfeas, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.send[2] = (unsigned long long)__hip_atomic_load(&ac->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.send[3] = (unsigned long long)(unsigned)__hip_atomic_load(&ac->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
                ((unsigned long long)(unsigned)__hip_atomic_load(&ac->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 32);
    __hip_atomic_store(&ac->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }

  const unsigned long long best = __hip_atomic_exchange(&ac->best, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int nfeas = __hip_atomic_exchange(&ac->nfeas, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int anyerr = __hip_atomic_exchange(&ac->err, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int glo = __hip_atomic_exchange(&ac->lo, 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int ghi = __hip_atomic_exchange(&ac->hi, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&ac->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  if (a.mode == 2) {
    // node-sharded cluster: this shard's totals go to the exchange (k_shard_commit finishes)
    a.send[0] = best;
    a.send[1] = (unsigned long long)nfeas;
    a.send[2] = (unsigned long long)anyerr;
    a.send[3] = (unsigned long long)(unsigned)glo | ((unsigned long long)(unsigned)ghi << 32);
    return;
  }
  // the rank -> node index map lives right after the replica's tags (see host)
  const int* rank2idx = reinterpret_cast<const int*>(rp.tags + (size_t)a.N * kTagStride);
  finish_cycle(a, rp, p, step, res_slot, best, nfeas, anyerr, glo, ghi, best ? rank2idx[key_rank(best)] : -1);
}

// Phase B of a PWR / PWR+FGD cycle (after k_step's phase A of the same step): the normalized PWR
// score (pwr_score.go:104-141) with the replica's min / max raw score, the weighted sum with FGD
// (framework.go:686-704, generic_scheduler.go:511-519), the packed argmax key, and the last
// workgroup of the replica finishes the cycle as k_step does.
// kShard (a.mode == 2, node-sharded): the range is the cluster's, from the shards' round-A records in a.recv, and the
// last workgroup sends the shard's record instead of finishing the cycle; the unsharded form is what it was.
template <bool kShard>
__global__ __launch_bounds__(kBlock) void k_step_pwr(StepArgs a) {
  const int r = a.rep_first + (int)blockIdx.x / a.bpr;
  const int b = (int)blockIdx.x % a.bpr;
  const int tid = (int)threadIdx.x;
  const ReplicaDev rp = a.reps[r];
  if (!is_pwr_policy(rp.policy)) return;
  const int step = (a.base ? *a.base : 0) + a.step_off;
  if (!a.pod_override && step >= rp.n_events) return;
  const PodDev p = a.pod_override ? *a.pod_override : rp.ev[step];
  if (p.flags & kPodDelete) return;
  ResultDev* res_slot = a.res_override ? a.res_override : (rp.res + step);
  Accum* ac = a.acc + r;
  int lo, hi;
  if (kShard) {
    // node-sharded cluster: NormalizeScore's range is the cluster's, from the shards' round-A records
    // (the shards with feasible nodes, as k_shard_commit counts them)
    lo = 0x7fffffff, hi = -1;
    for (int k = 0; k < a.world; ++k) {
      const unsigned long long* r4 = a.recv + 4 * k;
      if ((int)r4[1] > 0) {
        lo = min(lo, (int)(unsigned)(r4[3] & 0xffffffffull));
        hi = max(hi, (int)(unsigned)(r4[3] >> 32));
      }
    }
  } else {
    lo = __hip_atomic_load(&ac->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hi = __hip_atomic_load(&ac->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __shared__ unsigned long long s_rkey[kBlock / 64];
  const int n0 = b * a.NB;
  const int nb = max(0, min(a.NB, a.N - n0));
  unsigned long long key = 0ull;
  if (tid < nb) {
    const int2 v = rp.pws[n0 + tid];
    if (v.x != INT_MIN) {
      const int norm = pwr_normalize(v.x + kPwrBias, lo, hi);
      const int pg = ((v.y >> 8) & 0xf) - 1, fg = ((v.y >> 12) & 0xf) - 1;
      const int total = rp.policy == POL_PWR_FGD ? rp.w_pwr * norm + rp.w_fgd * (v.y & 0xff) : norm;
      key = pack_key((unsigned)total, rp.nodes[n0 + tid].name_rank, rp.gpusel == SEL_PWR ? pg : fg);
    }
  }
  key = wave_max_u64(key);
  const int w = tid >> 6;
  if ((tid & 63) == 0) s_rkey[w] = key;
  __syncthreads();
  if (tid != 0) return;
  for (int i = 1; i < kBlock / 64; ++i) key = s_rkey[i] > key ? s_rkey[i] : key;
  if (key) __hip_atomic_fetch_max(&ac->best, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the contribution performed before the ticket
  const unsigned t = __hip_atomic_fetch_add(&ac->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t != (unsigned)(a.bpr - 1)) return;
  const unsigned long long best = __hip_atomic_exchange(&ac->best, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int nfeas = __hip_atomic_exchange(&ac->nfeas, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int anyerr = __hip_atomic_exchange(&ac->err, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int glo = __hip_atomic_exchange(&ac->lo, 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int ghi = __hip_atomic_exchange(&ac->hi, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&ac->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (kShard) {
    // round B of a sharded PWR cycle: the shard's best key under the cluster's range (k_shard_commit finishes)
    a.send[0] = best;
    a.send[1] = (unsigned long long)nfeas;
    a.send[2] = (unsigned long long)anyerr;
    a.send[3] = (unsigned long long)(unsigned)glo | ((unsigned long long)(unsigned)ghi << 32);
    return;
  }
  const int* rank2idx = reinterpret_cast<const int*>(rp.tags + (size_t)a.N * kTagStride);
  finish_cycle(a, rp, p, step, res_slot, best, nfeas, anyerr, glo, ghi, best ? rank2idx[key_rank(best)] : -1);
}

// Node-sharded cluster (ksim_engine_set_shard): one workgroup reduces the `world` shard records
// gathered by the exchange and finishes the cycle; only the shard owning the winning node binds.
// Node ranks are global and shard-contiguous (local node i has rank node_off + i).
__global__ __launch_bounds__(64) void k_shard_commit(StepArgs a) {
  const ReplicaDev rp = a.reps[0];
  const int step = (a.base ? *a.base : 0) + a.step_off;
  if (step >= rp.n_events || threadIdx.x != 0) return;
  const PodDev p = rp.ev[step];
  if (p.flags & kPodDelete) return;  // k_step applied it on the owner
  unsigned long long best = 0ull;
  int nfeas = 0, anyerr = 0, glo = 0x7fffffff, ghi = -1;
  for (int k = 0; k < a.world; ++k) {
    const unsigned long long* r4 = a.recv + 4 * k;
    best = r4[0] > best ? r4[0] : best;
    const int c = (int)r4[1];
    nfeas += c;
    anyerr |= (int)r4[2];
    if (c > 0) {
      glo = min(glo, (int)(unsigned)(r4[3] & 0xffffffffull));
      ghi = max(ghi, (int)(unsigned)(r4[3] >> 32));
    }
  }
  const int local = best ? (int)key_rank(best) - rp.node_off : -1;
  finish_cycle(a, rp, p, step, rp.res + step, best, nfeas, anyerr, glo, ghi, (local >= 0 && local < a.N) ? local : -1);
}

// In-process shard group: every shard's record to every shard's exchange buffer (one launch).
__global__ void k_shard_gather(unsigned long long* const* sends, unsigned long long* const* recvs, int world) {
  const int i = (int)threadIdx.x;  // world * world * 4 <= 1024
  if (i >= world * world * 4) return;
  const int dst = i / (world * 4), src = (i / 4) % world, f = i & 3;
  recvs[dst][4 * src + f] = sends[src][f];
}

#include "ksim_replay.hpp"
#include "ksim_report.hpp"
#include "ksim_memo.hpp"
#include "ksim_hmemo.hpp"

// ---------------------------------------------------------------------------
// k_replay: the whole event stream of every replica in one launch (see ksim_replay.hpp).
// Dynamic LDS: ReplayShared | NodeRec nodes[S+1] | u16 tags[S+1][16] | f64 F0[S+1] | f64 E0[S+1] |
// i32x2 pe[S+1] | i32 last[S+1] | i32 praw[S+1] | i32 pinf[S+1].
//
// PWR: NormalizeScore (pwr_score.go:104-141) sends exactly the nodes with the max raw score to 100,
// so the argmax of the normalized score is the argmax of the raw one: one key exchange per step, the
// raw score biased into the 24-bit key field.  PWR + FGD (the weighted sum, framework.go:686-704)
// needs the cluster's min / max raw PWR score before any node's total is known: an A round (min,
// max, feasible count, Score error) per step, then the normalized totals of the slice and the key
// round, which overlaps the next step's evaluation as for every other policy.
constexpr int kPfFeas = 1 << 30, kPfErr = 1 << 29;  // pinf flags (low 16 bits: FGD score, GPU choices)
constexpr int kPwrKeyBias = 1 << 23;                // raw PWR score -> 24-bit key field
// ---------------------------------------------------------------------------
__device__ __forceinline__ int lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Polled granules of the pending exchange, per wave-0 lane: workgroups lane + 64 j, j < kSub.
template <int kSub>
struct GranV {
  unsigned long long g0[kSub], g1[kSub], g2[kSub];
};

// kSub = ceil(K / 64): 1 for K <= 64, 4 for K <= 256 (one wave-0 lane polls kSub workgroups); 0 for
// K = 1 (no exchange), where the cheap policies are built for two 1024-thread workgroups per CU (64
// VGPRs: 8 waves per SIMD), so the paper sweep's single-workgroup replicas pack two to a CU.
// kGeneral: the KSIM_PROFILE timers, the cluster-report stores and delete events (bind history);
// the lean instantiation (none of them: the bench, the paper sweeps, C5) compiles them out of the
// step loop, as k_memo's does.
#include "ksim_random_go.hpp"
#include "ksim_scan1.hpp"
#include "ksim_wsum.hpp"
#include "ksim_desched.hpp"

template <int kPol, int kSub, bool kGeneral>
__global__ __launch_bounds__(ksim_replay::kRBlock, (kSub == 0 && kPol >= POL_BESTFIT && kPol <= POL_RANDOM &&
                                                     kPol != POL_DOTPROD) ? 8 : 1)
void k_replay(ksim_replay::ReplayArgs a,
                                                                 const TypDev* __restrict__ tp_all) {
  using namespace ksim_replay;
  constexpr int kS = kSub > 0 ? kSub : 1;  // granule columns per polling lane (K = 1 polls none)
  constexpr bool kPwr = kPol == POL_PWR;
  constexpr bool kPF = kPol == POL_PWR_FGD;
  constexpr bool kFgd = kPol == POL_FGD || kPF;  // the FGD candidate evaluation
  constexpr bool kMinMax = kPol == POL_BESTFIT;  // NormalizeScore needs the raw min / max
  constexpr bool kErr = kPol == POL_BESTFIT || kPol == POL_DOTPROD || kPol == POL_PACKING || kPol == POL_CLUSTERING || kPwr || kPF;
  // all LDS is dynamic (no static __shared__ in front of it), carved 16-byte aligned
  extern __shared__ __attribute__((aligned(16))) char smem[];
  ReplayShared& sh = *reinterpret_cast<ReplayShared*>(smem);
  const int r = a.rep_list[(int)blockIdx.x / a.K];
  const int w = (int)blockIdx.x % a.K;
  // the exchange: Kx columns (every workgroup of the replica; a node-sharded group, a.xK: every workgroup of
  // every shard), this workgroup's column wx
  const int Kx = a.xK > 0 ? a.xK : a.K;
  const int wx = (int)blockIdx.x % Kx;
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const ReplicaDev rp = a.reps[r];
  const TypDev* __restrict__ tp = tp_all + (size_t)r * kMaxTypical;
  const int n_lo = w * a.S;
  const int ns = max(0, min(a.S, (a.group ? rp.n_local : a.N) - n_lo));
  constexpr bool kTags = kPol == POL_CLUSTERING;  // GpuClustering reads the tag counts per pod step
  const RLayout L = replay_layout(a.S, kPol, kGeneral, kPF ? a.pm_c : 0);
  ReplayFgd& fs = *reinterpret_cast<ReplayFgd*>(smem + L.fgd);  // FGD launches only
  NodeRec* s_nodes = reinterpret_cast<NodeRec*>(smem + L.nodes);
  uint16_t* s_tags = reinterpret_cast<uint16_t*>(smem + L.tags);  // kTags only
  // the other policies keep the slice's tag counts in HBM (changed by a Bind / delete, read by none)
  uint16_t* g_tags = rp.tags + (size_t)n_lo * kTagStride;
  double* s_F0 = reinterpret_cast<double*>(smem + L.F0);
  // PWR policies: the cached energy of each slot's current state (kEnergyStale: recompute) and the
  // node's static energy terms {rc, ncpus << 3 | CPU model} (energy_static)
  double* s_E0 = reinterpret_cast<double*>(smem + L.E0);
  int2* s_pe = reinterpret_cast<int2*>(smem + L.pe);
  // cluster report: the last event that changed each slot (-1: none yet)
  int* s_last = reinterpret_cast<int*>(smem + L.last);
  int* s_praw = reinterpret_cast<int*>(smem + L.praw);  // PWR+FGD per-slot scratch of the current step
  int* s_pinf = reinterpret_cast<int*>(smem + L.pinf);
  // PWR+FGD: each class's two most recent cluster-wide raw PWR ranges {lo0, hi0, lo1, hi1} (most recent first;
  // classes alias mod kPfGuess -- a guess only ever saves a round, the decision checks it)
  int4* s_gtab = reinterpret_cast<int4*>(smem + L.gtab);
  // PWR+FGD memo (a.pm_c > 0): every class's Filter + Score of every real slot, kept while the slot's
  // record is unchanged (s_pver), so a step evaluates only the slots changed since its class last came
  // and the virtual slot
  const bool pmon = kPF && a.pm_c > 0;
  unsigned* s_pver = reinterpret_cast<unsigned*>(smem + L.pver);
  uint2* s_pm = reinterpret_cast<uint2*>(smem + L.pm);
  auto pm_bump = [&](int i) {  // (one lane) slot i's record changed: its entries are stale
    unsigned v = s_pver[i] + 1u;
    if (v == kPmInvalid) {  // the version field wraps: forget the slot's entries first
      v = 0u;
      for (int c = 0; c < a.pm_c; ++c) s_pm[(size_t)c * a.S + i].y = kPmInvalid << 18;
    }
    s_pver[i] = v;
  };
  // hist[step]: (node, mask+1) bound here | (-1,0) no winner | (-2,0) winner elsewhere | (-3,0) Reserve failed here
  // (null when no replica of the launch has a delete event: nothing ever reads it)
  int2* hist = (kGeneral && a.hist) ? a.hist + (size_t)(r * a.K + w) * a.hist_stride : nullptr;
  NodeRec* const snap = kGeneral ? rp.snap : nullptr;
  unsigned long long* gr = a.gran + (size_t)(blockIdx.x / Kx) * 2 * Kx * kGranW;

  for (int i = tid; i < ns; i += kRBlock) store_node(&s_nodes[i], load_node(rp.nodes + n_lo + i));
  if (kTags)
    for (int i = tid; i < ns * kTagStride; i += kRBlock) s_tags[i] = rp.tags[(size_t)n_lo * kTagStride + i];
  if (kGeneral)
    for (int i = tid; i <= ns; i += kRBlock) s_last[i] = -1;
  if (kPwr || kPF) {
    for (int i = tid; i < (int)(sizeof(PowerDev) / 8); i += kRBlock)
      reinterpret_cast<unsigned long long*>(&sh.pw)[i] = reinterpret_cast<const unsigned long long*>(rp.pw)[i];
    for (int i = tid; i < ns; i += kRBlock) s_pe[i] = energy_static(rp.cap[n_lo + i], rp.cpum[n_lo + i], *rp.pw);
    for (int i = tid; i <= ns; i += kRBlock) s_E0[i] = kEnergyStale;
  }
  if (kPF)
    for (int i = tid; i < kPfGuess; i += kRBlock) s_gtab[i] = make_int4(1, 0, 1, 0);  // lo > hi: never a range
  if (pmon) {
    for (int i = tid; i <= ns; i += kRBlock) s_pver[i] = a.pm_ver0;
    for (int i = tid; i < a.pm_c * a.S; i += kRBlock) s_pm[i] = make_uint2(0u, kPmInvalid << 18);
  }
  if (kFgd) {
    for (int i = tid; i <= ns; i += kRBlock) s_F0[i] = -1.0;  // every cached F stale
    for (int i = tid; i < rp.nt * 2; i += kRBlock)
      reinterpret_cast<uint4*>(fs.tp)[i] = reinterpret_cast<const uint4*>(tp)[i];
  }
  auto reset_agg = [&]() {
    sh.agg_key = 0ull;
    sh.agg_key1 = 0ull;
    sh.agg_cnt = 0;
    sh.agg_err = 0;
    sh.agg_lo = 0x7fffffff;
    sh.agg_hi = kPF ? INT_MIN : -1;
  };
  if (tid == 0) { sh.stop = 0; sh.nitems = 0; sh.pend_valid = 0; sh.pend_b = -1; reset_agg(); }
  for (int i = tid; i < 32; i += kRBlock) sh.dead[i] = 0u;

  // wave 0's copy of the pending exchange (the previous pod step, published, not committed)
  int p_step = 0, p_seq = 0, p_b = -1, p_mask = -1, seq = 0, p_cls = 0;
  int p_tag = -1;  // the pending Bind's affinity tag (policies keeping the tag counts in HBM)
  unsigned long long p_key = 0ull;
  int p_st0 = 0, p_st1 = 0, p_st2 = 0, p_st3 = 0;  // K == 1: the step's own totals

  // phase timer (wall clock, 100 MHz): only with a profile buffer, thread 0 of each workgroup
  const bool prof = kGeneral && a.prof != nullptr;
  if (prof && tid < kProfPhases) sh.prof[tid] = 0ull;
  unsigned long long t_last = prof ? __builtin_amdgcn_s_memrealtime() : 0ull;
  const unsigned long long t_start = t_last, c_start = prof ? __builtin_amdgcn_s_memtime() : 0ull;
  auto mark = [&](int ph) {
    if (prof && tid == 0) {
      const unsigned long long t = __builtin_amdgcn_s_memrealtime();
      sh.prof[ph] += t - t_last;
      t_last = t;
    }
  };

  // Wave 0, lane k: the granules of workgroups k, k+64, .. (< K) of the pending exchange
  // (relaxed agent-scope loads).
  auto poll_once = [&](GranV<kS>& g) {
    const unsigned long long* slot = gr + (size_t)(p_seq & 1) * Kx * kGranW;
#pragma unroll
    for (int j = 0; j < kS; ++j) {
      const int k = lane + 64 * j;
      if (k < Kx) {
        g.g0[j] = gload(slot + (size_t)k * kGranW + 0);
        g.g1[j] = gload(slot + (size_t)k * kGranW + 1);
        g.g2[j] = gload(slot + (size_t)k * kGranW + 2);
      }
    }
  };
  // Wave 0, PWR+FGD: ONE round per pod step.  NormalizeScore needs the cluster-wide min / max raw PWR score
  // before any node's weighted total exists; instead of a round for it and then a key round, every slice
  // publishes its A totals (min, max, feasible count | Score error: words 4-6) together with its best key under
  // each of the two ranges last seen for the pod's class (words 0-1, 2-3).  When the true range is one of them
  // (or at most one node is feasible: no normalisation), that key column decides; else every slice re-keys
  // the step under the true range from its scratch (kept two steps) and a miss round (words 7-8) decides.
  // The round overlaps the next pod's evaluation like every policy's key round.
  // (x: an earlier poll when `have`, issued before the evaluation's last barrier so its latency overlaps the wait)
  auto pf_collect = [&](unsigned long long (&x)[kS][7], bool have, int* gc, int* ge, int* gl, int* gh,
                        unsigned long long* W0, unsigned long long* W1) -> bool {
    const unsigned long long* slot = gr + (size_t)(p_seq & 1) * Kx * kGranW;
    const unsigned long long tag = (unsigned long long)(unsigned)(p_seq + 1) << 32;
    auto load = [&]() {
#pragma unroll
      for (int j = 0; j < kS; ++j) {
        const int k = lane + 64 * j;
        if (k < Kx) {
#pragma unroll
          for (int q = 0; q < 7; ++q) x[j][q] = gload(slot + (size_t)k * kGranW + q);
        }
      }
    };
    auto ready = [&]() {
      bool r = true;
#pragma unroll
      for (int j = 0; j < kS; ++j) {
        bool t = true;
#pragma unroll
        for (int q = 0; q < 7; ++q) t = t && (x[j][q] & ~0xffffffffull) == tag;
        r = r && (lane + 64 * j >= Kx || t);
      }
      return r;
    };
    if (!have) load();
    unsigned spins = 0;
    bool ok = true;
    while (!__all(ready())) {
      if (++spins > kSpinLimit) { ok = false; break; }
      __builtin_amdgcn_s_sleep(1);
      load();
    }
    if (prof && lane == 0) sh.prof[8] += spins;
    int cs = 0, lo = INT_MAX, hi = INT_MIN, e1 = 0;
    unsigned long long b0 = 0ull, b1 = 0ull;
#pragma unroll
    for (int j = 0; j < kS; ++j) {
      if (lane + 64 * j < Kx) {
        const unsigned long long k0 = ((x[j][1] & 0xffffffffull) << 32) | (x[j][0] & 0xffffffffull);
        const unsigned long long k1 = ((x[j][3] & 0xffffffffull) << 32) | (x[j][2] & 0xffffffffull);
        const unsigned st = (unsigned)x[j][6];
        const int c = (int)(st & 0x7fffffffu);
        cs += c;
        e1 |= (int)(st >> 31);
        if (c > 0) {
          lo = min(lo, (int)(unsigned)x[j][4]);
          hi = max(hi, (int)(unsigned)x[j][5]);
        }
        b0 = k0 > b0 ? k0 : b0;
        b1 = k1 > b1 ? k1 : b1;
      }
    }
    *gc = wave_sum_dpp(cs);
    *ge = __any(e1 != 0) ? 1 : 0;
    *gl = wave_min_dpp(lo);
    *gh = wave_max_dpp(hi);
    *W0 = wave_max_u64_dpp(b0);
    *W1 = wave_max_u64_dpp(b1);
    return ok;
  };
  auto pf_miss_round = [&](unsigned long long mine, unsigned long long* W) -> bool {
    unsigned long long* slot = gr + (size_t)(p_seq & 1) * Kx * kGranW;
    const unsigned long long tag = (unsigned long long)(unsigned)(p_seq + 1) << 32;
    if (lane == 0) {
      gstore(slot + (size_t)wx * kGranW + 7, tag | (mine & 0xffffffffull));
      gstore(slot + (size_t)wx * kGranW + 8, tag | (mine >> 32));
    }
    unsigned long long x0[kS], x1[kS];
    auto load = [&]() {
#pragma unroll
      for (int j = 0; j < kS; ++j) {
        const int k = lane + 64 * j;
        if (k < Kx) {
          x0[j] = gload(slot + (size_t)k * kGranW + 7);
          x1[j] = gload(slot + (size_t)k * kGranW + 8);
        }
      }
    };
    auto ready = [&]() {
      bool r = true;
#pragma unroll
      for (int j = 0; j < kS; ++j)
        r = r && (lane + 64 * j >= Kx || ((x0[j] & ~0xffffffffull) == tag && (x1[j] & ~0xffffffffull) == tag));
      return r;
    };
    load();
    unsigned spins = 0;
    bool ok = true;
    while (!__all(ready())) {
      if (++spins > kSpinLimit) { ok = false; break; }
      __builtin_amdgcn_s_sleep(1);
      load();
    }
    unsigned long long b = 0ull;
#pragma unroll
    for (int j = 0; j < kS; ++j)
      if (lane + 64 * j < Kx) {
        const unsigned long long k = ((x1[j] & 0xffffffffull) << 32) | (x0[j] & 0xffffffffull);
        b = k > b ? k : b;
      }
    *W = wave_max_u64_dpp(b);
    return ok;
  };
  // Wave 0: the pending step's exchange result -- every workgroup's granules (K > 1) or
  // this workgroup's own totals (K == 1); g holds an earlier poll.  Returns the winning key.
  auto exchange = [&](GranV<kS>& g, int* gc, int* ge, int* gl, int* gh, bool* ok) -> unsigned long long {
    *ok = true;
    if (Kx == 1) {
      *gc = p_st0; *ge = p_st1; *gl = p_st2; *gh = p_st3;
      return p_key;
    }
    const unsigned long long tag = (unsigned long long)(unsigned)(p_seq + 1) << 32;
    auto ready = [&]() {
      bool r = true;
#pragma unroll
      for (int j = 0; j < kS; ++j)
        r = r && (lane + 64 * j >= Kx || ((g.g0[j] & ~0xffffffffull) == tag && (g.g1[j] & ~0xffffffffull) == tag &&
                                          (g.g2[j] & ~0xffffffffull) == tag));
      return r;
    };
    unsigned spins = 0;
    while (!__all(ready())) {
      if (++spins > kSpinLimit) { *ok = false; break; }
      __builtin_amdgcn_s_sleep(1);
      poll_once(g);
    }
    if (prof && lane == 0) sh.prof[8] += spins;
    int c = 0, lo = 0x7fffffff, hi = -1;
    bool e1 = false;
    unsigned long long best = 0ull;
#pragma unroll
    for (int j = 0; j < kS; ++j) {
      const bool in = lane + 64 * j < Kx;
      const unsigned st = in ? (unsigned)(g.g2[j] & 0xffffffffull) : 0u;
      const int cj = (int)(st & 0x1ffff);
      c += cj;
      e1 = e1 || (st >> 31) != 0u;
      const unsigned long long kj = in ? ((g.g1[j] & 0xffffffffull) << 32) | (g.g0[j] & 0xffffffffull) : 0ull;
      if (kMinMax && cj > 0) {
        // BestFit: a slice's max raw score is its key's score field; its bit 17 says whether its scores differ.
        // NormalizeScore needs only whether any two feasible scores differ (result_score: hi > lo).
        const int sj = key_score(kj);
        lo = min(lo, sj - (int)((st >> 17) & 1u));
        hi = max(hi, sj);
      }
      best = kj > best ? kj : best;
    }
    *gc = wave_sum_dpp(c);
    *ge = __any(e1) ? 1 : 0;
    *gl = 0x7fffffff;
    *gh = -1;
    if (kMinMax) {
      *gl = wave_min_dpp(lo);
      *gh = wave_max_dpp(hi);
    }
    return wave_max_u64_dpp(best);
  };

  // Wave 0: commit the pending step -- the owner of the winning node turns the virtual slot
  // into that node (Reserve + Bind were applied to it when it was prepared).  Lanes 0-6 copy.
  auto commit = [&](unsigned long long W, int nfeas, int gerr, int glo, int ghi) {
    const bool owner = W != 0ull && W == p_key;
    // nothing feasible anywhere: the pending event's class stays infeasible (create-only streams)
    if (a.skip && nfeas == 0 && lane == 0) sh.dead[p_cls >> 5] |= 1u << (p_cls & 31);
    ResultDev out{-1, 0, 0, nfeas, ST_UNSCHED};
    int2 hrec = make_int2(-1, 0);
    bool writer = w == 0;
    if (nfeas > 0) {
      out.status = (nfeas > 1 && gerr) ? ST_ERROR : ST_OK;
      if (out.status == ST_OK) {
        out.score = result_score(rp, nfeas, key_score(W), glo, ghi);
        writer = owner;  // the owner of the winning node reports
        hrec.x = -2;
        if (owner) {
          if (p_mask < 0) {  // Reserve failed: allocateGpuId returned "" / panicked
            out.status = ST_ERROR;
            out.score = 0;
            hrec.x = -3;
          } else {
            if (lane < 2) reinterpret_cast<uint4*>(&s_nodes[p_b])[lane] = reinterpret_cast<const uint4*>(&s_nodes[ns])[lane];
            else if (lane < 6 && kTags)
              reinterpret_cast<uint2*>(&s_tags[(size_t)p_b * kTagStride])[lane - 2] =
                  reinterpret_cast<const uint2*>(&s_tags[(size_t)ns * kTagStride])[lane - 2];
            else if (lane == 2 && !kTags && p_tag >= 0) tag_add(g_tags + (size_t)p_b * kTagStride, p_tag, +1);
            else if (lane == 6 && kFgd) s_F0[p_b] = s_F0[ns];
            else if (lane == 8 && kPF) { s_praw[p_b] = s_praw[ns]; s_pinf[p_b] = s_pinf[ns]; }
            else if (lane == 10 && pmon) pm_bump(p_b);
            else if (lane == 9 && (kPwr || kPF)) s_E0[p_b] = s_E0[ns];
            else if (lane == 7 && snap) {  // cluster report: the post-Bind record (the virtual slot)
              store_node(snap + p_step, load_node(&s_nodes[ns]));
              rp.prev[p_step] = s_last[p_b];
              s_last[p_b] = p_step;
            }
            out.node = a.group ? (int)key_rank(W) : n_lo + p_b;
            out.gpu_mask = p_mask;
            hrec = make_int2(n_lo + p_b, p_mask + 1);
          }
        }
      }
    }
    if (lane == 0) {
      if (hist) hist[p_step] = hrec;
      if (writer) {
        rp.res[p_step] = out;
      } else if (a.group && w == 0) {  // a shard that does not own the winner names it (the owner's record rules)
        // (the owner's shard -- its ranks are [node_off, node_off + n_local) -- has its owning workgroup write)
        const uint32_t rk = key_rank(W);
        if (rk - (uint32_t)rp.node_off >= (uint32_t)rp.n_local) {
          out.node = (int)rk;
          rp.res[p_step] = out;
        }
      }
    }
  };

  // PWR+FGD: a feasible slot's packed key under the range [lo, hi]: w_pwr * NormalizeScore(PWR) + w_fgd * FGD
  // (framework.go:686-704; unsigned arithmetic: a guessed range that is not the step's may give any value, and
  // is then never used)
  auto pf_key = [&](int praw, int inf, int lo, int hi, int i) -> unsigned long long {
    // pwr_normalize in 32 bits: on the step's true range 0 <= praw - lo <= hi - lo < 2^24, so (praw - lo) * 100 < 2^31
    const unsigned norm = lo == hi ? 100u : (unsigned)(praw - lo) * 100u / (unsigned)(hi - lo);
    const unsigned total = (unsigned)rp.w_pwr * norm + (unsigned)rp.w_fgd * (unsigned)(inf & 0xff);
    const int kg = rp.gpusel == SEL_PWR ? ((inf >> 8) & 0xf) - 1 : ((inf >> 12) & 0xf) - 1;
    return pack_key(total, load_node(&s_nodes[i]).name_rank, kg, i);
  };
  // Wave 0: the pending step's best key of this slice under the true range, from its scratch
  auto pf_rekey = [&](int lo, int hi) -> unsigned long long {
    const int* q_praw = s_praw + (p_step & 1) * (a.S + 1);
    const int* q_pinf = s_pinf + (p_step & 1) * (a.S + 1);
    unsigned long long b = 0ull;
    for (int i = lane; i < ns; i += 64) {
      const int inf = q_pinf[i];
      if (inf & kPfFeas) {
        const unsigned long long k = pf_key(q_praw[i], inf, lo, hi, i);
        b = k > b ? k : b;
      }
    }
    return wave_max_u64_dpp(b);
  };
  // Wave 0: decide and commit the pending step.  The owner of the winner applies the virtual node when the winner
  // is the node it prepared (guess 0's local best), else Reserve + Bind on the winner's slot itself; `overlapped`:
  // this step's evaluation already ran, and *redo asks for it again (one of its slots changed under it).
  auto pf_resolve = [&](unsigned long long (&x)[kS][7], bool have, bool overlapped, bool* redo) -> bool {
    *redo = false;
    int gc = p_st0, ge = p_st1, gl = p_st2, gh = p_st3;
    const unsigned long long p_key1 = sh.pf_key1;
    const int4 p_g = sh.pf_g;
    unsigned long long W0 = p_key, W1 = p_key1;
    if (Kx > 1 && !pf_collect(x, have, &gc, &ge, &gl, &gh, &W0, &W1)) return false;
    const bool m0 = gc <= 1 || (gl == p_g.x && gh == p_g.y);  // at most one feasible node: no normalisation
    const bool m1 = !m0 && gl == p_g.z && gh == p_g.w;
    unsigned long long W = m0 ? W0 : W1, mine = m0 ? p_key : p_key1;
    if (!m0 && !m1 && !ge) {  // (a Score error aborts the cycle: no winner needed)
      if (prof && lane == 0) sh.prof[9] += 1ull;  // KSIM_PROFILE: misses (low half), re-evaluations (high)
      mine = pf_rekey(gl, gh);
      W = mine;
      if (Kx > 1 && !pf_miss_round(mine, &W)) return false;
    }
    if (gc > 1 && lane == 0 && a.pf_guess) {  // the class's most recent ranges (every workgroup updates alike)
      int4& t = s_gtab[p_cls & (kPfGuess - 1)];
      if (!(t.x == gl && t.y == gh)) t = make_int4(gl, gh, t.x, t.y);
    }
    // commit
    const bool owner = W != 0ull && W == mine;
    if (a.skip && gc == 0 && lane == 0) sh.dead[p_cls >> 5] |= 1u << (p_cls & 31);
    ResultDev out{-1, 0, 0, gc, ST_UNSCHED};
    int2 hrec = make_int2(-1, 0);
    bool writer = w == 0;
    if (gc > 0) {
      out.status = (gc > 1 && ge) ? ST_ERROR : ST_OK;  // framework.go:650-656: a Score error aborts
      if (out.status == ST_OK) {
        out.score = result_score(rp, gc, key_score(W), gl, gh);
        writer = owner;
        hrec.x = -2;
        if (owner) {
          const int x = key_loc(W);
          int mask = p_mask;
          const bool virt = x == p_b;
          NodeV bn{};
          const PodDev p_pod = sh.pf_pod;
          if (!virt) {  // Reserve + Bind on the winner's slot (the virtual node holds another)
            bn = load_node(&s_nodes[x]);
            mask = select_gpus(bn, p_pod, rp.gpusel, sel_arg<false>(rp, bn, p_pod, n_lo + x, key_gpu(W)), rp.seed, p_step);
            if (mask >= 0) bind_node(bn, p_pod, mask, +1);
          }
          if (mask < 0) {  // Reserve failed: allocateGpuId returned "" / panicked
            out.status = ST_ERROR;
            out.score = 0;
            hrec.x = -3;
          } else {
            const int tg = (int)p_pod.tag;
            if (virt) {
              if (lane < 2) reinterpret_cast<uint4*>(&s_nodes[x])[lane] = reinterpret_cast<const uint4*>(&s_nodes[ns])[lane];
              else if (lane == 6) s_F0[x] = s_F0[ns];
              else if (lane == 9) s_E0[x] = s_E0[ns];
              else if (lane == 8 && overlapped) {  // this step's scratch: the post-Bind node (the virtual slot's)
                int* c_pr = s_praw + ((p_step + 1) & 1) * (a.S + 1);
                int* c_pi = s_pinf + ((p_step + 1) & 1) * (a.S + 1);
                c_pr[x] = c_pr[ns];
                c_pi[x] = c_pi[ns];
              }
            } else {
              if (lane == 0) store_node(&s_nodes[x], bn);
              else if (lane == 6) s_F0[x] = -1.0;
              else if (lane == 9) s_E0[x] = kEnergyStale;
              *redo = overlapped;
              if (prof && lane == 0 && overlapped) sh.prof[9] += 1ull << 32;
            }
            if (lane == 2 && tg >= 0) tag_add(g_tags + (size_t)x * kTagStride, tg, +1);
            else if (lane == 10 && pmon) pm_bump(x);
            else if (lane == 7 && snap) {  // cluster report: the post-Bind record
              store_node(snap + p_step, virt ? load_node(&s_nodes[ns]) : bn);
              rp.prev[p_step] = s_last[x];
              s_last[x] = p_step;
            }
            out.node = a.group ? (int)key_rank(W) : n_lo + x;
            out.gpu_mask = mask;
            hrec = make_int2(n_lo + x, mask + 1);
          }
        }
      }
    }
    if (lane == 0) {
      if (hist) hist[p_step] = hrec;
      if (writer) {
        rp.res[p_step] = out;
      } else if (a.group && w == 0) {  // a shard that does not own the winner names it, as in commit()
        const uint32_t rk = key_rank(W);
        if (rk - (uint32_t)rp.node_off >= (uint32_t)rp.n_local) {
          out.node = (int)rk;
          rp.res[p_step] = out;
        }
      }
    }
    return true;
  };

  // Finish the pending step with nothing to overlap (before a delete / at the end).
  auto finish_pending = [&]() {
    if (wv == 0) {
      bool ok = true;
      if constexpr (kPF) {
        bool redo;
        unsigned long long x[kS][7];
        ok = pf_resolve(x, false, false, &redo);
      } else {
        GranV<kS> g{};
        if (Kx > 1) poll_once(g);
        int gc, ge, gl, gh;
        const unsigned long long W = exchange(g, &gc, &ge, &gl, &gh, &ok);
        if (ok) commit(W, gc, ge, gl, gh);
      }
      if (lane == 0) {
        if (!ok) { sh.stop = 1; atomicOr(a.fail, 1); }
        sh.pend_valid = 0;
        sh.pend_b = -1;
      }
    }
    __syncthreads();
  };

  __syncthreads();
  for (int step = 0; step < rp.n_events; ++step) {
    const int eb = step & (kEvBuf - 1);
    if (eb == 0) {
      // refill the LDS event window (every thread passed the previous step's final barrier)
      const int nl = min(kEvBuf, rp.n_events - step) * 2;
      const uint4* src = reinterpret_cast<const uint4*>(rp.ev + step);
      for (int i = tid; i < nl; i += kRBlock) reinterpret_cast<uint4*>(sh.ev)[i] = src[i];
      __syncthreads();
    }
    const PodDev p = uniform_pod(&sh.ev[eb]);
    const int2 pvb = *reinterpret_cast<const int2*>(&sh.pend_valid);
    const bool pend = __builtin_amdgcn_readfirstlane(pvb.x) != 0;
    // Dead-class skip (create-only streams): Filter is monotone in the resources a creation takes, so an
    // event whose class found no feasible node before finds none now -- unscheduled, 0 feasible, nothing
    // changes.  The pending step is finished first (its commit may add to the dead set); every workgroup
    // marks the same classes at the same commit, so all skip the same steps.
    if (a.skip && ((sh.dead[p.pad >> 5] >> (p.pad & 31)) & 1u)) {
      if (pend) finish_pending();
      if (sh.stop) break;
      if (tid == 0 && w == 0) rp.res[step] = ResultDev{-1, 0, 0, 0, ST_UNSCHED};
      __syncthreads();
      continue;
    }
    if (kGeneral && (p.flags & kPodDelete)) {  // lean: launched on create-only streams
      if (pend) finish_pending();
      if (sh.stop) break;
      // removePod on the owner of the creation (every workgroup recorded its view of it)
      if (tid == 0) {
        const int2 h = (p.ref >= 0 && p.ref < step) ? hist[p.ref] : make_int2(-1, 0);
        if (h.x >= 0) {
          PodDev cp = rp.ev[p.ref];
          const int loc = h.x - n_lo;
          if (!kTags && cp.tag >= 0) {  // the HBM counts: an atomic, not a read-modify-write
            tag_add(g_tags + (size_t)loc * kTagStride, cp.tag, -1);
            cp.tag = -1;
          }
          apply_bind(&s_nodes[loc], kTags ? &s_tags[(size_t)loc * kTagStride] : nullptr, cp, h.y - 1, -1);
          if (kFgd) s_F0[loc] = -1.0;
          if (kPwr || kPF) s_E0[loc] = kEnergyStale;
          if (pmon) pm_bump(loc);
          if (snap) {
            store_node(snap + step, load_node(&s_nodes[loc]));
            rp.prev[step] = s_last[loc];
            s_last[loc] = step;
          }
          rp.res[step] = ResultDev{h.x, h.y - 1, 0, 0, ST_DELETED};
        } else if ((h.x == -1 && w == 0) || h.x == -3) {
          rp.res[step] = ResultDev{-1, 0, 0, 0, ST_DELETED};
        }
        if (hist) hist[step] = make_int2(-1, 0);
      }
      __syncthreads();
      mark(0);
      continue;
    }
    mark(0);
    // ---- Filter + Score of the slice, the pending best node b excluded, plus the virtual node
    const bool share = is_share_pod(p);
    const int vb = pend ? __builtin_amdgcn_readfirstlane(pvb.y) : -1;
    const int nsv = ns + (vb >= 0 ? 1 : 0);
    // PWR+FGD: this step's per-slot scratch (by step parity: the pending step's stays intact for a miss round)
    int* const c_praw = s_praw + (step & 1) * (a.S + 1);
    int* const c_pinf = s_pinf + (step & 1) * (a.S + 1);
    unsigned long long px[kS][7];  // PWR+FGD: wave 0's early poll of the pending round
    // early poll of the pending exchange by wave 0 (consumed after the evaluation)
    GranV<kS> pg{};
    // one node's packed key into the workgroup aggregate (LDS atomics), or the excluded pair
    auto route = [&](bool leader, int i, bool feas, bool e1, int raw, unsigned long long k) {
      const bool excl = leader && (i == vb || i == ns);
      if (excl) {
        // the pending best node as it is / as it would be after the pending Bind
        if (i == ns) { sh.post_key = k; sh.post_feas = feas ? 1 : 0; sh.post_err = (feas && e1) ? 1 : 0; }
        else { sh.pre_key = k; sh.pre_feas = feas ? 1 : 0; sh.pre_err = (feas && e1) ? 1 : 0; }
      }
      const bool agg = leader && feas && !excl;
      const unsigned long long am = __ballot(agg);
      if (am) {
        if (agg) {
          atomicMax(&sh.agg_key, k);
          if (kMinMax) { atomicMin(&sh.agg_lo, raw); atomicMax(&sh.agg_hi, raw); }
        }
        if (lane == 0) atomicAdd(&sh.agg_cnt, (int)__popcll(am));
        if (kErr) {
          if (__any(agg && e1) && lane == 0) atomicOr(&sh.agg_err, 1);
        }
      }
    };
    if constexpr (kFgd) {
      for (int c0 = 0; c0 < nsv; c0 += kFChunk) {
        const int cn = min(kFChunk, nsv - c0);
        const int i = c0 + (tid >> 3), g = tid & 7;
        const bool valid = (tid >> 3) < cn;
        NodeV n{};
        bool feas = false;
        // PWR+FGD memo: a real slot unchanged since this class last came reuses its entry
        bool hit = false;
        uint2 me = make_uint2(0u, 0u);
        if (pmon && valid && i < ns) {
          me = s_pm[(size_t)p.pad * a.S + i];
          hit = pf_memo_hit(me, s_pver[i]);
        }
        if (valid && !hit) {
          n = load_node(&s_nodes[i]);
          feas = filter_node(n, p);
        }
        // lane g's candidate: share pod -> GPU g if it fits and no lower GPU has the same milli
        // left (equal values give the same GPU multiset, hence the same F); else the Sub state
        bool cand = false;
        if (feas) {
          if (share) {
            const int v = gl_dyn(n, g);
            cand = g < n.gpu_cnt() && v >= p.milli && (gl_equal_mask(n, v) & ((1u << g) - 1u)) == 0u;
          } else {
            cand = g == 0;
          }
        }
        const bool cur = feas && g == 0 && s_F0[i] < 0.0;  // cached F of the current state stale
        const unsigned long long cm = __ballot(cand), um = __ballot(cur);
        const int nw = __popcll(cm) + __popcll(um);
        int base = 0;
        if (nw > 0) {
          if (lane == 0) base = atomicAdd(&sh.nitems, nw);
          base = __builtin_amdgcn_readfirstlane(base);
        }
        int my_item = -1;
        if (cand) {
          my_item = base + lanes_below(cm);
          fs.item_node[my_item] = (uint16_t)i;
          fs.item_code[my_item] = (uint8_t)(share ? 1 + g : 9);
        }
        if (cur) {
          const int o = base + __popcll(cm) + lanes_below(um);
          fs.item_node[o] = (uint16_t)i;
          fs.item_code[o] = 0;
        }
        __syncthreads();
        mark(1);
        const int tot = sh.nitems;
        const int q = tid & 3;
        for (int j = tid >> 2; j < tot; j += kRBlock / 4) {  // one quad per item
          const int loc = fs.item_node[j], code = fs.item_code[j];
          const NodeV m = load_node(&s_nodes[loc]);
          int cpuL, total;
          uint32_t gs[4];
          fgd_candidate(m, code, p, &cpuL, gs, &total);
          const uint32_t tb = 1u << m.gpu_type();
          const double F = rp.typed ? frag_F_quad<true>(cpuL, gs, total, tb, tp, fs.tp, rp.ncpu, rp.nt, q)
                                    : frag_F_quad<false>(cpuL, gs, total, tb, tp, fs.tp, rp.ncpu, rp.nt, q);
          if (q == 0) {
            if (code == 0) s_F0[loc] = F;
            else fs.F[j] = F;
          }
        }
        __syncthreads();
        mark(2);
        if (!kPF && pend && Kx > 1 && wv == 0 && c0 == 0) poll_once(pg);
        if (tid == 0) sh.nitems = 0;  // every thread has read tot; the next writer is past a barrier
        // fgd_score.go:100-141: every candidate lane scores itself; the node keeps the max,
        // ties to the lowest GPU index (fgd_score.go:128 keeps the first max)
        int v = -1;
        if (cand) v = fgd_frag_score(s_F0[i], fs.F[my_item]) * 16 + (15 - g);
        v = group8_max(v);
        // PWR + FGD: the node's raw PWR score and GPU choice by the same 8 lanes
        int pv = -1;
        bool perr = false;
        if constexpr (kPF) {
          bool ovf = false;
          if (feas) {
            const int2 pe = s_pe[i == ns ? vb : i];
            double e0 = s_E0[i];
            if (e0 == kEnergyStale) {
              e0 = node_energy_now(n, pe, sh.pw);
              if (g == 0) s_E0[i] = e0;
            }
            pv = pwr_cand8(n, p, pe, e0, sh.pw, g, &perr, &ovf);
          }
          if (ovf) atomicOr(a.fail, 2);
          pv = group8_max(pv);
        }
        // a feasible node with no candidate (share pod with milli 0 on a GPU-less node) scores 0
        const int raw = v < 0 ? 0 : v >> 4;
        const int gpu = (share && v >= 0) ? 15 - (v & 15) : -1;
        if constexpr (kPF) {
          // the node's raw PWR score and GPU choice (pwr_score.go:48-91) beside its FGD score
          int pgpu = -1;
          int praw = pwr8_finish(pv, &pgpu);
          int pinf = feas ? (kPfFeas | (perr ? kPfErr : 0) | (raw & 0xff) | ((pgpu + 1) & 0xf) << 8 |
                             ((gpu + 1) & 0xf) << 12)
                          : 0;
          if (hit) {
            praw = (int)me.x;
            pinf = pf_memo_pinf(me);
            feas = (pinf & kPfFeas) != 0;
            perr = (pinf & kPfErr) != 0;
          }
          if (valid && g == 0) {
            c_praw[i] = praw;
            c_pinf[i] = pinf;
            if (pmon && !hit && i < ns) s_pm[(size_t)p.pad * a.S + i] = pf_memo_pack(praw, pinf, s_pver[i]);
          }
        } else {
          const unsigned long long k = feas ? pack_key((unsigned)raw, n.name_rank, gpu, i == ns ? vb : i) : 0ull;
          route(valid && g == 0, i, feas, false, raw, k);
        }
        if (c0 + kFChunk < nsv) __syncthreads();  // F / items are reused by the next chunk
        mark(3);
      }
    } else if constexpr (kPwr) {
      // PWR: eight lanes per node (lane g <-> GPU g), the raw score biased into the key field
      if (pend && Kx > 1 && wv == 0) poll_once(pg);
      for (int c0 = 0; c0 < nsv; c0 += kFChunk) {
        const int cn = min(kFChunk, nsv - c0);
        const int i = c0 + (tid >> 3), g = tid & 7;
        const bool valid = (tid >> 3) < cn;
        NodeV n{};
        bool feas = false, perr = false, ovf = false;
        int pv = -1;
        if (valid) {
          n = load_node(&s_nodes[i]);
          feas = filter_node(n, p);
          if (feas) {
            const int2 pe = s_pe[i == ns ? vb : i];
            double e0 = s_E0[i];
            if (e0 == kEnergyStale) {
              e0 = node_energy_now(n, pe, sh.pw);
              if (g == 0) s_E0[i] = e0;
            }
            pv = pwr_cand8(n, p, pe, e0, sh.pw, g, &perr, &ovf);
          }
        }
        if (ovf) atomicOr(a.fail, 2);
        pv = group8_max(pv);
        int pgpu = -1;
        const int pr = pwr8_finish(pv, &pgpu);
        const unsigned raw = (unsigned)(pr + kPwrKeyBias);  // |pr| < 2^23 (else the run fails)
        const unsigned long long k =
            feas ? pack_key(raw, n.name_rank, rp.gpusel == SEL_PWR ? pgpu : -1, i == ns ? vb : i) : 0ull;
        route(valid && g == 0, i, feas, perr, (int)raw, k);
      }
    } else {
      if (pend && Kx > 1 && wv == 0) poll_once(pg);
      for (int c0 = 0; c0 < nsv; c0 += kChunk) {
        const int cn = min(kChunk, nsv - c0);
        const int i = c0 + tid;
        bool feas = false, e1 = false;
        int raw = 0;
        NodeV n{};
        if (tid < cn) {
          n = load_node(&s_nodes[i]);
          feas = filter_node(n, p);
          if (feas) {
            const int cap = (kPol == POL_DOTPROD && dp_norm(rp.dpcfg) == NORM_NODE) ? rp.cap[n_lo + (i == ns ? vb : i)] : 0;
            raw = cheap_score<kPol>(n, p, rp.seed, kTags ? &s_tags[(size_t)i * kTagStride] : nullptr, step, &e1,
                                    rp.dpcfg, cap);
          }
        }
        const unsigned long long k = feas ? pack_key((unsigned)raw, n.name_rank, -1, i == ns ? vb : i) : 0ull;
        route(tid < cn, i, feas, e1, raw, k);
      }
    }
    if (kPF && pend && Kx > 1 && wv == 0) {  // the pending round's granules: loads in flight over the barrier
      const unsigned long long* slot = gr + (size_t)(p_seq & 1) * Kx * kGranW;
#pragma unroll
      for (int j = 0; j < kS; ++j)
        if (lane + 64 * j < Kx) {
#pragma unroll
          for (int q = 0; q < 7; ++q) px[j][q] = gload(slot + (size_t)(lane + 64 * j) * kGranW + q);
        }
    }
    __syncthreads();
    mark(4);
    if constexpr (kPF) {
      // 1. the pending step (its round overlapped the evaluation above): decide and commit.  The owner of a winner
      //    other than its virtual node re-evaluates this step: that slot changed under the evaluation.
      if (pend) {
        if (wv == 0) {
          bool redo = false;
          const bool ok = pf_resolve(px, Kx > 1, true, &redo);
          if (lane == 0) {
            sh.pf_redo = redo ? 1 : 0;
            sh.pend_valid = 0;
            sh.pend_b = -1;
            if (!ok) { sh.stop = 1; atomicOr(a.fail, 1); }
          }
        }
        __syncthreads();
        if (sh.stop) break;
        if (sh.pf_redo) {  // the same step again, nothing pending
          --step;
          continue;
        }
      }
      mark(5);
      // 2. the slice's A totals and its best key under each of the class's two guessed ranges
      const int4 gs = s_gtab[p.pad & (kPfGuess - 1)];
      if (wv * 64 < ns) {
        int c = 0, e = 0, lo = INT_MAX, hi = INT_MIN;
        unsigned long long k0 = 0ull, k1 = 0ull;
        for (int i = tid; i < ns; i += kRBlock) {
          const int inf = c_pinf[i];
          if (inf & kPfFeas) {
            const int pr = c_praw[i];
            ++c;
            e |= (inf & kPfErr) ? 1 : 0;
            lo = min(lo, pr);
            hi = max(hi, pr);
            const unsigned long long q0 = pf_key(pr, inf, gs.x, gs.y, i), q1 = pf_key(pr, inf, gs.z, gs.w, i);
            k0 = q0 > k0 ? q0 : k0;
            k1 = q1 > k1 ? q1 : k1;
          }
        }
        c = wave_sum_dpp(c);
        e = __any(e != 0) ? 1 : 0;
        lo = wave_min_dpp(lo);
        hi = wave_max_dpp(hi);
        k0 = wave_max_u64_dpp(k0);
        k1 = wave_max_u64_dpp(k1);
        if (lane == 0 && c > 0) {
          atomicAdd(&sh.agg_cnt, c);
          if (e) atomicOr(&sh.agg_err, 1);
          atomicMin(&sh.agg_lo, lo);
          atomicMax(&sh.agg_hi, hi);
          atomicMax(&sh.agg_key, k0);
          atomicMax(&sh.agg_key1, k1);
        }
      }
      __syncthreads();
      // 3. publish the round, then prepare the virtual node: guess 0's local best with this step's Reserve + Bind
      if (wv == 0) {
        const unsigned long long mk = sh.agg_key, mk1 = sh.agg_key1;
        const int c = sh.agg_cnt, e = sh.agg_err, l = sh.agg_lo, h = sh.agg_hi;
        if (lane == 0) {
          if (Kx > 1) {
            unsigned long long* slot = gr + (size_t)(seq & 1) * Kx * kGranW + (size_t)wx * kGranW;
            const unsigned long long tag = (unsigned long long)(unsigned)(seq + 1) << 32;
            gstore(slot + 0, tag | (mk & 0xffffffffull));
            gstore(slot + 1, tag | (mk >> 32));
            gstore(slot + 2, tag | (mk1 & 0xffffffffull));
            gstore(slot + 3, tag | (mk1 >> 32));
            gstore(slot + 4, tag | (unsigned)l);
            gstore(slot + 5, tag | (unsigned)h);
            gstore(slot + 6, tag | ((unsigned)e << 31) | ((unsigned)c & 0x7fffffffu));
          }
          reset_agg();
        }
        const int mloc = key_loc(mk);
        int mask = -1;
        if (mk != 0ull) {
          NodeV bn = load_node(&s_nodes[mloc]);
          mask = select_gpus(bn, p, rp.gpusel, sel_arg<kPol == POL_DOTPROD>(rp, bn, p, n_lo + mloc, key_gpu(mk)), rp.seed,
                             step);
          if (mask >= 0) bind_node(bn, p, mask, +1);
          if (lane == 0) store_node(&s_nodes[ns], bn);
          else if (kTags && lane >= 2 && lane < 6) {
            uint2 t = reinterpret_cast<const uint2*>(&s_tags[(size_t)mloc * kTagStride])[lane - 2];
            if (mask >= 0 && p.tag >= 0 && (p.tag >> 2) == lane - 2) {
              const uint32_t inc = 1u << (16 * (p.tag & 1));
              t.x += (p.tag & 2) ? 0u : inc;
              t.y += (p.tag & 2) ? inc : 0u;
            }
            reinterpret_cast<uint2*>(&s_tags[(size_t)ns * kTagStride])[lane - 2] = t;
          } else if (lane == 6) {
            s_F0[ns] = mask >= 0 ? -1.0 : s_F0[mloc];
          } else if (lane == 7) {
            s_E0[ns] = mask >= 0 ? kEnergyStale : s_E0[mloc];
          }
        }
        p_step = step;
        p_cls = p.pad;
        p_seq = seq;
        p_b = mk != 0ull ? mloc : -1;
        p_key = mk;
        if (lane == 0) {
          sh.pf_key1 = mk1;
          sh.pf_g = gs;
          sh.pf_pod = p;
        }
        p_st0 = c; p_st1 = e; p_st2 = l; p_st3 = h;
        p_mask = mask;
        p_tag = mask >= 0 ? (int)p.tag : -1;
        ++seq;
        if (lane == 0) { sh.pend_valid = 1; sh.pend_b = p_b; }
      }
    } else if (wv == 0) {
      // the slice's aggregate without b (LDS atomics above), then b's two versions
      unsigned long long mk = sh.agg_key;
      int c = sh.agg_cnt, e = sh.agg_err, l = sh.agg_lo, h = sh.agg_hi;
      const unsigned long long k_pre = sh.pre_key, k_post = sh.post_key;
      const int f_pre = sh.pre_feas, f_post = sh.post_feas, e_pre = sh.pre_err, e_post = sh.post_err;
      // finish the pending exchange (its latency overlapped the evaluation above)
      bool owner = false, ok = true;
      unsigned long long W = 0ull;
      int gc = 0, ge = 0, gl = 0, gh = 0;
      if (pend) {
        W = exchange(pg, &gc, &ge, &gl, &gh, &ok);
        // b's post-Bind version only if the pending step binds: a Score error (framework.go:650-656,
        // e.g. BestFit's -1 on a node with less CPU left than the non-zero request) aborts the cycle
        owner = W != 0ull && W == p_key && !(gc > 1 && ge);
      }
      mark(5);
      // add b back: post-Bind if this workgroup owned the pending winner, else as it was
      if (vb >= 0 && (owner ? f_post : f_pre)) {
        const unsigned long long vk = owner ? k_post : k_pre;
        mk = vk > mk ? vk : mk;
        ++c;
        e |= owner ? e_post : e_pre;
        if (kMinMax) { l = min(l, key_score(vk)); h = max(h, key_score(vk)); }
      }
      if (ok) {
        if (lane == 0) {
          // publish this step first: granules {tag, key lo32}, {tag, key hi32}, {tag, err|hi|lo|cnt}
          if (Kx > 1) {
            unsigned long long* slot = gr + (size_t)(seq & 1) * Kx * kGranW;
            const unsigned long long tag = (unsigned long long)(unsigned)(seq + 1) << 32;
            // bit 17 (BestFit): the slice's feasible raw scores are not all equal (its max is mk's score)
            const unsigned stat = ((unsigned)e << 31) | (l < h ? 1u << 17 : 0u) | ((unsigned)c & 0x1ffff);
            gstore(slot + (size_t)wx * kGranW + 0, tag | (mk & 0xffffffffull));
            gstore(slot + (size_t)wx * kGranW + 1, tag | (mk >> 32));
            gstore(slot + (size_t)wx * kGranW + 2, tag | stat);
          }
          reset_agg();
        }
        if (pend) commit(W, gc, ge, gl, gh);
        // prepare the virtual node: this step's best node with this step's Reserve + Bind applied
        const int mloc = key_loc(mk);
        int mask = -1;
        if (mk != 0ull) {
          NodeV bn = load_node(&s_nodes[mloc]);
          mask = select_gpus(bn, p, rp.gpusel, sel_arg<kPol == POL_DOTPROD>(rp, bn, p, n_lo + mloc, key_gpu(mk)), rp.seed,
                             step);
          if (mask >= 0) bind_node(bn, p, mask, +1);
          if (lane == 0) store_node(&s_nodes[ns], bn);
          else if (kTags && lane >= 2 && lane < 6) {
            uint2 t = reinterpret_cast<const uint2*>(&s_tags[(size_t)mloc * kTagStride])[lane - 2];
            if (mask >= 0 && p.tag >= 0 && (p.tag >> 2) == lane - 2) {
              // +1 on u16 tag p.tag (counts stay far below 2^16, no carry across halves)
              const uint32_t inc = 1u << (16 * (p.tag & 1));
              t.x += (p.tag & 2) ? 0u : inc;
              t.y += (p.tag & 2) ? inc : 0u;
            }
            reinterpret_cast<uint2*>(&s_tags[(size_t)ns * kTagStride])[lane - 2] = t;
          } else if (lane == 6 && kFgd) {
            s_F0[ns] = mask >= 0 ? -1.0 : s_F0[mloc];
          } else if (lane == 7 && kPwr) {
            s_E0[ns] = mask >= 0 ? kEnergyStale : s_E0[mloc];
          }
        }
        p_step = step;
        p_cls = p.pad;
        p_seq = seq;
        p_b = mk != 0ull ? mloc : -1;
        p_key = mk;
        p_mask = mask;
        p_tag = mask >= 0 ? (int)p.tag : -1;
        p_st0 = c; p_st1 = e; p_st2 = l; p_st3 = h;
        ++seq;
        if (lane == 0) { sh.pend_valid = 1; sh.pend_b = p_b; }
      } else if (lane == 0) {
        sh.stop = 1;
        atomicOr(a.fail, 1);
      }
    }
    mark(6);
    __syncthreads();
    mark(7);
    if (sh.stop) break;
  }
  if (!sh.stop && __builtin_amdgcn_readfirstlane(sh.pend_valid)) finish_pending();
  if (prof && tid == 0) {
    sh.prof[10] = __builtin_amdgcn_s_memtime() - c_start;
    sh.prof[11] = __builtin_amdgcn_s_memrealtime() - t_start;
  }
  __syncthreads();
  if (prof && tid < kProfPhases) a.prof[(size_t)blockIdx.x * kProfPhases + tid] = sh.prof[tid];
  // write the slice back (final cluster state)
  for (int i = tid; i < ns; i += kRBlock) store_node(rp.nodes + n_lo + i, load_node(&s_nodes[i]));
  if (kTags)
    for (int i = tid; i < ns * kTagStride; i += kRBlock) rp.tags[(size_t)n_lo * kTagStride + i] = s_tags[i];
}

__global__ void k_advance(int* base, int k) { *base += k; }

// Reserve on an explicit node (ksim_engine_reserve): candidate F values for the
// FGD selector are evaluated by one workgroup, then thread 0 binds.
__global__ __launch_bounds__(64) void k_reserve(ReplicaDev* reps, const TypDev* __restrict__ tp_all, int r, PodDev p,
                                                int node, int step, int* out_mask, int sign, int mask_in) {
  const ReplicaDev rp = reps[r];
  const TypDev* __restrict__ tp = tp_all + (size_t)r * kMaxTypical;
  __shared__ double s_F[kMaxCand];
  const int tid = (int)threadIdx.x;
  NodeRec* nr = rp.nodes + node;
  uint16_t* tg = rp.tags + (size_t)node * kTagStride;
  if (sign < 0) {
    // removePod (cache.go:100-111, deviceinfo.go:39-60): every released device gets its milli back
    // without exceeding the device (left + milli <= 1000, the invariant of the packed u16 lanes), and
    // the CPU and memory stay within the node's allocatable; else nothing changes (e.g. a second
    // Unreserve of the same pod on a node still hosting another one)
    if (tid == 0) {
      const NodeV n = load_node(nr);
      bool ok = n.pods_left() < 32767 && (long long)n.cpu_left + p.cpu_req <= (long long)rp.cap[node] &&
                (long long)n.mem_left + p.mem <= (long long)rp.mcap[node];
      for (int g = 0; g < kMaxGpu; ++g)
        if ((mask_in >> g) & 1) ok = ok && g < n.gpu_cnt() && n.gl(g) + (int)p.milli <= kMilli;
      if (ok) apply_bind(nr, tg, p, mask_in, -1);
      *out_mask = ok ? mask_in : -1;
    }
    return;
  }
  if (mask_in >= 0) {
    // a predefined gpu-index (open_gpu_share.go:260-271): every named device must hold the milli
    if (tid == 0) {
      const NodeV n = load_node(nr);
      bool ok = true;
      for (int g = 0; g < kMaxGpu; ++g)
        if ((mask_in >> g) & 1) ok = ok && g < n.gpu_cnt() && n.gl(g) >= (int)p.milli;
      if (ok) apply_bind(nr, tg, p, mask_in, +1);
      *out_mask = ok ? mask_in : -1;
    }
    return;
  }
  const NodeV n = load_node(nr);
  const bool need_fgd = rp.gpusel == SEL_FGD && is_share_pod(p) && p.milli > 0;
  if (need_fgd) {
    if (tid < kMaxCand) {
      int gl[kMaxGpu];
      unpack_gl(n, gl);
      int cpuL = n.cpu_left;
      bool valid = true;
      if (tid > 0) {
        cpuL -= p.cpu_nz;
#pragma unroll
        for (int g = 0; g < kMaxGpu; ++g) {
          if (g == tid - 1) {
            valid = g < n.gpu_cnt() && gl[g] >= p.milli;
            gl[g] -= valid ? (int)p.milli : 0;
          }
        }
      }
      double F = 0.0;
      if (valid)
        F = rp.typed ? frag_F<true>(cpuL, gl, 1u << n.gpu_type(), tp, rp.ncpu, rp.nt)
                     : frag_F<false>(cpuL, gl, 1u << n.gpu_type(), tp, rp.ncpu, rp.nt);
      s_F[tid] = F;
    }
    __syncthreads();
  }
  if (tid != 0) return;
  int fgd_gpu = -1;
  if (need_fgd) {
    int bs = 0;
#pragma unroll
    for (int g = 0; g < kMaxGpu; ++g) {
      if (g < n.gpu_cnt() && n.gl(g) >= p.milli) {
        const int fs = fgd_frag_score(s_F[0], s_F[1 + g]);
        if (fgd_gpu < 0 || fs > bs) { bs = fs; fgd_gpu = g; }
      }
    }
  }
  if (rp.gpusel == SEL_PWR && is_share_pod(p) && p.milli > 0) {  // allocateGpuIdBasedOnPWRScore
    bool perr = false;
    (void)pwr_score(n, p, rp.cap[node], rp.cpum[node], *rp.pw, &fgd_gpu, &perr);
    if (perr) fgd_gpu = -1;
  }
  const int mask = select_gpus(n, p, rp.gpusel, sel_arg(rp, n, p, node, fgd_gpu), rp.seed, step);
  *out_mask = mask;
  if (mask >= 0) apply_bind(nr, tg, p, mask, +1);
}

#define KSIM_HIP(x)                                \
  do {                                             \
    hipError_t _e = (x);                           \
    if (_e != hipSuccess) {                        \
      std::fprintf(stderr, "ksim: %s failed: %s\n", #x, hipGetErrorString(_e)); \
      return KSIM_EHIP;                            \
    }                                              \
  } while (0)

}  // namespace

#include "ksim_host.hpp"
#include "ksim_report_host.hpp"
#include "ksim_desched_host.hpp"
#include "ksim_desched_merge_host.hpp"
#include "ksim_run_host.hpp"

// ---------------------------------------------------------------------------
// Host engine object
// ---------------------------------------------------------------------------
// The memoised FGD replays: each kernel's plan (ksim_plan.hpp), whether it holds, the replicas it was made for, and
// the device tables uploaded from it.
struct MemoState {  // k_memo
  MemoPlan plan;  // uploaded before the timed run
  bool ok = false;
  std::vector<int> reps;
  DevBuf<PodDev> pod;
  DevBuf<int> owner, wgcls, wgref;
  DevBuf<unsigned long long> wggrp;
  DevBuf<int> evo;
  DevBuf<int> evcls;       // decider mode: class of each event
  DevBuf<unsigned> hkeys;  // the keys in HBM (MemoPlan::hkeys)
  DevBuf<int> wgmap;       // each block's launch position << 8 | workgroup (MemoArgs::wg_map)
  DevBuf<unsigned> win;
  DevBuf<unsigned> topg;   // decider mode: top granules
};
struct HMemoState {  // k_hmemo (the keys in HBM)
  HPlan plan;
  bool ok = false;
  std::vector<int> reps;
  DevBuf<int> cg;
  DevBuf<PodDev> cls;
  DevBuf<uint16_t> cgrp;
  DevBuf<PodDev> gpod;
  DevBuf<int> mtoff;  // the per-model tables (typed replicas)
  DevBuf<uint8_t> mtab;
  DevBuf<double> na;  // their NA bins per (model, total), k_hinit_na
  DevBuf<int> evc;
  DevBuf<NodeRec> st;
  DevBuf<int> ns, nstate;
  DevBuf<unsigned> gsc, keys, l1;
  DevBuf<unsigned> l2;  // initial second maxima (HPlan::l2)
  DevBuf<int> cnt;
  DevBuf<unsigned long long> prof;
  DevBuf<uint8_t> hist;  // the wide form with deletes: per-workgroup bind history
};

enum DsPlan { kDsNone, kDsFrag, kDsCos };
struct DeschedState {  // the descheduling plan (desched_plan), made from the results and final node records of the
                       // last completed run: an engine holds one, of one policy
  DsPlan plan = kDsNone;
  std::vector<long long> eoff;      // [R + 1] each replica's offset in the per-event buffers
  std::vector<int32_t> budget, nv;  // [R] (on a shard, budget is the cap of its select: desched_plan)
  std::vector<int32_t> bound;       // [R] the pods bound (on a shard: to its own nodes)
  double ratio = 0;                 // the plan's ratio
  unsigned long long gen = 0;       // counts the plans made and dropped (a group's merged list names the plans it read)
  DevBuf<long long> d_eoff;
  DevBuf<uint8_t> gone;
  DevBuf<int32_t> cnt;              // [3][R] bound pods, budget, victims
  DevBuf<uint8_t> tab;              // the select kernel's per-node tables when they do not fit in LDS
  DevBuf<ksim_ds::EvalRec> eval;    // frag policies: per-event records, candidate lists, victims
  DevBuf<int32_t> plist;
  DevBuf<ksim_victim> vict;
  DevBuf<ksim_ds::CosRec> cos;      // cosSim: per-event records, victims
  DevBuf<ksim_cos_victim> cvict;
  DevEvent ev0, ev1;
  double last_ms = 0;
  void invalidate() { plan = kDsNone, ++gen; }
};

static hipError_t destroy_comm(ncclComm_t c);  // through the dlopen'd RCCL
using ShardComm = DevHandle<ncclComm_t, destroy_comm>;

struct ShardState {  // a node-sharded cluster's shard (ksim_engine_set_shard): its place, its transport and what that holds
  int world = 0;     // 0: not sharded
  int rank = 0, node_off = 0, n_global = 0;
  ShardTransport transport = ShardTransport::none;
  // the per-step exchange records (the k_step paths of every transport but peer)
  DevBuf<unsigned long long> d_send;  // this shard's record {best, nfeas, err, lo|hi}
  DevBuf<unsigned long long> d_recv;  // [world][4] gathered records
  ShardComm comm;                     // rccl (declared after the records it gathers: destroyed before they are freed)
  ksim_shard_exchange_fn xfn = nullptr;  // host (ksim_engine_set_shard_exchange)
  void* xuser = nullptr;
  std::vector<uint64_t> h_send, h_recv;  // its staging records
  // peer, one shard per process (ksim_shard_peer_handle / ksim_engine_set_shard_peers): this shard's exchange buffer
  // (uncached device memory, exported by IPC), the handle exported (exports differ per call), the peers' buffers
  // mapped here (closed before the own buffer is freed), the run epoch
  DevBuf<unsigned long long> d_pgran;
  std::vector<uint8_t> pgran_handle;
  PeerMap peers;
  int peer_epoch = 0;
  // What an in-process group (ksim_shard_group_run) keeps: on engine 0 of the group only, empty on every other engine.
  struct Group {
    DevBuf<unsigned long long*> d_ptrs;     // k_step path: the shards' send / recv pointer tables
    DevBuf<unsigned long long> d_ggran;     // k_hmemo_group: exchange granules
    DevBuf<ksim_hmemo::HMemoArgs> d_hgargs; // its per-shard arguments
    DevBuf<unsigned long long> d_rgran;     // k_replay group: exchange granules
    DevBuf<ReplicaDev> d_rgreps;            // its shards' replicas, and their list
    DevBuf<int> d_rglist;
    DevBuf<TypDev> d_rgtp;                  // and, for PWR+FGD, each shard's typical table (kMaxTypical entries apiece)
    DevBuf<RepAcc> d_rmerge;                // the merged report records (k_report_merge)
    int rmerge_n = -1;  // events they hold (-1: no group run with the report on since the events were loaded)
    // the merged descheduling plan (k_victim_merge; ksim_shard_group_deschedule): the list of the policy kind
    // `dplan`, its length and the cluster's budget, and the plan of every shard it was merged from
    DevBuf<ksim_victim> d_vmerge;
    DevBuf<ksim_cos_victim> d_cmerge;
    DevBuf<int32_t> d_nmerge;
    DevBuf<uint8_t> d_margs;  // k_victim_merge's arguments
    DsPlan dplan = kDsNone;
    int dmerge_n = 0, dbudget = 0;
    std::vector<unsigned long long> dgen;
  } group;

  // the entry points decide through these (ksim_run_host.hpp)
  bool on() const { return shard_on(transport); }
  bool runs_peer() const { return ::runs_peer(transport); }
  bool exchanges_on_host() const { return ::exchanges_on_host(transport); }
  bool exchanges_by_rccl() const { return ::exchanges_by_rccl(transport); }
  bool needs_group_run() const { return ::needs_group_run(transport, world); }
  bool takes_exchange_fn() const { return ::takes_exchange_fn(transport); }
  bool in_process() const { return ::in_process(transport, xfn != nullptr); }
  bool can_map_peers() const { return ::can_map_peers(transport, d_pgran.p && !pgran_handle.empty()); }
};

// Every device resource is a member handle (ksim_host.hpp) that frees itself: a new buffer is one new member and nothing
// else.  Declaration order carries meaning, since members go in reverse: the streams come first and so go last, after
// every buffer and event used on them, the communicator and the peers' mapped buffers (ShardState) included.  Before
// that the destructor sets the device, drains the side streams and then the engine's (no dispatch, or a profiler's
// completion callback on it, may outlive its buffers, streams or graph) and destroys the graph.
struct ksim_engine {
  int device = 0;
  static constexpr int kSide = kSideStreams;
  DevStream stream;
  DevStream side[kSide];  // for concurrent single-workgroup k_replay groups (created on first use)
  int N = 0, R = 0, NB = 64, bpr = 0, K = 256;
  int run_mode = 0;        // 0: auto (k_memo for FGD when it fits, else k_replay), 1: k_step per pod (hipGraph),
                           // 2: k_replay only, 3: k_memo required for FGD
  int wgs_req = 0;         // requested workgroups per replica (0 = auto)
  int cus = 256;
  bool coop = true;  // K > 1 persistent grids through hipLaunchCooperativeKernel (KSIM_COOP=0: plain launch)
  DevBuf<unsigned long long> d_gran;
  DevBuf<int2> d_hist;
  DevBuf<int> d_fail;
  DevBuf<int> d_replist;              // replicas ordered by policy (k_replay groups)
  DevBuf<unsigned long long> d_prof;  // KSIM_PROFILE=1: k_replay phase timers
  DevBuf<NodeRec> d_nodes;
  DevBuf<NodeRec> d_nodes_init;  // cluster state given to set_nodes (run() restarts from it)
  DevBuf<uint16_t> d_tags;  // per replica: N*16 u16 tags, then N int rank->index
  DevBuf<uint16_t> d_tags_init;
  size_t tags_stride = 0;      // u16 elements per replica
  DevBuf<TypDev> d_tp;
  DevBuf<Accum> d_acc;
  DevBuf<ReplicaDev> d_reps;
  DevBuf<int> d_base;
  DevBuf<int> d_scratch;     // single-pod calls: [0] mask
  DevBuf<PodDev> d_pod;      // single-pod calls
  DevBuf<ResultDev> d_res1;  // single-pod calls
  DevBuf<uint8_t> d_feas;
  DevBuf<int32_t> d_score;
  DevBuf<int32_t> d_gpu;
  std::vector<ReplicaDev> reps;
  std::vector<std::vector<ksim_node>> h_nodes;  // caller's static node fields per replica
  std::vector<DevBuf<PodDev>> d_ev;
  std::vector<DevBuf<ResultDev>> d_res;
  std::vector<int> n_events;
  std::vector<char> has_delete;  // the replica's stream has deletion events (k_replay keeps a bind history)
  std::vector<int> n_create;     // its creation events (a shard's descheduling cap)
  // k_memo (memoised FGD replay): per replica the distinct pod requests of its creation events
  // (PodDev.pad = class id) and how many events each has
  std::vector<std::vector<PodDev>> h_cls;
  std::vector<std::vector<TypDev>> h_tp;  // each replica's typical table as uploaded (k_hmemo's per-model tables)
  std::vector<std::vector<int>> h_cls_n;
  std::vector<std::vector<int>> h_ev_cls;  // class of each event, -1 delete
  MemoState memo;
  HMemoState hmemo;
  // their cache key: the plans hold until events, policies, nodes, typical tables or hints change
  bool mplan_dirty = true;
  std::vector<int> mplan_all;  // the FGD replicas the plans were made for
  int mplan_max_ev = -1;
  bool split_fgd = false;      // the wide-hinted FGD replicas on k_memo beside the others on k_hmemo (one run)
  DevBuf<unsigned long long> d_done;  // [2 + R] the overlapped report's queue (ksim_scan1.hpp Scan1Args::done)
  DevBuf<__int128> d_ragg;     // [R][kScanPartsMax][2][kFields] the multi-workgroup report scan's part sums
  unsigned done_epoch = 0;
  DevEvent ev_ovl;    // the queue's tickets zeroed (the report's stream waits on it)
  DevBuf<double> d_th;       // FGD score steps (build_score_thresholds), null if unusable
  std::vector<int> wgs_hint;    // per replica: workgroups asked by ksim_engine_set_replica_wgs (0: the engine's choice)
  std::vector<DevEvent> grp_rev;  // concurrent groups' report kernels: a timing event pair per group
  int grp_rev_used = 0;             // pairs recorded by the last run
  int scan1 = 2;       // single-workgroup cheap-policy groups on k_scan1, node records in VGPRs where they fit
                       // (KSIM_VARIANT scan1=1: records in LDS; 0: k_replay)
  std::vector<std::vector<NodeRec>> h_rec;  // the records set_nodes gave each replica (k_hmemo's initial states)
  std::vector<int> nt;
  GraphExec graph;
  int graph_R = -1;
  bool graph_pwr = false;    // the graph carries k_step_pwr after every k_step
  DevBuf<PowerDev> d_pw;  // [R] PWR energy model
  DevBuf<uint8_t> d_cpum; // [R][N] CPU model id per node
  DevBuf<int2> d_pws;     // [R][N] PWR phase-A scratch
  std::vector<char> pw_set;  // set_power_model called
  // KSIM_POLICY_WEIGHTED: per replica the kNumPlugins weights and the plugin mask (k_wsum's argument table, uploaded
  // at launch), and whether ksim_engine_set_plugin_weights has set them since the policy was set
  std::vector<std::array<int32_t, ksim_wsum::kWStride>> wsum_w;
  std::vector<char> wsum_set;
  DevBuf<int> d_wsum;     // [R][kWStride]
  DevEvent ev0, ev1, ev_mid;
  MappedFlags started;  // residency gate: host-mapped flags, one per FGD workgroup
  int gate_epoch = 0;
  long long gate_timeouts = 0;  // gates given up at their bound, over the engine's life
  DevEvent side_ev[kSide];
  DevEvent ev_fork;
  bool report_done = false;
  // KSIM_GROUP_TIMES=1: timing events at the fork and at each used side stream's end (the last run's
  // concurrent groups, printed on stderr after the run)
  DevEvent tev_fork;
  DevEvent tev_side[kSide];
  unsigned tev_used = 0u;
  // cluster report (ksim_engine_set_report)
  bool report = false;
  DevBuf<int32_t> d_cap;   // [R][N] allocatable milli-CPU
  DevBuf<int32_t> d_mcap;  // [R][N] allocatable memory, MiB (Unreserve's removePod guard)
  DevBuf<int32_t> d_last;  // [R][N] k_step: last event that changed each node
  std::vector<DevBuf<NodeRec>> d_snap;
  std::vector<DevBuf<int32_t>> d_prev;
  std::vector<DevBuf<RepAcc>> d_rep;
  std::vector<int64_t> total_gpus;
  bool rep_ready = false;      // the records of d_rep are those of a completed run (ksim_engine_get_report_parts)
  ShardState shard;            // node-sharded cluster (ksim_engine_set_shard)
  // the Random draw structure on Go's math/rand stream (ksim_engine_set_go_stream): per replica the
  // source state {vec[607], tap, feed}, empty = the hash contract
  std::vector<std::vector<unsigned long long>> go_state;
  DevBuf<unsigned long long> d_go;
  RunStats stats;        // the last run's diagnostics (ksim_run_host.hpp)
  bool ran = false;     // a ksim_engine_run completed since the last set_nodes / set_typical / load_events
  DeschedState ds;       // the descheduling plan made from that run
  ~ksim_engine();
};

static int check_gfx950(int dev) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= dev) return KSIM_ENODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return KSIM_ENODEV;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return KSIM_ENODEV;
  return KSIM_OK;
}

static int alloc_report(ksim_engine* e, int r);

static int upload_reps(ksim_engine* e) {
  KSIM_HIP(hipMemcpyAsync(e->d_reps.p, e->reps.data(), sizeof(ReplicaDev) * e->R, hipMemcpyHostToDevice, e->stream));
  return KSIM_OK;
}

// Workgroups of kernel `f` (1024 threads, `lds` B of dynamic LDS) that can be resident at once on the
// CUs the engine may use: the occupancy query times the CU count.  A persistent grid whose workgroups
// exchange granules (K > 1) must not exceed it.
static int resident_cap(const ksim_engine* e, const void* f, size_t lds);
static int run_hmemo_peer(ksim_engine* e, const RunEnv& env, int max_ev);

// A persistent launch: K > 1 workgroups per replica poll each other's granules every step, so the
// whole grid must be resident -- a cooperative launch, which the runtime refuses up front
// (hipErrorCooperativeLaunchTooLarge) instead of letting a non-resident workgroup stall the pollers.
// K = 1 needs no co-residency: a plain launch (it may share the device with side-stream groups).
template <typename A>
static int launch_persistent(const void* f, int grid, int block, size_t lds, hipStream_t st, bool coop, A& args,
                             const TypDev*& tp) {
  KSIM_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  void* params[] = {(void*)&args, (void*)&tp};
  const hipError_t r = coop ? hipLaunchCooperativeKernel(f, dim3(grid), dim3(block), params, (unsigned)lds, st)
                            : hipLaunchKernel(f, dim3(grid), dim3(block), params, lds, st);
  if (r == hipErrorCooperativeLaunchTooLarge) {
    std::fprintf(stderr, "ksim: %d co-resident workgroups of %zu B LDS do not fit the device\n", grid, lds);
    (void)hipGetLastError();
    return KSIM_ERANGE;
  }
  KSIM_HIP(r);
  return KSIM_OK;
}

// k_scan1 for the policies it serves, else null (reg: the node records in VGPRs)
template <bool R, bool G>
static const void* scan1_fn(int pol) {
  switch (pol) {
    case POL_BESTFIT: return (const void*)ksim_scan1::k_scan1<POL_BESTFIT, R, G>;
    case POL_DOTPROD: return (const void*)ksim_scan1::k_scan1<POL_DOTPROD, R, G>;
    case POL_PACKING: return (const void*)ksim_scan1::k_scan1<POL_PACKING, R, G>;
    case POL_CLUSTERING: return (const void*)ksim_scan1::k_scan1<POL_CLUSTERING, R, G>;
    case POL_RANDOM: return (const void*)ksim_scan1::k_scan1<POL_RANDOM, R, G>;
    default: return nullptr;
  }
}
// k_wsum by what the launch carries: FGD's evaluation, PWR's energy model, deletes and report stores
template <bool F, bool P>
static const void* wsum_fn(bool general) {
  return general ? (const void*)ksim_wsum::k_wsum<F, P, true> : (const void*)ksim_wsum::k_wsum<F, P, false>;
}
static const void* scan1_fn(int pol, bool report, bool reg) {
  return report ? (reg ? scan1_fn<true, true>(pol) : scan1_fn<true, false>(pol))
                : (reg ? scan1_fn<false, true>(pol) : scan1_fn<false, false>(pol));
}

template <int P, bool G>
static const void* replay_fn(int K) {
  return K == 1 ? (const void*)k_replay<P, 0, G> : K <= 64 ? (const void*)k_replay<P, 1, G> : (const void*)k_replay<P, 4, G>;
}
template <int P>
static const void* replay_fn(int K, bool general) {
  return general ? replay_fn<P, true>(K) : replay_fn<P, false>(K);
}
static const void* replay_kernel(int pol, int K, bool general) {
  switch (pol) {
    case POL_FGD: return replay_fn<POL_FGD>(K, general);
    case POL_BESTFIT: return replay_fn<POL_BESTFIT>(K, general);
    case POL_DOTPROD: return replay_fn<POL_DOTPROD>(K, general);
    case POL_PACKING: return replay_fn<POL_PACKING>(K, general);
    case POL_CLUSTERING: return replay_fn<POL_CLUSTERING>(K, general);
    case POL_PWR: return replay_fn<POL_PWR>(K, general);
    case POL_PWR_FGD: return replay_fn<POL_PWR_FGD>(K, general);
    default: return replay_fn<POL_RANDOM>(K, general);
  }
}

// ---- k_memo / k_hmemo: the plans (ksim_plan.hpp) onto the device ----
// The instantiation of each form (memo_form, hmemo_form): the only place that names them.  No default: a form with no
// instantiation is a compiler warning here, and a null kernel the launch refuses.
static const void* memo_kernel(MemoForm f) {
  using ksim_memo::k_memo;
  switch ((MemoFormCode)f.code()) {
    case kMemoLean: return (const void*)k_memo<false, false>;
    case kMemoDecider: return (const void*)k_memo<true, true>;
    case kMemoGeneral: return (const void*)k_memo<false, true>;
    case kMemoStress: return (const void*)k_memo<false, false, true>;
    case kMemoReport: return (const void*)k_memo<false, false, false, true>;
    case kMemoHKeysLean: return (const void*)k_memo<false, false, false, false, true>;
    case kMemoHKeysGeneral: return (const void*)k_memo<false, true, false, false, true>;
    case kMemoHKeysReport: return (const void*)k_memo<false, false, false, true, true>;
  }
  return nullptr;
}
static const void* hmemo_kernel(HMemoForm f) {
  using ksim_hmemo::k_hmemo;
  using ksim_hmemo::k_hmemo_group;
  switch ((HMemoFormCode)f.code()) {
    case kHMemoOne: return (const void*)k_hmemo<0, false>;
    case kHMemoOneProf: return (const void*)k_hmemo<0, true>;
    case kHMemoOneModel: return (const void*)k_hmemo<0, false, true>;
    case kHMemoOneProfModel: return (const void*)k_hmemo<0, true, true>;
    case kHMemoWide: return (const void*)k_hmemo<1, false>;
    case kHMemoWideProf: return (const void*)k_hmemo<1, true>;
    case kHMemoWide4: return (const void*)k_hmemo<4, false>;
    case kHMemoWide4Prof: return (const void*)k_hmemo<4, true>;
    case kHMemoGroup: return (const void*)k_hmemo_group<1, false>;
    case kHMemoGroupProf: return (const void*)k_hmemo_group<1, true>;
    case kHMemoGroup4: return (const void*)k_hmemo_group<4, false>;
    case kHMemoGroup4Prof: return (const void*)k_hmemo_group<4, true>;
  }
  return nullptr;
}

// The FGD score steps, built once per process on the host (nullptr if the check fails: k_memo
// then evaluates the sigmoid expression itself).
static const double* score_table() {
  static double th[102];
  static const bool ok = build_score_thresholds(th);
  return ok ? th : nullptr;
}

// The table on the device, uploaded on first use; d_th stays null without a table.
static int ensure_score_table(ksim_engine* e, hipStream_t st) {
  if (e->d_th.p || !score_table()) return KSIM_OK;
  if (const int rc = e->d_th.alloc(102)) return rc;
  KSIM_HIP(hipMemcpyAsync(e->d_th.p, score_table(), sizeof(double) * 102, hipMemcpyHostToDevice, st));
  return KSIM_OK;
}

// What the planners read of the engine, for the replicas `reps` in launch order; residency is k_memo's.
static PlanInput plan_input(const ksim_engine* e, const RunEnv& env, const std::vector<int>& reps, bool decider = false) {
  PlanInput in;
  for (int r : reps)
    in.reps.push_back({&e->h_cls[r], &e->h_ev_cls[r], &e->h_rec[r], &e->h_tp[r], e->reps[r].typed, e->reps[r].ncpu,
                       e->reps[r].nt});
  in.N = e->N;
  in.node_off = e->shard.node_off;
  in.cus = e->cus;
  in.wgs_req = e->wgs_req;
  in.run_mode = e->run_mode;
  in.decider = decider;
  in.hl2 = env.hl2;
  in.hmodel = env.hmodel;
  in.score_table = score_table() != nullptr;
  in.resident = [e](size_t lds) { return resident_cap(e, (const void*)ksim_memo::k_memo<false, false>, lds); };
  return in;
}

static int prepare_hmemo(ksim_engine* e, const RunEnv& env, const std::vector<int>& reps, int max_ev, int forceK = 0,
                         int forceS = 0) {
  e->hmemo.ok = false;
  HPlan& pl = e->hmemo.plan;
  const int stride = std::max(max_ev, 1);
  if (!hmemo_plan(plan_input(e, env, reps), stride, pl, forceK, forceS)) return KSIM_OK;
  const int Rg = (int)reps.size();
  e->hmemo.reps = reps;
  hipStream_t st = e->stream;
  int rc;
  if ((rc = e->hmemo.cg.upload(pl.cg, st))) return rc;
  if ((rc = e->hmemo.cls.upload(pl.cls, st))) return rc;
  if ((rc = e->hmemo.cgrp.upload(pl.cgrp, st))) return rc;
  if ((rc = e->hmemo.gpod.upload(pl.gpod, st))) return rc;
  if ((rc = e->hmemo.evc.upload(pl.evc, st))) return rc;
  if ((rc = e->hmemo.st.upload(pl.st, st))) return rc;
  if ((rc = e->hmemo.ns.upload(pl.ns, st))) return rc;
  if ((rc = e->hmemo.nstate.upload(pl.nstate, st))) return rc;
  if ((rc = e->hmemo.gsc.ensure((size_t)Rg * pl.Gmax * pl.Smax))) return rc;
  if ((rc = e->hmemo.keys.ensure((size_t)Rg * pl.Cmax * pl.Npad))) return rc;
  if ((rc = e->hmemo.l1.ensure((size_t)Rg * pl.Cmax * pl.nb))) return rc;
  if (pl.l2 && (rc = e->hmemo.l2.ensure((size_t)Rg * pl.Cmax * pl.nb))) return rc;
  if ((rc = e->hmemo.cnt.ensure((size_t)Rg * pl.Cmax))) return rc;
  if (pl.Mtab > 0) {
    if ((rc = e->hmemo.mtoff.upload(pl.mtoff, st))) return rc;
    if ((rc = e->hmemo.mtab.upload(pl.mtab, st))) return rc;
    if ((rc = e->hmemo.na.ensure((size_t)Rg * pl.Mslots * ksim_hmemo::kNaStride))) return rc;
  }
  if ((rc = ensure_score_table(e, st))) return rc;
  KSIM_HIP(hipStreamSynchronize(st));  // the host vectors are pageable
  e->hmemo.ok = true;
  return KSIM_OK;
}

// Plan and upload the k_memo launch of the FGD replicas (before the timed region of a run; cached
// until events or policies change).
static int upload_memo(ksim_engine* e, const PlanInput& in, const std::vector<int>& reps, int max_ev);

static int prepare_memo(ksim_engine* e, const RunEnv& env, int max_ev) {
  if (e->run_mode == 1 || e->run_mode == 2 || e->shard.on()) return KSIM_OK;
  std::vector<int> reps, wide, narrow;
  for (int r = 0; r < e->R; ++r)
    if (e->reps[r].policy == POL_FGD) {
      reps.push_back(r);
      (e->wgs_hint[r] > 1 ? wide : narrow).push_back(r);
    }
  if (!e->mplan_dirty && reps == e->mplan_all && max_ev == e->mplan_max_ev) return KSIM_OK;
  e->mplan_dirty = false;
  e->mplan_all = reps;
  e->mplan_max_ev = max_ev;
  e->memo.ok = false;
  e->hmemo.ok = false;
  e->split_fgd = false;
  e->memo.reps.clear();
  e->hmemo.reps.clear();
  if (reps.empty()) return KSIM_OK;
  if (e->run_mode == 5) return prepare_hmemo(e, env, reps, max_ev);  // k_hmemo required
  MemoPlan& pl = e->memo.plan;
  // run_mode 4 (or KSIM_VARIANT=memo_decider=1 with run_mode 0): the decider variant of k_memo
  const bool decider = e->run_mode == 4 || (e->run_mode == 0 && env.memo_decider);
  // run_mode 0 with some FGD replicas hinted wide (ksim_engine_set_replica_wgs, the paper sweep's longest chains):
  // those on k_memo, each at its hinted width (the keys in HBM when they do not fit in LDS), the others on k_hmemo at
  // one workgroup each, both groups in one concurrent run (run_persistent)
  if (e->run_mode == 0 && !wide.empty() && !narrow.empty() && !decider) {
    std::vector<int> kr;  // each wide replica at its own hinted width
    for (int r : wide) kr.push_back(e->wgs_hint[r]);
    const PlanInput in = plan_input(e, env, wide);
    if (memo_plan(in, pl, 0, true, &kr)) {
      int rc = upload_memo(e, in, wide, max_ev);
      if (rc) return rc;
      rc = prepare_hmemo(e, env, narrow, max_ev);
      if (rc) return rc;
      if (e->hmemo.ok && e->hmemo.plan.K == 1) {
        e->split_fgd = true;
        return KSIM_OK;
      }
      e->memo.ok = false;  // no one-workgroup plan for the others: one plan for every FGD replica, below
      e->memo.reps.clear();
      e->hmemo.ok = false;
    }
  }
  std::vector<int> kr;  // every FGD replica hinted: each at its width
  if (wide.size() == reps.size())
    for (int r : reps) kr.push_back(e->wgs_hint[r]);
  const PlanInput in = plan_input(e, env, reps, decider);
  if (!memo_plan(in, pl, 0, e->run_mode == 3 || !kr.empty(), kr.empty() ? nullptr : &kr))
    return e->run_mode == 0 ? prepare_hmemo(e, env, reps, max_ev) : KSIM_OK;
  return upload_memo(e, in, reps, max_ev);
}

// Upload the k_memo plan of `reps` (memo_plan made it from `in`): the per-class tables, the owner code of every event.
static int upload_memo(ksim_engine* e, const PlanInput& in, const std::vector<int>& reps, int max_ev) {
  MemoPlan& pl = e->memo.plan;
  const int Rg = (int)reps.size();
  int rc;
  const int stride = std::max(max_ev, 1);
  if ((rc = e->memo.win.ensure((size_t)Rg * stride))) return rc;
  if ((rc = e->memo.topg.ensure((size_t)Rg * stride * ksim_memo::kTopWords))) return rc;
  const MemoEvents t = memo_events(in, pl, stride);
  hipStream_t st = e->stream;
  if ((rc = e->memo.evo.upload(t.evo, st))) return rc;
  if ((rc = e->memo.evcls.upload(t.evcls, st))) return rc;
  if ((rc = e->memo.pod.upload(pl.pod, st))) return rc;
  if ((rc = e->memo.owner.upload(pl.owner, st))) return rc;
  if ((rc = e->memo.wgcls.upload(pl.wgcls, st))) return rc;
  if ((rc = e->memo.wgref.upload(pl.wgref, st))) return rc;
  if ((rc = e->memo.wggrp.upload(pl.wggrp, st))) return rc;
  if ((rc = ensure_score_table(e, st))) return rc;
  if ((rc = e->memo.wgmap.upload(t.wgmap, st))) return rc;
  KSIM_HIP(hipStreamSynchronize(st));  // the host vectors are pageable and short-lived
  if (pl.hkeys && (rc = e->memo.hkeys.ensure((size_t)pl.nwg * pl.Cw * e->N))) return rc;
  e->memo.reps = reps;
  e->memo.ok = true;
  return KSIM_OK;
}

// KSIM_PROFILE=2: the step trace of the launch just enqueued (d_trace: kTrace words per workgroup and each of the first
// TS steps).
static int print_memo_trace(ksim_engine* e, const MemoPlan& pl, DevBuf<unsigned long long>& d_trace, int TS, hipStream_t st) {
  constexpr int kT = ksim_memo::kTrace;
  // per step: owner's start -> publish, publish -> each other workgroup's receive, receive -> start
  // (s_memrealtime, 100 MHz); replica 0 only
  KSIM_HIP(hipStreamSynchronize(st));
  const int K = pl.Kr[0];
  std::vector<unsigned long long> h((size_t)kT * pl.nwg * TS);
  KSIM_HIP(hipMemcpy(h.data(), d_trace.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
  d_trace.release();
  std::vector<int> evo((size_t)TS);
  KSIM_HIP(hipMemcpy(evo.data(), e->memo.evo.p, sizeof(int) * TS, hipMemcpyDeviceToHost));
  auto at = [&](int w, int s, int k) { return (double)h[((size_t)w * TS + s) * kT + k]; };
  double crit = 0, hand = 0, hmax = 0, period = 0, lag = 0, f0 = 0, spin = 0, nhand = 0;
  int nc = 0, nh = 0, nf = 0, nn = 0;
  // the steps whose granule left before the critical F (d cannot host the step's class), [1], against the others, [0]
  double ecrit[2] = {0, 0}, ehand[2] = {0, 0};
  int enc[2] = {0, 0}, enn[2] = {0, 0}, nearly = 0;
  for (int s = 0; s < TS; ++s)  // every traced step, the first and the last included
    if (evo[s] >= 0 && at(evo[s] >> 16, s, 3) > at(evo[s] >> 16, s, 1)) ++nearly;
  for (int s = 1; s + 1 < TS; ++s) {
    if (evo[s] < 0 || evo[s + 1] < 0) continue;
    const int o = evo[s] >> 16, o2 = evo[s + 1] >> 16;
    crit += at(o, s, 1) - at(o, s, 0);
    const int ee = at(o, s, 3) > at(o, s, 1) ? 1 : 0;  // the F join came after the publish
    ecrit[ee] += at(o, s, 1) - at(o, s, 0);
    ++enc[ee];
    if (at(o, s, 2) > 0 && at(o, s, 3) > 0) {
      f0 += at(o, s, 3) - at(o, s, 0);   // start -> all critical F done
      spin += at(o, s, 2) - at(o, s, 3); // -> fresh key known
      ++nf;
    }
    period += at(o2, s + 1, 1) - at(o, s, 1);
    if (o2 != o) lag += at(o2, s + 1, 0) - at(o2, s, 1);  // next owner: receive s -> start s+1
    if (o2 != o) {  // the hand-off the chain goes through: the next owner's own receive, not the mean of all
      nhand += at(o2, s, 1) - at(o, s, 1);
      ++nn;
      ehand[ee] += at(o2, s, 1) - at(o, s, 1);
      ++enn[ee];
    }
    ++nc;
    for (int w = 0; w < K; ++w) {
      if (w == o) continue;
      const double d = at(w, s, 1) - at(o, s, 1);
      hand += d;
      hmax = std::max(hmax, d);
      ++nh;
    }
  }
  if (nc && nh)
    std::fprintf(stderr, "ksim memo trace (replica 0, %d steps, us): owner start->publish %.3f; publish->receive mean %.3f max %.3f; "
                 "next owner receive->start %.3f; publish->publish %.3f; owner start->all F done %.3f, ->fresh key %.3f; "
                 "next owner publish->receive %.3f (%d of %d steps hand over)\n",
                 TS, crit / nc / 100, hand / nh / 100, hmax / 100, lag / nc / 100, period / nc / 100,
                 nf ? f0 / nf / 100 : 0.0, nf ? (f0 + spin) / nf / 100 : 0.0, nn ? nhand / nn / 100 : 0.0, nn, nc);
  if (nc && nh)
    std::fprintf(stderr, "ksim memo trace, early publish (d cannot host the step's class): %d of the %d traced steps; owner "
                 "start->publish early %.3f (%d), other %.3f (%d); next owner publish->receive early %.3f (%d), other %.3f (%d)\n",
                 nearly, TS, enc[1] ? ecrit[1] / enc[1] / 100 : 0.0, enc[1], enc[0] ? ecrit[0] / enc[0] / 100 : 0.0, enc[0],
                 enn[1] ? ehand[1] / enn[1] / 100 : 0.0, enn[1], enn[0] ? ehand[0] / enn[0] / 100 : 0.0, enn[0]);
  return KSIM_OK;
}

// KSIM_PROFILE=1: the phase table of the launch just enqueued (d_prof).
static int print_memo_profile(ksim_engine* e, const MemoPlan& pl, int Rg, int max_ev, hipStream_t st) {
  KSIM_HIP(hipStreamSynchronize(st));
  const int nb = pl.nwg, P = ksim_memo::kProfPhases;
  std::vector<unsigned long long> h((size_t)nb * P);
  KSIM_HIP(hipMemcpy(h.data(), e->d_prof.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
  static const char* names[] = {"init", "A:crit-F+list", "syncA", "B:publish", "B:eval", "syncB", "C:keys", "top2",
                                "poll+bind", "end-sync"};
  std::fprintf(stderr, "ksim memo profile: %d workgroups (K=%d Cw=%d nfw=%d), %d steps; us/step mean [max]:", nb, pl.K,
               pl.Cw, pl.nfw, max_ev);
  double init = 0;
  for (int b = 0; b < nb; ++b) init += (double)h[(size_t)b * P] / 1e5;
  std::fprintf(stderr, " (init %.3f ms)", init / nb);
  for (int ph = 1; ph < 10; ++ph) {
    double sum = 0, mx = 0;
    for (int b = 0; b < nb; ++b) {
      const double us = (double)h[(size_t)b * P + ph] / 100.0 / std::max(max_ev, 1);
      sum += us;
      mx = std::max(mx, us);
    }
    std::fprintf(stderr, " %s %.3f [%.3f];", names[ph], sum / nb, mx);
  }
  double cyc = 0, tick = 0;
  for (int b = 0; b < nb; ++b) { cyc += (double)h[(size_t)b * P + 10]; tick += (double)h[(size_t)b * P + 11]; }
  for (int ph = 12; ph < 21; ++ph) {
    double sum = 0;
    for (int b = 0; b < nb; ++b) sum += (double)h[(size_t)b * P + ph] / 100.0 / std::max(max_ev, 1);
    static const char* extra[] = {"listwave-A", "listwave-C", "step-start loads", "owner A per step",
                                  "owner: prefetch done", "crit F all done", "keys", "result written",
                                  "granule stored"};
    // owner phases: summed over the K workgroups of a replica (one owner per step)
    std::fprintf(stderr, " %s %.3f;", extra[ph - 12], ph >= 15 ? sum / std::max(Rg, 1) : sum / nb);
  }
  if (pl.decider) {  // the deciders' own phases (workgroup 0 of each replica)
    static const char* dn[] = {"list + top wait", "F", "decide + bind", "end barrier"};
    std::fprintf(stderr, " | decider:");
    for (int ph = 20; ph < 24; ++ph) {
      double sum = 0;
      for (int b = 0; b < nb; b += pl.K) sum += (double)h[(size_t)b * P + ph] / 100.0 / std::max(max_ev, 1);
      std::fprintf(stderr, " %s %.3f;", dn[ph - 20], sum / std::max(nb / pl.K, 1));
    }
  }
  if (tick > 0) std::fprintf(stderr, " shader clock %.0f MHz, wall %.3f ms", cyc / tick * 100.0, tick / nb / 1e5);
  std::fprintf(stderr, "\n");
  return KSIM_OK;
}

// st: the stream (a concurrent run's side stream, else the engine's); started / gate_epoch: the residency gate's
// flags (a concurrent run launches the next group once every workgroup of this one has started: a plain launch
// then, since the device is otherwise idle until the gate opens)
static int launch_memo(ksim_engine* e, const RunEnv& env, const MemoPlan& pl, int Rg, int first, int max_ev, hipStream_t st,
                       int* started = nullptr, int gate_epoch = 0) {
  int rc;
  const int stride = std::max(max_ev, 1);
  KSIM_HIP(hipMemsetAsync(e->memo.win.p, 0, sizeof(unsigned) * (size_t)Rg * stride, st));
  if (pl.decider)
    KSIM_HIP(hipMemsetAsync(e->memo.topg.p, 0, sizeof(unsigned) * (size_t)Rg * stride * ksim_memo::kTopWords, st));
  ksim_memo::MemoArgs ma;
  ma.reps = e->d_reps.p;
  ma.rep_list = e->d_replist.p + first;
  ma.wg_map = e->memo.wgmap.p;
  ma.N = e->N;
  ma.K = pl.K;
  ma.Cw = pl.Cw;
  ma.nfw = pl.nfw;
  ma.Cmax = pl.Cmax;
  ma.cls_pod = e->memo.pod.p;
  ma.cls_owner = e->memo.owner.p;
  ma.wg_cls = e->memo.wgcls.p;
  ma.wg_ref = e->memo.wgref.p;
  ma.wg_grp = e->memo.wggrp.p;
  ma.ev_owner = e->memo.evo.p;
  ma.th = e->d_th.p;
  ma.win = e->memo.win.p;
  ma.win_stride = stride;
  ma.fail = e->d_fail.p;
  ma.prof = nullptr;
  ma.trace = nullptr;
  ma.trace_steps = 0;
  ma.decider = pl.decider ? 1 : 0;
  ma.ev_cls = e->memo.evcls.p;
  ma.topg = e->memo.topg.p;
  ma.hkeys = pl.hkeys ? e->memo.hkeys.p : nullptr;
  ma.started = started;
  ma.gate_epoch = gate_epoch;
  ma.skip = env.skip;
  ma.delay = env.hdelay;
  const bool profile = env.timers();
  const bool tracing = env.profile == 2;
  DevBuf<unsigned long long> d_trace;
  const int TS = std::min(max_ev, 4000);
  if (tracing) {
    if ((rc = d_trace.alloc(ksim_memo::kTrace * (size_t)pl.nwg * TS))) return rc;
    if ((rc = d_trace.zero(st))) return rc;
    ma.trace = d_trace.p;
    ma.trace_steps = TS;
  }
  if (profile) {
    if ((rc = e->d_prof.ensure((size_t)pl.nwg * ksim_memo::kProfPhases))) return rc;
    KSIM_HIP(hipMemsetAsync(e->d_prof.p, 0, sizeof(unsigned long long) * (size_t)pl.nwg * ksim_memo::kProfPhases, st));
    ma.prof = e->d_prof.p;
  }
  const bool any_delete = std::any_of(e->memo.reps.begin(), e->memo.reps.end(), [&](int r) { return e->has_delete[r] != 0; });
  const void* f = memo_kernel(memo_form(pl.decider, pl.hkeys, profile, tracing, e->d_th.p != nullptr, any_delete, e->report,
                                        ma.delay));
  const TypDev* tpp = e->d_tp.p;
  rc = launch_persistent(f, pl.nwg, ksim_memo::kMBlock, pl.lds, st, e->coop && pl.K > 1 && !started, ma, tpp);
  if (rc) return rc;
  hipLaunchKernelGGL(ksim_memo::k_memo_finish, dim3((unsigned)((stride + 255) / 256), (unsigned)Rg), dim3(256), 0, st,
                     e->d_reps.p, (const int*)(e->d_replist.p + first), e->N);
  KSIM_HIP(hipGetLastError());
  if (tracing && (rc = print_memo_trace(e, pl, d_trace, TS, st))) return rc;
  if (profile && (rc = print_memo_profile(e, pl, Rg, max_ev, st))) return rc;
  return KSIM_OK;
}

// The initial keys, L1 maxima and feasible counts of k_hmemo's plan (k_hinit_gk, k_hinit_keys); roff: a
// node-sharded engine's first global rank.
static int hmemo_init_keys(ksim_engine* e, int Rg, int first, hipStream_t st, int roff) {
  using namespace ksim_hmemo;
  const HPlan& pl = e->hmemo.plan;
  HInitArgs ia;
  ia.roff = roff;
  ia.reps = e->d_reps.p;
  ia.rep_list = e->d_replist.p + first;
  ia.N = e->N;
  ia.Npad = pl.Npad;
  ia.nb = pl.nb;
  ia.Cmax = pl.Cmax;
  ia.Gmax = pl.Gmax;
  ia.Smax = pl.Smax;
  ia.cg = e->hmemo.cg.p;
  ia.cls = e->hmemo.cls.p;
  ia.cgrp = e->hmemo.cgrp.p;
  ia.gpod = e->hmemo.gpod.p;
  ia.st = e->hmemo.st.p;
  ia.ns = e->hmemo.ns.p;
  ia.nstate = e->hmemo.nstate.p;
  ia.gsc = e->hmemo.gsc.p;
  ia.keys = e->hmemo.keys.p;
  ia.l1 = e->hmemo.l1.p;
  ia.l2 = pl.l2 ? e->hmemo.l2.p : nullptr;
  ia.cnt = e->hmemo.cnt.p;
  ia.th = e->d_th.p;
  ia.mtoff = pl.Mtab > 0 ? e->hmemo.mtoff.p : nullptr;
  ia.na = pl.Mtab > 0 ? e->hmemo.na.p : nullptr;
  ia.Mslots = pl.Mslots;
  if (pl.Mtab > 0) {
    hipLaunchKernelGGL(k_hinit_na, dim3((unsigned)((kNaStride + 255) / 256), (unsigned)pl.Mslots, (unsigned)Rg), dim3(256), 0,
                       st, ia, (const TypDev*)e->d_tp.p);
    KSIM_HIP(hipGetLastError());
  }
  KSIM_HIP(hipMemsetAsync(e->hmemo.cnt.p, 0, sizeof(int) * (size_t)Rg * pl.Cmax, st));
  hipLaunchKernelGGL(k_hinit_gk, dim3((unsigned)((pl.Smax + 255) / 256), (unsigned)pl.Gmax, (unsigned)Rg), dim3(256), 0,
                     st, ia, (const TypDev*)e->d_tp.p);
  KSIM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_hinit_keys, dim3((unsigned)((pl.Npad + 255) / 256), (unsigned)pl.Cmax, (unsigned)Rg), dim3(256), 0,
                     st, ia);
  KSIM_HIP(hipGetLastError());
  return KSIM_OK;
}

static bool dead_skip(const ksim_engine* e, const RunEnv& env, const std::vector<int>& reps);

// k_hmemo's arguments for the planned launch (one group of Rg replicas from d_replist + first).
static ksim_hmemo::HMemoArgs hmemo_args(ksim_engine* e, const RunEnv& env, int first, int stride) {
  using namespace ksim_hmemo;
  const HPlan& pl = e->hmemo.plan;
  HMemoArgs ma;
  std::memset(&ma, 0, sizeof ma);  // every field a caller does not set (the gate, profile, exchange pointers) is null
  ma.reps = e->d_reps.p;
  ma.rep_list = e->d_replist.p + first;
  ma.Mtab = pl.Mtab;
  ma.Mslots = pl.Mslots;
  ma.mtoff = pl.Mtab > 0 ? e->hmemo.mtoff.p : nullptr;
  ma.mtab = pl.Mtab > 0 ? e->hmemo.mtab.p : nullptr;
  ma.na = pl.Mtab > 0 ? e->hmemo.na.p : nullptr;
  ma.N = e->N;
  ma.Npad = pl.Npad;
  ma.nb = pl.nb;
  ma.Cmax = pl.Cmax;
  ma.Gmax = pl.Gmax;
  ma.cg = e->hmemo.cg.p;
  ma.cls = e->hmemo.cls.p;
  ma.cgrp = e->hmemo.cgrp.p;
  ma.gpod = e->hmemo.gpod.p;
  ma.evc = e->hmemo.evc.p;
  ma.stride = stride;
  ma.keys = e->hmemo.keys.p;
  ma.l1 = e->hmemo.l1.p;
  ma.l2 = pl.l2 ? e->hmemo.l2.p : nullptr;
  ma.cnt0 = e->hmemo.cnt.p;
  ma.th = e->d_th.p;
  ma.prof = nullptr;
  ma.K = pl.K;
  ma.S = pl.S;
  ma.nbw = pl.nbw;
  ma.gran = e->d_gran.p;
  ma.fail = e->d_fail.p;
  ma.hist = nullptr;
  ma.roff = 0;
  ma.wbase = 0;
  ma.Ktot = pl.K;
  ma.tp = e->d_tp.p;
  ma.npeer = 0;
  ma.epoch = 0;
  {
    std::vector<int> all(e->R);
    std::iota(all.begin(), all.end(), 0);
    ma.skip = dead_skip(e, env, all) ? 1 : 0;
  }
  ma.pf = env.hpf;
  ma.delay = env.hdelay;
  ma.prune_t = env.hprune;
  for (int q = 0; q < kMaxPeers; ++q) ma.peer[q] = nullptr;
  return ma;
}

// KSIM_PROFILE=1: the phase table of the k_hmemo launch just enqueued (hmemo.prof).
static int print_hmemo_profile(ksim_engine* e, const HPlan& pl, int Rg, int max_ev, hipStream_t st) {
  using namespace ksim_hmemo;
  // per workgroup phase sums; refresh phases 0-4 run on one workgroup per step (the owner of the
  // changed node), so they are summed over a replica's workgroups, phase 5 is averaged over them
  KSIM_HIP(hipStreamSynchronize(st));
  const int nwg = Rg * pl.K;
  std::vector<unsigned long long> h((size_t)nwg * kHProf);
  KSIM_HIP(hipMemcpy(h.data(), e->hmemo.prof.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
  // waves 1-15 (the bulk: every class but the event's own): 0 + 2 on the F waves, 4 on the class
  // waves beside them, then 3; wave 0: 1 (the own class's refresh, the critical path), 5 (the rest of
  // its step: decide + Bind, then the end-of-step barrier)
  static const char* names[] = {"bulk: list (wave 1)", "critical own-class refresh", "bulk: F (F waves)",
                                 "bulk: join + class update", "class waves: class pass + flagged blocks",
                                 "wave 0 decide+bind+wait"};
  std::fprintf(stderr, "ksim hmemo profile: %d replicas x K=%d (S %d), LDS %zu B, Cmax %d Gmax %d Smax %d; us/step mean [max]:",
               Rg, pl.K, pl.S, pl.lds, pl.Cmax, pl.Gmax, pl.Smax);
  const double steps = std::max(max_ev, 1);
  for (int ph = 0; ph < 6; ++ph) {
    double sum = 0, mx = 0;
    for (int g = 0; g < Rg; ++g) {
      double us = 0;
      for (int k = 0; k < pl.K; ++k) us += (double)h[((size_t)g * pl.K + k) * kHProf + ph] / 100.0 / steps;
      if (ph == 5) us /= pl.K;
      sum += us;
      mx = std::max(mx, us);
    }
    std::fprintf(stderr, " %s %.3f [%.3f];", names[ph], sum / Rg, mx);
  }
  double it = 0, fl = 0, rs = 0, cyc = 0, tick = 0;
  for (int b = 0; b < nwg; ++b) {
    it += (double)h[(size_t)b * kHProf + 7];
    fl += (double)h[(size_t)b * kHProf + 8];
    rs += (double)h[(size_t)b * kHProf + 9];
    cyc += (double)h[(size_t)b * kHProf + 10];
    tick += (double)h[(size_t)b * kHProf + 11];
  }
  if (rs > 0) std::fprintf(stderr, " F items/refresh %.1f, flagged classes/refresh %.1f;", it / rs, fl / rs);
  if (tick > 0) std::fprintf(stderr, " shader clock %.0f MHz, wall %.3f ms", cyc / tick * 100.0, tick / nwg / 1e5);
  std::fprintf(stderr, "\n");
  return KSIM_OK;
}

// started: the residency gate's flags (K = 1 only); *gated tells the caller whether the launch carries them --
// not when its Rg workgroups cannot all be resident at once (a gate that could never open)
static int launch_hmemo(ksim_engine* e, const RunEnv& env, int Rg, int first, int max_ev, hipStream_t st,
                        int* started = nullptr, int gate_epoch = 0, bool* gated = nullptr) {
  using namespace ksim_hmemo;
  const HPlan& pl = e->hmemo.plan;
  const int stride = std::max(max_ev, 1);
  int irc = hmemo_init_keys(e, Rg, first, st, 0);
  if (irc) return irc;
  HMemoArgs ma = hmemo_args(e, env, first, stride);
  ma.started = pl.K == 1 ? started : nullptr;
  ma.gate_epoch = gate_epoch;
  if (gated) *gated = false;
  bool any_delete = false;
  for (const int r : e->hmemo.reps) any_delete = any_delete || e->has_delete[r];  // the FGD replicas
  if (pl.K > 1) {
    if (any_delete) {
      int rc = e->hmemo.hist.ensure((size_t)Rg * pl.K * stride);
      if (rc) return rc;
      ma.hist = e->hmemo.hist.p;
    }
    KSIM_HIP(hipMemsetAsync(e->d_gran.p, 0, sizeof(unsigned long long) * (size_t)Rg * 2 * pl.K * 2, st));
  }
  const bool profile = env.timers();
  if (profile) {
    int rc = e->hmemo.prof.ensure((size_t)Rg * pl.K * kHProf);
    if (rc) return rc;
    KSIM_HIP(hipMemsetAsync(e->hmemo.prof.p, 0, sizeof(unsigned long long) * (size_t)Rg * pl.K * kHProf, st));
    ma.prof = e->hmemo.prof.p;
  }
  // the large-table instantiations (per-model tables of typed replicas, the F-list pruning) when a replica of
  // the launch has use for them
  bool model = pl.Mtab > 0;
  for (const int r : e->hmemo.reps) model = model || e->reps[r].nt > ma.prune_t;  // the FGD replicas
  const void* f = hmemo_kernel(hmemo_form(kHLocal, pl.K, profile, ma.delay, model));
  if (pl.K > 1 && Rg * pl.K > resident_cap(e, f, pl.lds)) {
    std::fprintf(stderr, "ksim: k_hmemo needs %d co-resident workgroups\n", Rg * pl.K);
    return KSIM_ERANGE;
  }
  if (ma.started && Rg > resident_cap(e, f, pl.lds)) ma.started = nullptr;
  if (gated) *gated = ma.started != nullptr;
  const TypDev* tpp = e->d_tp.p;
  const int lrc = launch_persistent(f, Rg * pl.K, kHBlock, pl.lds, st, e->coop && pl.K > 1, ma, tpp);
  if (lrc) return lrc;
  hipLaunchKernelGGL(ksim_memo::k_memo_finish, dim3((unsigned)((stride + 255) / 256), (unsigned)Rg), dim3(256), 0, st,
                     e->d_reps.p, (const int*)(e->d_replist.p + first), e->N);
  KSIM_HIP(hipGetLastError());
  if (profile) return print_hmemo_profile(e, pl, Rg, max_ev, st);
  return KSIM_OK;
}

extern "C" {

const char* ksim_strerror(int code) {
  switch (code) {
    case KSIM_OK: return "ok";
    case KSIM_EINVAL: return "invalid argument";
    case KSIM_ENOMEM: return "out of memory";
    case KSIM_EHIP: return "HIP runtime error";
    case KSIM_ERANGE: return "value outside engine encoding";
    case KSIM_ESTATE: return "call out of order";
    case KSIM_ENOTSUP: return "not supported";
    case KSIM_ENODEV: return "no gfx950 device";
    case KSIM_EIO: return "trace I/O error";
    case KSIM_EPEER: return "peer shard's device not reachable from this one";
    default: return "unknown error";
  }
}

int ksim_abi_version(void) { return KSIM_ABI_VERSION; }

#ifndef KSIM_SOURCE_HASH
#define KSIM_SOURCE_HASH "unknown"
#endif
const char* ksim_build_id(void) { return KSIM_SOURCE_HASH; }

int ksim_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int c = 0;
  for (int i = 0; i < n; ++i)
    if (check_gfx950(i) == KSIM_OK) ++c;
  return c;
}

// ksim_engine_create, step 1: the configuration, the device's properties and the process's knobs.
static int read_config(ksim_engine* e, const ksim_config* cfg, int dev, int n_nodes, int n_replicas) {
  e->device = dev;
  e->N = n_nodes;
  e->R = n_replicas;
  if (cfg && cfg->nodes_per_block > 0) e->NB = std::min(cfg->nodes_per_block, kNBMax);
  if (cfg && cfg->steps_per_graph > 0) e->K = cfg->steps_per_graph;
  if (cfg) e->run_mode = cfg->run_mode, e->wgs_req = cfg->wgs_per_replica;
  hipDeviceProp_t prop;
  KSIM_HIP(hipGetDeviceProperties(&prop, dev));
  e->cus = prop.multiProcessorCount;
  // KSIM_CUS: use at most this many CUs for co-resident persistent grids (a device shared with
  // another process; also the tests' way to exercise the residency checks)
  if (const char* c = std::getenv("KSIM_CUS")) e->cus = std::max(1, std::min(e->cus, std::atoi(c)));
  // KSIM_COOP=0: launch K > 1 grids with hipLaunchKernel (the grid is still capped by resident_cap);
  // the profiler passes of scripts/profile_config.sh use it -- rocprofv3 7.2 faults at process exit
  // after a cooperative launch
  if (const char* c = std::getenv("KSIM_COOP")) e->coop = std::atoi(c) != 0;
  // KSIM_VARIANT scan1: single-workgroup cheap-policy groups on k_scan1 with the records in VGPRs (2, default),
  // in LDS (1), or on k_replay (0) -- A/B switches
  e->scan1 = (int)variant("scan1", 2);
  e->bpr = (n_nodes + e->NB - 1) / e->NB;
  e->tags_stride = (size_t)n_nodes * kTagStride + (size_t)n_nodes * 2;  // + int rank2idx[N]
  return KSIM_OK;
}

// Step 2: the stream, the timing events and the buffers whose size the node and replica counts fix, by size; the
// cluster state, the capacities and the power model start zeroed.
static int alloc_fixed(ksim_engine* e) {
  const size_t n = (size_t)e->N, r = (size_t)e->R, nr = n * r, tags = e->tags_stride * r;
  int rc = e->stream.ensure();  // after the first failure the rest does nothing
  const auto alloc = [&](size_t count, auto&... buf) { ((rc = rc ? rc : buf.alloc(count)), ...); };
  const auto zero = [&](auto&... buf) { ((rc = rc ? rc : buf.zero(e->stream)), ...); };
  alloc(nr, e->d_nodes, e->d_nodes_init, e->d_cap, e->d_mcap, e->d_last, e->d_cpum, e->d_pws);
  alloc(tags, e->d_tags, e->d_tags_init);
  alloc(r, e->d_acc, e->d_reps, e->d_replist, e->d_pw);
  alloc(n, e->d_feas, e->d_score, e->d_gpu);
  alloc(4, e->d_base, e->d_scratch);
  alloc(1, e->d_pod, e->d_res1, e->d_fail);
  alloc(kMaxTypical * r, e->d_tp);
  alloc(r * 2 * ksim_replay::kMaxK * ksim_replay::kGranW, e->d_gran);
  zero(e->d_nodes, e->d_nodes_init, e->d_tags, e->d_tags_init, e->d_cap, e->d_mcap, e->d_pw, e->d_cpum);
  for (DevEvent* ev : {&e->ev0, &e->ev1, &e->ev_mid}) rc = rc ? rc : ev->ensure();
  return rc;
}

// Step 3: the per-replica host state, each replica's view of the buffers, and the empty accumulators.
static int init_replicas(ksim_engine* e) {
  const int R = e->R;
  const size_t n = (size_t)e->N;
  const auto per_replica = [R](auto&... v) { (v.resize(R), ...); };  // empty buffers, zero counts
  per_replica(e->reps, e->h_nodes, e->h_rec, e->h_cls, e->h_tp, e->h_cls_n, e->h_ev_cls, e->go_state, e->d_ev, e->d_res,
              e->d_snap, e->d_prev, e->d_rep, e->n_events, e->has_delete, e->n_create, e->wgs_hint, e->nt, e->total_gpus, e->pw_set,
              e->wsum_w, e->wsum_set);
  for (int r = 0; r < R; ++r) {
    ReplicaDev& rp = e->reps[r];
    std::memset(&rp, 0, sizeof rp);
    rp.policy = POL_FGD;
    rp.gpusel = SEL_FGD;
    rp.tp = e->d_tp.p + (size_t)r * kMaxTypical;
    rp.nodes = e->d_nodes.p + r * n;
    rp.n_local = e->N;
    rp.tags = e->d_tags.p + r * e->tags_stride;
    rp.cap = e->d_cap.p + r * n;
    rp.mcap = e->d_mcap.p + r * n;
    rp.init = e->d_nodes_init.p + r * n;
    rp.last = e->d_last.p + r * n;
    rp.pw = e->d_pw.p + r;
    rp.cpum = e->d_cpum.p + r * n;
    rp.pws = e->d_pws.p + r * n;
    rp.w_pwr = 1000;
  }
  Accum none;
  std::memset(&none, 0, sizeof none);
  none.lo = 0x7fffffff, none.hi = -1;
  const std::vector<Accum> acc(R, none);
  int rc = e->d_acc.upload(acc, e->stream);
  if (!rc) rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));  // `acc` is pageable
  return KSIM_OK;
}

// All or nothing: the engine is handed out only when every step succeeded; a failing step destroys it with
// whatever the steps before it made.
int ksim_engine_create(const ksim_config* cfg, int n_nodes, int n_replicas, ksim_engine** out) {
  if (!out || n_nodes <= 0 || n_replicas <= 0) return KSIM_EINVAL;
  *out = nullptr;
  if (n_nodes > kMaxRank) return KSIM_ERANGE;  // name ranks are 24-bit fields of the argmax key
  if (cfg && (cfg->run_mode < 0 || cfg->run_mode > 5)) return KSIM_EINVAL;
  const int dev = cfg ? cfg->device : 0;
  int rc = check_gfx950(dev);
  if (rc) return rc;
  KSIM_HIP(hipSetDevice(dev));
  auto e = std::make_unique<ksim_engine>();
  if ((rc = read_config(e.get(), cfg, dev, n_nodes, n_replicas))) return rc;
  if ((rc = alloc_fixed(e.get()))) return rc;
  if ((rc = init_replicas(e.get()))) return rc;
  *out = e.release();
  return KSIM_OK;
}

ksim_engine::~ksim_engine() {
  (void)hipSetDevice(device);
  for (DevStream& s : side)
    if (s) (void)hipStreamSynchronize(s);
  if (stream) (void)hipStreamSynchronize(stream);
  graph.reset();
}

void ksim_engine_destroy(ksim_engine* e) { if (e) delete e; }

int ksim_engine_set_nodes(ksim_engine* e, int replica, const ksim_node* nodes) {
  if (!e || !nodes || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  std::vector<NodeRec> h(e->N);
  std::vector<int32_t> cap(e->N), mcap(e->N);
  std::vector<uint8_t> cpum(e->N);
  int64_t gpus = 0;
  std::vector<uint16_t> tags(e->tags_stride, 0);
  int* rank2idx = reinterpret_cast<int*>(tags.data() + (size_t)e->N * kTagStride);
  std::vector<char> seen(e->N, 0);
  for (int i = 0; i < e->N; ++i) {
    const ksim_node& s = nodes[i];
    if (s.gpu_count < 0 || s.gpu_count > kMaxGpu || s.gpu_type < 0 || s.gpu_type >= KSIM_MAX_TYPES)
      return KSIM_ERANGE;
    // sharded cluster: ranks are global and shard-contiguous (local node i has rank node_off + i)
    if (e->shard.on() && s.name_rank != (uint32_t)(e->shard.node_off + i)) return KSIM_EINVAL;
    const uint32_t lr = s.name_rank - (uint32_t)e->shard.node_off;
    if (lr >= (uint32_t)e->N || seen[lr]) return KSIM_EINVAL;
    if (s.cpu_alloc_milli < 0 || s.cpu_alloc_milli > 0x3fffffff) return KSIM_ERANGE;
    cap[i] = (int32_t)s.cpu_alloc_milli;
    if (s.mem_alloc_mib < 0 || s.mem_alloc_mib > 0x3fffffff) return KSIM_ERANGE;
    mcap[i] = (int32_t)s.mem_alloc_mib;
    if (s.cpu_model < 0 || s.cpu_model >= kMaxCpuModels) return KSIM_ERANGE;
    cpum[i] = (uint8_t)s.cpu_model;
    gpus += s.gpu_count;
    seen[lr] = 1;
    const int64_t cpu_left = s.cpu_alloc_milli - s.cpu_used_milli;
    const int64_t mem_left = s.mem_alloc_mib - s.mem_used_mib;
    const int64_t pods_left = (int64_t)s.pods_alloc - s.pods_used;
    if (cpu_left < -0x3fffffff || cpu_left > 0x3fffffff || mem_left < -0x3fffffff || mem_left > 0x3fffffff ||
        pods_left > 32767 || pods_left < -32768)
      return KSIM_ERANGE;
    NodeRec& n = h[i];
    std::memset(&n, 0, sizeof n);
    n.cpu_left = (int32_t)cpu_left;
    n.mem_left = (int32_t)mem_left;
    n.pods_left = (int16_t)pods_left;
    n.gpu_cnt = (uint8_t)s.gpu_count;
    n.gpu_type = (uint8_t)s.gpu_type;
    n.name_rank = s.name_rank;
    for (int g = 0; g < kMaxGpu; ++g) {
      const int left = g < s.gpu_count ? kMilli - s.gpu_used_milli[g] : 0;
      if (left < 0 || left > kMilli) return KSIM_ERANGE;
      n.gl[g] = (uint16_t)left;
    }
    for (int k = 0; k < kNumTags; ++k) tags[(size_t)i * kTagStride + k] = (uint16_t)s.tag_count[k];
    rank2idx[lr] = i;
  }
  e->h_nodes[replica].assign(nodes, nodes + e->N);
  e->h_rec[replica] = h;
  e->mplan_dirty = true;  // k_hmemo's plan holds the distinct initial node states
  e->ran = false;
  e->ds.invalidate();
  e->total_gpus[replica] = gpus;
  KSIM_HIP(hipSetDevice(e->device));
  KSIM_HIP(hipMemcpyAsync(e->d_cap.p + (size_t)replica * e->N, cap.data(), sizeof(int32_t) * e->N, hipMemcpyHostToDevice,
                          e->stream));
  KSIM_HIP(hipMemcpyAsync(e->d_mcap.p + (size_t)replica * e->N, mcap.data(), sizeof(int32_t) * e->N, hipMemcpyHostToDevice,
                          e->stream));
  KSIM_HIP(hipMemcpyAsync(e->d_cpum.p + (size_t)replica * e->N, cpum.data(), e->N, hipMemcpyHostToDevice, e->stream));
  KSIM_HIP(hipMemcpyAsync(e->reps[replica].nodes, h.data(), sizeof(NodeRec) * e->N, hipMemcpyHostToDevice, e->stream));
  KSIM_HIP(hipMemcpyAsync(e->d_tags.p + (size_t)replica * e->tags_stride, tags.data(), sizeof(uint16_t) * e->tags_stride,
                          hipMemcpyHostToDevice, e->stream));
  KSIM_HIP(hipMemcpyAsync(e->d_nodes_init.p + (size_t)replica * e->N, h.data(), sizeof(NodeRec) * e->N,
                          hipMemcpyHostToDevice, e->stream));
  KSIM_HIP(hipMemcpyAsync(e->d_tags_init.p + (size_t)replica * e->tags_stride, tags.data(),
                          sizeof(uint16_t) * e->tags_stride, hipMemcpyHostToDevice, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

int ksim_engine_set_typical(ksim_engine* e, int replica, const ksim_typical* tp, int n) {
  if (!e || replica < 0 || replica >= e->R || n < 0 || (n > 0 && !tp)) return KSIM_EINVAL;
  std::vector<TypDev> cpu, gpu;
  bool typed = false;
  for (int i = 0; i < n; ++i) {
    // frag.go:154-158: entries with freq outside [0,1] are skipped
    if (tp[i].freq < 0 || tp[i].freq > 1 || tp[i].freq != tp[i].freq) continue;
    if (tp[i].gpu_milli < 0 || tp[i].gpu_milli > 0x7fff || tp[i].cpu_milli > 0x3fffffff || tp[i].cpu_milli < -0x3fffffff)
      return KSIM_ERANGE;
    TypDev d;
    std::memset(&d, 0, sizeof d);
    d.cpu = (int32_t)tp[i].cpu_milli;
    d.milli = tp[i].gpu_milli;
    d.num_eff = std::max(tp[i].gpu_count, 1);
    d.tmask = tp[i].type_mask;
    d.freq = tp[i].freq;
    if (d.milli == 0) {
      cpu.push_back(d);  // XL/XR bins only (frag.go:463-469)
    } else {
      typed |= d.tmask != KSIM_TYPE_ANY;
      gpu.push_back(d);
    }
  }
  std::vector<TypDev> h(cpu);
  h.insert(h.end(), gpu.begin(), gpu.end());
  if ((int)h.size() > kMaxTypical) return KSIM_ERANGE;
  KSIM_HIP(hipSetDevice(e->device));
  if (!h.empty())
    KSIM_HIP(hipMemcpyAsync(e->d_tp.p + (size_t)replica * kMaxTypical, h.data(), sizeof(TypDev) * h.size(),
                            hipMemcpyHostToDevice, e->stream));
  e->reps[replica].nt = (int)h.size();
  e->reps[replica].ncpu = (int)cpu.size();
  e->reps[replica].typed = typed ? 1 : 0;
  e->h_tp[replica] = h;
  e->mplan_dirty = true;  // k_hmemo's plan holds per-model views of the table
  e->ran = false;
  e->ds.invalidate();
  int rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

int ksim_engine_set_policy(ksim_engine* e, int replica, int policy, int gpusel, uint64_t seed) {
  if (e) e->mplan_dirty = true;
  if (!e || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  if (policy < POL_FGD || policy > POL_WEIGHTED || gpusel < SEL_BEST || gpusel > SEL_DOTPROD) return KSIM_ENOTSUP;
  // allocateGpuIdFunc only holds the selectors of the enabled plugins (fgd_score.go:37, pwr_score.go:40,
  // dot_product_score.go:37).  POL_WEIGHTED: which plugins are enabled is known with the weights
  // (ksim_engine_set_plugin_weights checks the selector, and ksim_engine_run again)
  if (policy != POL_WEIGHTED && gpusel == SEL_PWR && !is_pwr_policy(policy)) return KSIM_ENOTSUP;
  if (policy != POL_WEIGHTED && gpusel == SEL_DOTPROD && policy != POL_DOTPROD) return KSIM_ENOTSUP;
  if (policy == POL_WEIGHTED && e->reps[replica].policy != POL_WEIGHTED) e->wsum_set[replica] = 0;
  if (policy == POL_PWR_FGD && e->reps[replica].policy != POL_PWR_FGD) {
    e->reps[replica].w_pwr = 500;  // "PWR 500 FGD 500" (generate_run_scripts.py:40) until set_weights
    e->reps[replica].w_fgd = 500;
  } else if (policy == POL_PWR) {
    e->reps[replica].w_pwr = 1000;
    e->reps[replica].w_fgd = 0;
  }
  e->reps[replica].policy = policy;
  e->reps[replica].gpusel = gpusel;
  e->reps[replica].seed = seed;
  KSIM_HIP(hipSetDevice(e->device));
  int rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

int ksim_engine_set_replica_wgs(ksim_engine* e, int replica, int wgs) {
  if (!e || replica < 0 || replica >= e->R || wgs < 0 || wgs > 64) return KSIM_EINVAL;
  e->wgs_hint[replica] = wgs;
  e->mplan_dirty = true;
  return KSIM_OK;
}

int ksim_engine_set_plugin_cfg(ksim_engine* e, int replica, int dim_ext, int norm) {
  if (!e || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  if (dim_ext < DIM_MERGE || dim_ext > DIM_EXTEND || norm < NORM_MAX || norm > NORM_POD) return KSIM_ENOTSUP;
  e->reps[replica].dpcfg = dim_ext | norm << 4;
  KSIM_HIP(hipSetDevice(e->device));
  int rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

int ksim_engine_set_go_stream(ksim_engine* e, int replica, const uint64_t* vec, int tap, int feed) {
  if (!e || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  if (!vec) {
    e->go_state[replica].clear();
    return KSIM_OK;
  }
  if (tap < 0 || tap >= ksim_random_go::kLen || feed < 0 || feed >= ksim_random_go::kLen) return KSIM_EINVAL;
  std::vector<unsigned long long>& s = e->go_state[replica];
  s.assign(vec, vec + ksim_random_go::kLen);
  s.push_back((unsigned long long)tap);
  s.push_back((unsigned long long)feed);
  return KSIM_OK;
}

// Replicas replaying the Random draw structure on Go's stream (k_random_go): policy Random with a
// source state set.
static bool go_random(const ksim_engine* e, int r) {
  return e->reps[r].policy == POL_RANDOM && !e->go_state[r].empty();
}

int ksim_engine_set_weights(ksim_engine* e, int replica, int32_t w_pwr, int32_t w_fgd) {
  if (!e || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  if (e->reps[replica].policy != POL_PWR_FGD) return KSIM_ESTATE;
  // framework weights are positive; the packed key holds w_pwr * 100 + w_fgd * 100 in 24 bits
  if (w_pwr <= 0 || w_fgd <= 0 || w_pwr > 50000 || w_fgd > 50000) return KSIM_ERANGE;
  e->reps[replica].w_pwr = w_pwr;
  e->reps[replica].w_fgd = w_fgd;
  KSIM_HIP(hipSetDevice(e->device));
  int rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

// The selector of a POL_WEIGHTED replica against its weights: allocateGpuIdFunc holds only the enabled plugins'
// selectors (fgd_score.go:37, pwr_score.go:40, dot_product_score.go:37).
static bool wsum_selector_ok(int gpusel, const int32_t* w) {
  if (gpusel == SEL_FGD) return w[POL_FGD] > 0;
  if (gpusel == SEL_PWR) return w[POL_PWR] > 0;
  if (gpusel == SEL_DOTPROD) return w[POL_DOTPROD] > 0;
  return true;
}

int ksim_engine_set_plugin_weights(ksim_engine* e, int replica, const int32_t* w) {
  static_assert(KSIM_NUM_PLUGINS == kNumPlugins && KSIM_POLICY_WEIGHTED == POL_WEIGHTED, "ksim_engine.h");
  if (!e || !w || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  if (e->reps[replica].policy != POL_WEIGHTED) return KSIM_ESTATE;
  // framework weights are positive; the packed key holds the total, at most 100 * sum(w), in 24 bits
  long long sum = 0;
  for (int p = 0; p < kNumPlugins; ++p) {
    if (w[p] < 0) return KSIM_ERANGE;
    sum += w[p];
  }
  if (sum <= 0 || 100 * sum >= (1ll << 24)) return KSIM_ERANGE;
  if (w[POL_RANDOM] > 0) return KSIM_ENOTSUP;  // RandomScore's PreScore pick is not reproducible
  if (!wsum_selector_ok(e->reps[replica].gpusel, w)) return KSIM_ENOTSUP;
  std::copy(w, w + kNumPlugins, e->wsum_w[replica].begin());
  e->wsum_w[replica][kNumPlugins] = (int32_t)ksim_plan::wsum::plugin_mask(w);
  e->wsum_set[replica] = 1;
  return KSIM_OK;
}

int ksim_engine_set_power_model(ksim_engine* e, int replica, const ksim_power_model* pm) {
  static_assert(sizeof(ksim_power_model) == sizeof(PowerDev), "ksim_power_model layout");
  if (!e || !pm || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  for (int c = 0; c < kMaxCpuModels; ++c)
    if (((pm->cpu_valid >> c) & 1u) && !(pm->cpu_cores[c] > 0)) return KSIM_ERANGE;
  KSIM_HIP(hipSetDevice(e->device));
  KSIM_HIP(hipMemcpyAsync(e->d_pw.p + replica, pm, sizeof(PowerDev), hipMemcpyHostToDevice, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  e->pw_set[replica] = 1;
  e->reps[replica].has_pw = 1;
  int rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

static bool any_pwr(const ksim_engine* e) {
  for (int r = 0; r < e->R; ++r)
    if (is_pwr_policy(e->reps[r].policy)) return true;
  return false;
}

static StepArgs base_args(ksim_engine* e) {
  StepArgs a;
  std::memset(&a, 0, sizeof a);
  a.reps = e->d_reps.p;
  a.acc = e->d_acc.p;
  a.N = e->N;
  a.NB = e->NB;
  a.bpr = e->bpr;
  return a;
}

int ksim_engine_filter_score(ksim_engine* e, int replica, const ksim_pod* pod, int32_t step, uint8_t* feasible,
                             int32_t* score, int32_t* gpu_mask) {
  if (!e || !pod || replica < 0 || replica >= e->R || !feasible || !score || !gpu_mask) return KSIM_EINVAL;
  PodDev p;
  int rc = to_pod_dev(*pod, &p);
  if (rc) return rc;
  if (p.flags & kPodDelete) return KSIM_EINVAL;
  // one plugin's Score per call: a weighted combination has two (query PWR and FGD replicas)
  if (e->reps[replica].policy == POL_PWR_FGD || e->reps[replica].policy == POL_WEIGHTED) return KSIM_ENOTSUP;
  if (is_pwr_policy(e->reps[replica].policy) && !e->pw_set[replica]) return KSIM_ESTATE;
  KSIM_HIP(hipSetDevice(e->device));
  KSIM_HIP(hipMemcpyAsync(e->d_pod.p, &p, sizeof p, hipMemcpyHostToDevice, e->stream));
  StepArgs a = base_args(e);
  a.rep_first = replica;
  a.step_off = step;
  a.pod_override = e->d_pod.p;
  a.res_override = e->d_res1.p;
  a.mode = 1;
  a.out_feas = e->d_feas.p;
  a.out_score = e->d_score.p;
  a.out_gpu = e->d_gpu.p;
  hipLaunchKernelGGL(k_step, dim3(e->bpr), dim3(kBlock), 0, e->stream, a, (const TypDev*)e->d_tp.p);
  KSIM_HIP(hipGetLastError());
  KSIM_HIP(hipMemcpyAsync(feasible, e->d_feas.p, e->N, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipMemcpyAsync(score, e->d_score.p, sizeof(int32_t) * e->N, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipMemcpyAsync(gpu_mask, e->d_gpu.p, sizeof(int32_t) * e->N, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

int ksim_engine_schedule(ksim_engine* e, int replica, const ksim_pod* pod, int32_t step, ksim_result* out) {
  if (!e || !pod || !out || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  PodDev p;
  int rc = to_pod_dev(*pod, &p);
  if (rc) return rc;
  if (p.flags & kPodDelete) return KSIM_EINVAL;  // deletions go through ksim_engine_unreserve
  if (e->reps[replica].policy == POL_WEIGHTED) return KSIM_ENOTSUP;  // the weighted combinations: ksim_engine_run only
  KSIM_HIP(hipSetDevice(e->device));
  KSIM_HIP(hipMemcpyAsync(e->d_pod.p, &p, sizeof p, hipMemcpyHostToDevice, e->stream));
  StepArgs a = base_args(e);
  a.rep_first = replica;
  a.step_off = step;
  a.pod_override = e->d_pod.p;
  a.res_override = e->d_res1.p;
  a.mode = 0;
  if (is_pwr_policy(e->reps[replica].policy) && !e->pw_set[replica]) return KSIM_ESTATE;
  hipLaunchKernelGGL(k_step, dim3(e->bpr), dim3(kBlock), 0, e->stream, a, (const TypDev*)e->d_tp.p);
  if (is_pwr_policy(e->reps[replica].policy))
    hipLaunchKernelGGL(k_step_pwr<false>, dim3(e->bpr), dim3(kBlock), 0, e->stream, a);
  KSIM_HIP(hipGetLastError());
  ResultDev r;
  KSIM_HIP(hipMemcpyAsync(&r, e->d_res1.p, sizeof r, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  std::memcpy(out, &r, sizeof r);
  return KSIM_OK;
}

int ksim_engine_reserve(ksim_engine* e, int replica, const ksim_pod* pod, int node, int32_t step, int32_t* gpu_mask_out) {
  if (!e || !pod || !gpu_mask_out || replica < 0 || replica >= e->R || node < 0 || node >= e->N) return KSIM_EINVAL;
  PodDev p;
  int rc = to_pod_dev(*pod, &p);
  if (rc) return rc;
  if (e->reps[replica].policy == POL_WEIGHTED) return KSIM_ENOTSUP;  // the weighted combinations: ksim_engine_run only
  KSIM_HIP(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_reserve, dim3(1), dim3(64), 0, e->stream, e->d_reps.p, (const TypDev*)e->d_tp.p, replica, p, node, step, e->d_scratch.p, +1, -1);
  KSIM_HIP(hipGetLastError());
  int m = 0;
  KSIM_HIP(hipMemcpyAsync(&m, e->d_scratch.p, sizeof m, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  *gpu_mask_out = m;
  return m < 0 ? KSIM_ESTATE : KSIM_OK;
}

int ksim_engine_unreserve(ksim_engine* e, int replica, const ksim_pod* pod, int node, int32_t gpu_mask) {
  if (!e || !pod || replica < 0 || replica >= e->R || node < 0 || node >= e->N) return KSIM_EINVAL;
  PodDev p;
  int rc = to_pod_dev(*pod, &p);
  if (rc) return rc;
  if (p.flags & kPodDelete) return KSIM_EINVAL;
  // the devices a Reserve of this pod can have assigned on this node (open_gpu_share.go:242-283): none
  // for a pod without GPU milli, else `num` devices the node has
  if (e->h_nodes[replica].size() != (size_t)e->N) return KSIM_ESTATE;
  const int cnt = e->h_nodes[replica][node].gpu_count;
  if (gpu_mask < 0 || gpu_mask >= (1 << cnt)) return KSIM_EINVAL;
  if ((p.milli == 0) != (gpu_mask == 0)) return KSIM_EINVAL;
  if (p.milli > 0 && __builtin_popcount((unsigned)gpu_mask) != p.num) return KSIM_EINVAL;
  KSIM_HIP(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_reserve, dim3(1), dim3(64), 0, e->stream, e->d_reps.p, (const TypDev*)e->d_tp.p, replica, p, node, 0, e->d_scratch.p, -1,
                     (int)gpu_mask);
  KSIM_HIP(hipGetLastError());
  int m = 0;
  KSIM_HIP(hipMemcpyAsync(&m, e->d_scratch.p, sizeof m, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return m < 0 ? KSIM_ESTATE : KSIM_OK;  // the node does not hold what the pod would release
}

int ksim_engine_bind(ksim_engine* e, int replica, const ksim_pod* pod, int node, int32_t gpu_mask) {
  if (!e || !pod || replica < 0 || replica >= e->R || node < 0 || node >= e->N) return KSIM_EINVAL;
  PodDev p;
  int rc = to_pod_dev(*pod, &p);
  if (rc) return rc;
  if (p.flags & kPodDelete) return KSIM_EINVAL;
  if (e->h_nodes[replica].size() != (size_t)e->N) return KSIM_ESTATE;
  const int cnt = e->h_nodes[replica][node].gpu_count;
  if (gpu_mask < 0 || gpu_mask >= (1 << cnt)) return KSIM_EINVAL;
  if ((p.milli == 0) != (gpu_mask == 0)) return KSIM_EINVAL;
  if (p.milli > 0 && __builtin_popcount((unsigned)gpu_mask) != p.num) return KSIM_EINVAL;
  KSIM_HIP(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_reserve, dim3(1), dim3(64), 0, e->stream, e->d_reps.p, (const TypDev*)e->d_tp.p, replica, p, node, 0,
                     e->d_scratch.p, +1, (int)gpu_mask);
  KSIM_HIP(hipGetLastError());
  int m = 0;
  KSIM_HIP(hipMemcpyAsync(&m, e->d_scratch.p, sizeof m, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return m < 0 ? KSIM_ESTATE : KSIM_OK;  // a named device lacks the milli (the reference panics)
}

int ksim_engine_load_events(ksim_engine* e, int replica, const ksim_pod* events, int n) {
  if (e) e->mplan_dirty = true;
  if (!e || replica < 0 || replica >= e->R || n < 0 || (n > 0 && !events)) return KSIM_EINVAL;
  e->ran = false;
  e->ds.invalidate();
  std::vector<PodDev> h(n);
  std::vector<char> gone(std::max(n, 1), 0);  // creations already deleted (the reference deletes a pod once)
  for (int i = 0; i < n; ++i) {
    int rc = to_pod_dev(events[i], &h[i]);
    if (rc) return rc;
    if (h[i].flags & kPodDelete) {
      const int ref = h[i].ref;
      if (ref < 0 || ref >= i || (h[ref].flags & kPodDelete) || gone[ref]) return KSIM_EINVAL;
      gone[ref] = 1;
    }
  }
  // pod classes for k_memo: the distinct Filter + Score requests of the creation events
  classify_events(h, e->h_cls[replica], e->h_cls_n[replica], e->h_ev_cls[replica]);
  KSIM_HIP(hipSetDevice(e->device));
  // the replica's buffers afresh: a failed alloc leaves its buffer empty, so the replica points at live memory or at
  // none, and has no events until both buffers are there
  const size_t ne = (size_t)std::max(n, 1);
  DevBuf<PodDev>& ev = e->d_ev[replica];
  DevBuf<ResultDev>& res = e->d_res[replica];
  int rc = ev.alloc(ne);
  if (!rc) rc = res.alloc(ne);
  if (!rc) rc = res.fill(0xff, e->stream);
  e->reps[replica].ev = ev.p;
  e->reps[replica].res = res.p;
  e->reps[replica].n_events = e->n_events[replica] = rc ? 0 : n;
  if (rc) return rc;
  if (n > 0) KSIM_HIP(hipMemcpyAsync(ev.p, h.data(), sizeof(PodDev) * n, hipMemcpyHostToDevice, e->stream));
  e->has_delete[replica] = false;
  for (int i = 0; i < n; ++i) e->has_delete[replica] = e->has_delete[replica] || events[i].is_delete;
  e->n_create[replica] = 0;
  for (int i = 0; i < n; ++i) e->n_create[replica] += events[i].is_delete ? 0 : 1;
  rc = alloc_report(e, replica);
  if (rc) return rc;
  rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

// Every replica back to the cluster state given to set_nodes (device-to-device).
static int reset_state(ksim_engine* e) {
  KSIM_HIP(hipMemcpyAsync(e->d_nodes.p, e->d_nodes_init.p, sizeof(NodeRec) * (size_t)e->N * e->R, hipMemcpyDeviceToDevice,
                          e->stream));
  KSIM_HIP(hipMemcpyAsync(e->d_tags.p, e->d_tags_init.p, sizeof(uint16_t) * e->tags_stride * e->R, hipMemcpyDeviceToDevice,
                          e->stream));
  return KSIM_OK;
}

// Per-event report buffers of one replica (allocated while the report is enabled).
static int alloc_report(ksim_engine* e, int r) {
  const bool on = e->report && e->d_ev[r].p;
  e->rep_ready = false;  // (new events or the report switched: the records are no run's)
  e->shard.group.rmerge_n = -1;
  const size_t ne = (size_t)std::max(e->n_events[r], 1);
  int rc = on ? e->d_snap[r].alloc(ne) : KSIM_OK;
  if (on && !rc) rc = e->d_prev[r].alloc(ne);
  if (on && !rc) rc = e->d_rep[r].alloc(ne);
  if (!on || rc) e->d_snap[r].release(), e->d_prev[r].release(), e->d_rep[r].release();  // all three or none
  e->reps[r].snap = e->d_snap[r].p;
  e->reps[r].prev = e->d_prev[r].p;
  e->reps[r].rep = e->d_rep[r].p;
  return rc;
}

// The per-event cluster report of every replica from the run's snapshots (ksim_report.hpp).
// list (device, nullable): only these R replicas -- one concurrent group's, on its own stream behind its replay.
static int run_report(ksim_engine* e, int max_ev, hipStream_t st, const int* list, int R) {
  if (max_ev <= 0 || R <= 0) return KSIM_OK;
  const dim3 grid((unsigned)((max_ev + ksim_rep::kDeltaBlock - 1) / ksim_rep::kDeltaBlock), (unsigned)R);
  hipLaunchKernelGGL(ksim_rep::k_report_delta, grid, dim3(ksim_rep::kDeltaBlock), 0, st,
                     (const ReplicaDev*)e->d_reps.p, (const TypDev*)e->d_tp.p, list,
                     (e->shard.world > 1 && e->shard.rank != 0) ? 0 : 1);  // a cluster's arrivals: shard rank 0 counts them
  KSIM_HIP(hipGetLastError());
  // the scan over B workgroups per replica when a few replicas would leave most CUs idle behind one workgroup's pass
  // (about a CU-full of workgroups, parts of >= 2048 events; KSIM_VARIANT report_parts=0: one workgroup each)
  const int B = variant("report_parts", 1) != 0
                    ? std::min({ksim_rep::kScanPartsMax, (e->cus + R - 1) / R, max_ev / 2048}) : 1;
  if (B > 1) {
    const int rc = e->d_ragg.ensure((size_t)e->R * ksim_rep::kScanPartsMax * 2 * ksim_rep::kFields);
    if (rc) return rc;
    hipLaunchKernelGGL(ksim_rep::k_report_part, dim3((unsigned)B, (unsigned)R), dim3(ksim_rep::kScanBlock), 0, st,
                       (const ReplicaDev*)e->d_reps.p, (const TypDev*)e->d_tp.p, e->N, list, e->d_ragg.p);
    KSIM_HIP(hipGetLastError());
    hipLaunchKernelGGL(ksim_rep::k_report_apply, dim3((unsigned)B, (unsigned)R), dim3(ksim_rep::kScanBlock), 0, st,
                       (const ReplicaDev*)e->d_reps.p, e->N, list, (const __int128*)e->d_ragg.p);
    KSIM_HIP(hipGetLastError());
    return KSIM_OK;
  }
  hipLaunchKernelGGL(ksim_rep::k_report_scan, dim3(R), dim3(ksim_rep::kScanBlock), 0, st,
                     (const ReplicaDev*)e->d_reps.p, (const TypDev*)e->d_tp.p, e->N, list);
  KSIM_HIP(hipGetLastError());
  return KSIM_OK;
}

// RCCL, loaded on first use (the node-sharded mode only): the library stays loadable without it.
struct RcclApi {
  ncclResult_t (*get_unique_id)(ncclUniqueId*);
  ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int);
  ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
  ncclResult_t (*comm_destroy)(ncclComm_t);
  const char* (*error_string)(ncclResult_t);
};
static RcclApi* rccl() {
  static RcclApi api;
  static int state = 0;  // 0 untried, 1 ok, -1 unavailable
  if (state == 0) {
    // the RCCL beside the HIP runtime this process bound (torch's or /opt/rocm's, ksim.hip_runtime_path):
    // an RCCL from another install would NEED its own runtime and take this library's streams across
    // runtimes; the bare names last (a RUNPATH / SONAME match)
    void* h = nullptr;
    Dl_info di;
    if (dladdr((const void*)(hipError_t(*)(void**, size_t))&hipMalloc, &di) && di.dli_fname) {
      std::string dir(di.dli_fname);
      dir = dir.substr(0, dir.find_last_of('/') + 1);
      for (const char* nm : {"librccl.so.1", "librccl.so"})
        if (!h) h = dlopen((dir + nm).c_str(), RTLD_NOW | RTLD_GLOBAL);
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    state = -1;
    if (h) {
      api.get_unique_id = (decltype(api.get_unique_id))dlsym(h, "ncclGetUniqueId");
      api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(h, "ncclCommInitRank");
      api.all_gather = (decltype(api.all_gather))dlsym(h, "ncclAllGather");
      api.comm_destroy = (decltype(api.comm_destroy))dlsym(h, "ncclCommDestroy");
      api.error_string = (decltype(api.error_string))dlsym(h, "ncclGetErrorString");
      if (api.get_unique_id && api.comm_init_rank && api.all_gather && api.comm_destroy && api.error_string) state = 1;
    }
  }
  return state == 1 ? &api : nullptr;
}

static hipError_t destroy_comm(ncclComm_t c) {  // ShardComm's destroyer
  if (rccl()) (void)rccl()->comm_destroy(c);
  return hipSuccess;
}

// One pod step of a sharded cluster, enqueued on `st`: local Filter+Score (k_step mode 2), the
// exchange of the shard records, the cluster-wide finish on every shard (owner binds).
static int shard_local(ksim_engine* e, hipStream_t st, const int* base, int step_off) {
  StepArgs a = base_args(e);
  a.base = base;
  a.step_off = step_off;
  a.mode = 2;
  a.send = e->shard.d_send.p;
  hipLaunchKernelGGL(k_step, dim3(e->bpr), dim3(kBlock), 0, st, a, (const TypDev*)e->d_tp.p);
  KSIM_HIP(hipGetLastError());
  return KSIM_OK;
}
// A PWR policy's second round: the shard's scores normalized with the cluster's raw range (gathered after
// shard_local), its best key to the exchange again.
static int shard_pwr(ksim_engine* e, hipStream_t st, const int* base, int step_off) {
  StepArgs a = base_args(e);
  a.base = base;
  a.step_off = step_off;
  a.mode = 2;
  a.send = e->shard.d_send.p;
  a.recv = e->shard.d_recv.p;
  a.world = e->shard.world;
  hipLaunchKernelGGL(k_step_pwr<true>, dim3(e->bpr), dim3(kBlock), 0, st, a);
  KSIM_HIP(hipGetLastError());
  return KSIM_OK;
}
static int shard_commit(ksim_engine* e, hipStream_t st, const int* base, int step_off) {
  StepArgs a = base_args(e);
  a.base = base;
  a.step_off = step_off;
  a.recv = e->shard.d_recv.p;
  a.world = e->shard.world;
  hipLaunchKernelGGL(k_shard_commit, dim3(1), dim3(64), 0, st, a);
  KSIM_HIP(hipGetLastError());
  return KSIM_OK;
}
static int shard_exchange(ksim_engine* e, hipStream_t st) {
  if (e->shard.exchanges_by_rccl()) {
    const ncclResult_t r = rccl()->all_gather(e->shard.d_send.p, e->shard.d_recv.p, 4, ncclUint64, e->shard.comm, st);
    if (r != ncclSuccess) {
      std::fprintf(stderr, "ksim: ncclAllGather failed: %s\n", rccl()->error_string(r));
      return KSIM_EHIP;
    }
    return KSIM_OK;
  }
  KSIM_HIP(hipMemcpyAsync(e->shard.d_recv.p, e->shard.d_send.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
  return KSIM_OK;
}

// Sharded run over RCCL (or a world of one): steps captured K at a time into a hipGraph when the
// stream capture accepts the collective, else enqueued eagerly.
static int run_sharded(ksim_engine* e, int max_ev) {
  int rc;
  ShardState& sh = e->shard;
  // a PWR policy takes two rounds per pod: the raw score range (k_step), then the keys under the cluster's range
  // (k_step_pwr); see DESIGN.md "PWR on shards"
  const bool pwr = any_pwr(e);
  if (sh.exchanges_on_host()) {  // the record goes through the caller's transport, one round at a time
    const size_t rec = 4 * sizeof(unsigned long long);
    auto round = [&]() -> int {
      KSIM_HIP(hipMemcpyAsync(sh.h_send.data(), sh.d_send.p, rec, hipMemcpyDeviceToHost, e->stream));
      KSIM_HIP(hipStreamSynchronize(e->stream));
      if (sh.xfn(sh.h_send.data(), sh.h_recv.data(), sh.xuser) != 0) return KSIM_ESTATE;
      // the caller's gather must hold this shard's own record at its rank
      if (std::memcmp(sh.h_recv.data() + 4 * (size_t)sh.rank, sh.h_send.data(), rec) != 0) return KSIM_ESTATE;
      KSIM_HIP(hipMemcpyAsync(sh.d_recv.p, sh.h_recv.data(), rec * (size_t)sh.world, hipMemcpyHostToDevice, e->stream));
      return KSIM_OK;
    };
    for (int s = 0; s < max_ev; ++s) {
      if ((rc = shard_local(e, e->stream, nullptr, s))) return rc;
      if (pwr && e->h_ev_cls[0][s] >= 0) {  // (a delete event has no scores to normalize: one round, as ever)
        if ((rc = round())) return rc;
        if ((rc = shard_pwr(e, e->stream, nullptr, s))) return rc;
      }
      if ((rc = round())) return rc;
      if ((rc = shard_commit(e, e->stream, nullptr, s))) return rc;
    }
    return KSIM_OK;
  }
  if (sh.needs_group_run()) return KSIM_ESTATE;  // in-process group: ksim_shard_group_run
  auto step = [&](const int* base, int i) {
    int r = shard_local(e, e->stream, base, i);
    if (!r && pwr && !(r = shard_exchange(e, e->stream))) r = shard_pwr(e, e->stream, base, i);
    if (!r && !(r = shard_exchange(e, e->stream))) r = shard_commit(e, e->stream, base, i);
    return r;
  };
  hipGraph_t g = nullptr;
  GraphExec ge;
  const int K = std::min(e->K, std::max(max_ev, 1));
  if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    bool ok = true;
    for (int i = 0; i < K && ok; ++i) ok = step(e->d_base.p, i) == KSIM_OK;
    if (ok) hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, e->stream, e->d_base.p, K);
    const hipError_t ce = hipStreamEndCapture(e->stream, &g);
    if (ok && ce == hipSuccess && hipGraphInstantiate(&ge.h, g, nullptr, nullptr, 0) != hipSuccess) ge.h = nullptr;
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
  }
  if (ge) {
    KSIM_HIP(hipMemsetAsync(e->d_base.p, 0, sizeof(int), e->stream));
    for (int s0 = 0; s0 < max_ev; s0 += K) {
      if (hipGraphLaunch(ge, e->stream) != hipSuccess) return KSIM_EHIP;
    }
    return KSIM_OK;
  }
  for (int s = 0; s < max_ev; ++s)
    if ((rc = step(nullptr, s))) return rc;
  return KSIM_OK;
}

static int build_graph(ksim_engine* e) {
  const bool pwr = any_pwr(e);
  if (e->graph && e->graph_R == e->R && e->graph_pwr == pwr) return KSIM_OK;
  e->graph.reset();
  hipGraph_t g;
  KSIM_HIP(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
  StepArgs a = base_args(e);
  a.rep_first = 0;
  a.base = e->d_base.p;
  for (int i = 0; i < e->K; ++i) {
    a.step_off = i;
    hipLaunchKernelGGL(k_step, dim3(e->bpr * e->R), dim3(kBlock), 0, e->stream, a, (const TypDev*)e->d_tp.p);
    if (pwr) hipLaunchKernelGGL(k_step_pwr<false>, dim3(e->bpr * e->R), dim3(kBlock), 0, e->stream, a);
  }
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, e->stream, e->d_base.p, e->K);
  KSIM_HIP(hipStreamEndCapture(e->stream, &g));
  KSIM_HIP(hipGraphInstantiate(&e->graph.h, g, nullptr, nullptr, 0));
  KSIM_HIP(hipGraphDestroy(g));
  e->graph_R = e->R;
  e->graph_pwr = pwr;
  return KSIM_OK;
}

// KSIM_PROFILE=1: per-phase k_replay time (us per step, mean and max over workgroups) on stderr.
static void print_replay_profile(ksim_engine* e, int R, int K, int steps) {
  const int nb = R * K, P = ksim_replay::kProfPhases;
  std::vector<unsigned long long> h((size_t)nb * P);
  if (hipMemcpy(h.data(), e->d_prof.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) != hipSuccess) return;
  static const char* names[] = {"pod", "filter(+emit)", "fgd-eval", "fgd-final", "agg-sync", "poll", "commit+publish", "end-sync"};
  std::fprintf(stderr, "ksim profile: %d workgroups (K=%d), %d steps, us/step mean [max]:", nb, K, steps);
  for (int ph = 0; ph < 8; ++ph) {
    double sum = 0, mx = 0;
    for (int b = 0; b < nb; ++b) {
      const double us = (double)h[(size_t)b * P + ph] / 100.0 / steps;  // 100 MHz ticks
      sum += us;
      mx = std::max(mx, us);
    }
    std::fprintf(stderr, " %s %.3f [%.3f];", names[ph], sum / nb, mx);
  }
  double spins = 0;
  for (int b = 0; b < nb; ++b) spins += (double)h[(size_t)b * P + 8];
  std::fprintf(stderr, " poll spins/step %.2f", spins / nb / steps);
  double miss = 0, redo = 0;  // PWR+FGD: guessed-range misses (every workgroup alike), re-evaluations
  for (int b = 0; b < nb; ++b) {
    miss += (double)(h[(size_t)b * P + 9] & 0xffffffffull);
    redo += (double)(h[(size_t)b * P + 9] >> 32);
  }
  if (miss + redo > 0) std::fprintf(stderr, " pf misses/step %.4f re-evaluations/step %.4f", miss / nb / steps, redo / nb / steps * K);
  double cyc = 0, tick = 0;
  for (int b = 0; b < nb; ++b) { cyc += (double)h[(size_t)b * P + 10]; tick += (double)h[(size_t)b * P + 11]; }
  if (tick > 0) std::fprintf(stderr, " shader clock %.0f MHz", cyc / tick * 100.0);
  std::fprintf(stderr, "\n");
}

static int resident_cap(const ksim_engine* e, const void* f, size_t lds) {
  (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 1024, lds) != hipSuccess) {
    (void)hipGetLastError();
    nb = 0;
  }
  return nb * e->cus;
}

// The dead-class skip (k_memo, k_hmemo, k_scan1): on create-only streams a class that once found no
// feasible node never finds one again (Filter is monotone in the resources a creation takes), so its
// later events are decided without a scan.  Needs every replica create-only with class ids < 1024;
// KSIM_VARIANT=skip=0 turns it off (A/B runs).
static bool dead_skip(const ksim_engine* e, const RunEnv& env, const std::vector<int>& reps) {
  if (!env.skip) return false;
  for (int r : reps)
    if (e->has_delete[r] || e->h_cls[r].size() > 1024) return false;
  return true;
}

// What the run planner (ksim_plan.hpp make_run_plan) reads of the engine, once prepare_memo has made the FGD plans.
static RunPlanInput run_plan_input(const ksim_engine* e, const RunEnv& env) {
  RunPlanInput in;
  for (int r = 0; r < e->R; ++r)
    in.reps.push_back({e->reps[r].policy, go_random(e, r), e->n_events[r], (bool)e->has_delete[r], e->reps[r].dpcfg,
                       e->reps[r].policy == POL_WEIGHTED ? (unsigned)e->wsum_w[r][kNumPlugins] : 0u});
  in.N = e->N;
  in.cus = e->cus;
  in.wgs_req = e->wgs_req;
  in.run_mode = e->run_mode;
  in.report = e->report;
  in.scan1 = e->scan1;
  in.split_fgd = e->split_fgd;
  in.memo_ok = e->memo.ok;
  in.memo_nwg = e->memo.plan.nwg;
  in.memo_reps = e->memo.reps;
  in.hmemo_ok = e->hmemo.ok;
  in.hmemo_K = e->hmemo.plan.K;
  in.hmemo_reps = e->hmemo.reps;
  in.timers = env.timers();
  in.scan1_mix = env.scan1_mix;
  in.side_streams = env.side_streams;
  return in;
}

static hipStream_t group_stream(const ksim_engine* e, const PlanGroup& g) { return g.side < 0 ? e->stream : e->side[g.side]; }

static std::vector<int> group_reps(const RunPlan& plan, const PlanGroup& g) {
  return std::vector<int>(plan.order.begin() + g.first, plan.order.begin() + g.first + g.count);
}

// ---- the launchers: one per kernel family ----
// The diagnostics of one replay launch (last_run_kernels, last_run_wgs, last_run_path): K <= 0 leaves the width,
// replicas (nullable) is the kernel's replica counter in e->stats.
static void note_launch(ksim_engine* e, const char* name, int K, int* replicas, int Rg) {
  note_kernel(e->stats, name);
  if (K > 0) e->stats.K = K;
  if (replicas) *replicas += Rg;
}

// The source states of the Random replicas on Go's stream, uploaded before anything of the run is enqueued.
static int upload_go_states(ksim_engine* e, const RunPlan& plan) {
  if (plan.groups.empty() || plan.groups.back().kind != kPolRandomGo) return KSIM_OK;
  const size_t words = (size_t)e->R * ksim_random_go::kStateWords;
  std::vector<unsigned long long> h(words, 0ull);
  for (int r = 0; r < e->R; ++r)
    if (go_random(e, r))
      std::copy(e->go_state[r].begin(), e->go_state[r].end(), h.begin() + (size_t)r * ksim_random_go::kStateWords);
  if (const int rc = e->d_go.upload(h, e->stream)) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));  // h is a local
  return KSIM_OK;
}

static int launch_random_go(ksim_engine* e, const PlanGroup& g, hipStream_t gs) {
  ksim_random_go::RandGoArgs ga{e->d_reps.p, e->d_replist.p + g.first, e->d_go.p, e->N};
  const bool in_lds = ksim_random_go::lds_bytes(e->N, true) <= kLdsMax;
  const size_t lds = ksim_random_go::lds_bytes(e->N, in_lds);
  if (in_lds) {
    KSIM_HIP(hipFuncSetAttribute((const void*)ksim_random_go::k_random_go<true>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ksim_random_go::k_random_go<true>, dim3(g.count), dim3(ksim_random_go::kBlock), lds, gs, ga);
  } else {
    hipLaunchKernelGGL(ksim_random_go::k_random_go<false>, dim3(g.count), dim3(ksim_random_go::kBlock), lds, gs, ga);
  }
  KSIM_HIP(hipGetLastError());
  note_launch(e, "k_random_go", 0, &e->stats.rgo, g.count);
  return KSIM_OK;
}

// The overlapped report (KSIM_VARIANT report_overlap=0 off): a cheap group with more replicas than the CUs the FGD
// groups leave can hold at once runs in waves of workgroups, so its last replicas end well after its first ones; its
// replicas then report one by one as each ends (k_report_overlap, behind the first group on that group's stream)
// instead of all after the last one.  Sets up the queue the replay feeds; *overlapped: the group gets that report.
static int overlap_queue(ksim_engine* e, const RunEnv& env, const RunPlan& plan, const PlanGroup& g, const void* f,
                         hipStream_t gs, ksim_scan1::Scan1Args& sa, bool* overlapped) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, ksim_scan1::kBlock, g.lds) != hipSuccess) {
    (void)hipGetLastError();
    nb = 0;
  }
  // (KSIM_TEST report_overlap=1: whatever the size, for the parity tests)
  if (!(nb > 0 && (g.count > std::max(0, e->cus - plan.fgd_cus) * nb || env.force_report_overlap))) return KSIM_OK;
  bool grew = false;
  const int rc = e->d_done.ensure(2 + (size_t)g.count, &grew);
  if (rc) return rc;
  if (grew) KSIM_HIP(hipMemset(e->d_done.p, 0, sizeof(unsigned long long) * (2 + (size_t)g.count)));
  if (int rc = e->ev_ovl.ensure(hipEventDisableTiming)) return rc;
  KSIM_HIP(hipMemsetAsync(e->d_done.p, 0, 2 * sizeof(unsigned long long), gs));  // tickets; entries keep epochs
  KSIM_HIP(hipEventRecord(e->ev_ovl, gs));
  *overlapped = true;
  e->stats.ovl += g.count;
  e->done_epoch = e->done_epoch % 0x7fffffffu + 1;
  sa.done = e->d_done.p;
  sa.epoch = e->done_epoch;
  return KSIM_OK;
}

// k_scan1 (one cheap policy) or k_scan1_mix (the policy per workgroup): one 256-thread workgroup per replica.
static int launch_scan1(ksim_engine* e, const RunEnv& env, const RunPlan& plan, int gi, hipStream_t gs, bool* overlapped) {
  using namespace ksim_scan1;
  const PlanGroup& g = plan.groups[gi];
  const bool mix = g.kind == kPolMix, reg = plan.reg1;
  const void* f = !mix ? scan1_fn(g.kind, e->report, reg)
                  : e->report ? (reg ? (const void*)k_scan1_mix<true, true> : (const void*)k_scan1_mix<true, false>)
                              : (reg ? (const void*)k_scan1_mix<false, true> : (const void*)k_scan1_mix<false, false>);
  if (!f) return KSIM_ENOTSUP;  // scan1_serves (the planner) names a policy scan1_fn has no instantiation for
  Scan1Args sa{e->d_reps.p, e->d_replist.p + g.first, e->N, dead_skip(e, env, group_reps(plan, g)) ? 1 : 0, nullptr, 0};
  KSIM_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
  if (mix && plan.concurrent && e->report && gi > 0 && env.report_overlap) {
    const int rc = overlap_queue(e, env, plan, g, f, gs, sa, overlapped);
    if (rc) return rc;
  }
  void* params[] = {(void*)&sa};
  KSIM_HIP(hipLaunchKernel(f, dim3(g.count), dim3(ksim_scan1::kBlock), params, g.lds, gs));
  note_launch(e, mix ? "k_scan1_mix" : "k_scan1", 1, &e->stats.scan1, g.count);
  return KSIM_OK;
}

// k_wsum (the weighted combinations): one 1024-thread workgroup per replica, the instantiation by what the group's
// plugin masks and the run need.  A cluster that does not fit one workgroup's LDS is refused.
// Its argument table (every replica's weights and plugin mask), uploaded before anything of the run is enqueued.
static int upload_wsum_weights(ksim_engine* e, const RunPlan& plan) {
  if (std::none_of(plan.groups.begin(), plan.groups.end(), [](const PlanGroup& g) { return g.kernel == kRunWsum; }))
    return KSIM_OK;
  std::vector<int> h((size_t)e->R * ksim_wsum::kWStride, 0);
  for (int r = 0; r < e->R; ++r) std::copy(e->wsum_w[r].begin(), e->wsum_w[r].end(), h.begin() + (size_t)r * ksim_wsum::kWStride);
  if (const int rc = e->d_wsum.upload(h, e->stream)) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));  // h is a local
  return KSIM_OK;
}
static int launch_wsum(ksim_engine* e, const RunPlan& plan, int gi, hipStream_t gs) {
  const PlanGroup& g = plan.groups[gi];
  if (!wsum::wsum_fits(e->N, g.wmask, plan.general)) return KSIM_ENOTSUP;
  const bool fgd = (g.wmask >> POL_FGD) & 1u, pwr = (g.wmask >> POL_PWR) & 1u;
  const void* f = fgd ? (pwr ? wsum_fn<true, true>(plan.general) : wsum_fn<true, false>(plan.general))
                      : (pwr ? wsum_fn<false, true>(plan.general) : wsum_fn<false, false>(plan.general));
  ksim_wsum::WsumArgs wa{e->d_reps.p, e->d_replist.p + g.first, e->d_wsum.p, e->N, g.wmask};
  const TypDev* tp = e->d_tp.p;
  const int rc = launch_persistent(f, g.count, ksim_wsum::kBlock, g.lds, gs, false, wa, tp);
  if (rc) return rc;
  note_launch(e, "k_wsum", 1, &e->stats.wsum, g.count);
  return KSIM_OK;
}

// A launch behind the residency gate (gate: asked for): fresh start flags for its n workgroups, launch(flags, epoch,
// &gated), then the host waits until every workgroup has started -- unless the launch cleared `gated` (it could not
// carry the flags).  The next group is launched after that, so none of its workgroups holds a CU these wait for.
static int launch_gated(ksim_engine* e, bool gate, int n, const char* what,
                        const std::function<int(int*, int, bool*)>& launch) {
  if (int rc = gate ? e->started.ensure((size_t)n) : KSIM_OK) return rc;  // the host-mapped start flags, one per workgroup
  int* flags = gate ? e->started.d : nullptr;
  const int epoch = gate ? (e->gate_epoch = (e->gate_epoch % 0x3fffffff) + 1) : 0;  // the launch stores it into them
  bool gated = gate;
  const int rc = launch(flags, epoch, &gated);
  if (rc) return rc;
  if (!gated) return KSIM_OK;
  // wait until the n workgroups have stored the epoch (bounded: past 2 s the gate gives up, counts it and says so on
  // stderr -- it orders work, it decides nothing)
  const auto t0 = std::chrono::steady_clock::now();
  volatile int* fl = e->started.h;
  if (e->stats.gate == 0) e->stats.gate = 1;
  for (int w = 0; w < n;) {
    if (fl[w] == epoch) { ++w; continue; }
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
      e->stats.gate = -1;
      ++e->gate_timeouts;
      std::fprintf(stderr, "ksim: residency gate given up after 2 s (%d of %d %s workgroups started); the next "
                   "groups launch unordered\n", w, n, what);
      break;
    }
    std::this_thread::yield();
  }
  return KSIM_OK;
}

// k_memo for the planned FGD replicas (prepare_memo; they are the first group of the order).  In a concurrent run
// (split_fgd) the next group is launched once all its workgroups have started: without the gate the later groups'
// workgroups could hold the CUs a wide replica's exchange waits on.
static int launch_memo_group(ksim_engine* e, const RunEnv& env, const RunPlan& plan, int gi, hipStream_t gs, int max_ev) {
  const PlanGroup& g = plan.groups[gi];
  const MemoPlan& pl = e->memo.plan;
  const bool gate = plan.concurrent && gi + 1 < (int)plan.groups.size();
  const int rc = launch_gated(e, gate, pl.nwg, "FGD k_memo", [&](int* flags, int epoch, bool*) {
    return launch_memo(e, env, pl, g.count, g.first, max_ev, gs, flags, epoch);
  });
  if (rc) return rc;
  note_launch(e, pl.hkeys ? "k_memo_hkeys" : "k_memo", pl.K, &e->stats.memo, g.count);
  if (env.timers()) std::fprintf(stderr, "ksim memo%s: %d replicas, K=%d, Cw=%d, F waves %d, LDS %zu B\n",
                                 pl.decider ? " (decider)" : "", g.count, pl.K, pl.Cw, pl.nfw, pl.lds);
  return KSIM_OK;
}

// k_hmemo: the keys in HBM.  The residency gate (concurrent groups behind a K = 1 FGD group; KSIM_VARIANT gate=0 off):
// the long FGD replays take their CUs before any short group's workgroup is dispatched, so none of them waits for
// a CU that short replays hold.  The host waits for every workgroup's start flag (bounded: a gate that does not open
// in 2 s lets the launches go on, it orders work, it decides nothing).
static int launch_hmemo_group(ksim_engine* e, const RunEnv& env, const RunPlan& plan, int gi, hipStream_t gs, int max_ev) {
  const PlanGroup& g = plan.groups[gi];
  const int K = e->hmemo.plan.K;
  const bool gate = plan.concurrent && gi + 1 < (int)plan.groups.size() && K == 1 && env.gate;
  const int rc = launch_gated(e, gate, g.count, "FGD k_hmemo", [&](int* flags, int epoch, bool* gated) {
    return launch_hmemo(e, env, g.count, g.first, max_ev, gs, flags, epoch, gated);
  });
  if (rc) return rc;
  note_launch(e, K == 1 ? "k_hmemo" : "k_hmemo_wide", K, &e->stats.hmemo, g.count);
  return KSIM_OK;
}

// PWR+FGD: the per-(class, slot) memo when every class of the group fits beside the slice (KSIM_VARIANT pf_memo=0:
// evaluate every slot every step, as before r04).  Returns the class stride (0: no memo) and the LDS bytes with it.
static int replay_pf_memo(const ksim_engine* e, const RunEnv& env, const RunPlan& plan, const PlanGroup& g, int K, int S,
                          size_t* lds) {
  if (g.kind != POL_PWR_FGD || !env.pf_memo) return 0;
  int pm_c = 0;
  for (int j = g.first; j < g.first + g.count; ++j) pm_c = std::max(pm_c, (int)e->h_cls[plan.order[j]].size());
  const size_t lm = ksim_replay::replay_layout(S, g.kind, plan.general, pm_c).total;
  if (!(pm_c > 0 && lm <= kLdsMax &&
        (K == 1 || resident_cap(e, replay_kernel(g.kind, K, plan.general), lm) >= g.count * K)))
    return 0;
  *lds = lm;
  return pm_c;
}

// The arguments of a k_replay launch, every field: the lean defaults (no PWR+FGD memo, the guessed ranges learnt, no
// profile buffer), which launch_replay overrides from the run's knobs.  xK > 0: a node-sharded group's launch
// (run_replay_group), the exchange spanning xK columns.
static ksim_replay::ReplayArgs replay_args(ReplicaDev* reps, const int* rep_list, int N, int K, int S,
                                           unsigned long long* gran, int2* hist, int max_ev, int* fail, bool skip, int xK) {
  ksim_replay::ReplayArgs ra;
  ra.reps = reps;
  ra.rep_list = rep_list;
  ra.N = N;
  ra.K = K;
  ra.S = S;
  ra.gran = gran;
  ra.hist = hist;
  ra.hist_stride = std::max(max_ev, 1);
  ra.fail = fail;
  ra.prof = nullptr;
  ra.skip = skip ? 1 : 0;
  ra.pm_c = 0;
  ra.pm_ver0 = 0u;
  ra.pf_guess = 1;
  ra.xK = xK;
  ra.group = xK > 0 ? 1 : 0;
  return ra;
}

// k_replay: one launch per policy (the kernel is specialised on it), K workgroups per replica.
static int launch_replay(ksim_engine* e, const RunEnv& env, const RunPlan& plan, int gi, hipStream_t gs, int max_ev) {
  const PlanGroup& g = plan.groups[gi];
  const int pol = g.kind, Rg = g.count;
  const bool general = plan.general, profile = env.timers();
  int K = g.K, S = g.S;
  if (g.lds > kLdsMax) return KSIM_ERANGE;
  if (K > 1) {
    // the occupancy query bounds the co-resident grid: fewer, larger slices when it is short
    const int cap = resident_cap(e, replay_kernel(pol, K, general), g.lds);
    const ReplayNarrow nw =
        replay_narrow(K, cap, Rg, e->N, e->wgs_req, [&](int s) { return replay::replay_lds(s, pol, general); });
    if (nw.refused == kNarrowLds)
      std::fprintf(stderr, "ksim: k_replay needs %d co-resident workgroups; the device holds %d\n", Rg * nw.K, cap);
    if (nw.refused != kNarrowOk) return KSIM_ERANGE;
    K = nw.K;
    S = nw.S;
  }
  int rc;
  if (plan.any_delete && (rc = e->d_hist.ensure((size_t)e->R * K * std::max(max_ev, 1)))) return rc;  // the bind history
  size_t lds = replay::replay_lds(S, pol, general);
  ksim_replay::ReplayArgs ra = replay_args(e->d_reps.p, e->d_replist.p + g.first, e->N, K, S, e->d_gran.p,
                                           plan.any_delete ? e->d_hist.p : nullptr, max_ev, e->d_fail.p,
                                           dead_skip(e, env, group_reps(plan, g)), 0);
  ra.pm_c = replay_pf_memo(e, env, plan, g, K, S, &lds);
  ra.pm_ver0 = env.pf_memo_ver0 > 0 && env.pf_memo_ver0 < (long)ksim_replay::kPmInvalid ? (unsigned)env.pf_memo_ver0 : 0u;
  ra.pf_guess = env.pf_guess ? 1 : 0;
  if (profile) {
    const size_t words = (size_t)Rg * K * ksim_replay::kProfPhases;
    if ((rc = e->d_prof.ensure(words))) return rc;
    KSIM_HIP(hipMemsetAsync(e->d_prof.p, 0, sizeof(unsigned long long) * words, e->stream));
    ra.prof = e->d_prof.p;
  }
  // re-initialise every polled word before the launch (granule tags restart at step 1; K = 1 polls none)
  if (K > 1)
    KSIM_HIP(hipMemsetAsync(e->d_gran.p, 0,
                            sizeof(unsigned long long) * (size_t)e->R * 2 * ksim_replay::kMaxK * ksim_replay::kGranW,
                            e->stream));
  const TypDev* tp = e->d_tp.p;
  rc = launch_persistent(replay_kernel(pol, K, general), Rg * K, ksim_replay::kRBlock, lds, gs, e->coop && K > 1, ra, tp);
  if (rc) return rc;
  note_launch(e, "k_replay", K, nullptr, Rg);
  if (profile) {
    // phase timers of this group (the stream is in order; read back before the next group reuses them)
    KSIM_HIP(hipStreamSynchronize(e->stream));
    print_replay_profile(e, Rg, K, max_ev);
  }
  return KSIM_OK;
}

// ---- a concurrent run's side streams ----
// Fork: the side streams start behind this point of the engine stream (KSIM_GROUP_TIMES=1: a timing event there too).
static int fork_streams(ksim_engine* e, const RunEnv& env) {
  if (int rc = e->ev_fork.ensure(hipEventDisableTiming)) return rc;
  KSIM_HIP(hipEventRecord(e->ev_fork, e->stream));
  if (env.group_times) {
    if (int rc = e->tev_fork.ensure()) return rc;
    KSIM_HIP(hipEventRecord(e->tev_fork, e->stream));
  }
  return KSIM_OK;
}

// The group's side stream, created on first use and put behind the fork the first time this run uses it.
static int enter_side_stream(ksim_engine* e, const PlanGroup& g, unsigned* used) {
  const int i = g.side;
  if (i < 0) return KSIM_OK;
  if (e->side[i].ensure() || e->side_ev[i].ensure(hipEventDisableTiming)) return KSIM_EHIP;
  if (!(*used & (1u << i))) KSIM_HIP(hipStreamWaitEvent(e->side[i], e->ev_fork, 0));
  *used |= 1u << i;
  return KSIM_OK;
}

// KSIM_GROUP_TIMES=1: a timing event at each used side stream's end (ksim_engine_run prints them).
static int record_group_times(ksim_engine* e, const RunEnv& env, const RunPlan& plan, unsigned used) {
  e->tev_used = 0u;
  if (!plan.concurrent || !env.group_times) return KSIM_OK;
  if (int rc = e->tev_fork.ensure()) return rc;
  for (int i = 0; i < (int)ksim_engine::kSide; ++i) {
    if (!(used & (1u << i))) continue;
    if (int rc = e->tev_side[i].ensure()) return rc;
    KSIM_HIP(hipEventRecord(e->tev_side[i], e->side[i]));
  }
  e->tev_used = used;
  return KSIM_OK;
}

// Join: the engine stream waits for every side stream used.
static int join_streams(ksim_engine* e, unsigned used) {
  for (int i = 0; i < (int)ksim_engine::kSide; ++i) {
    if (!(used & (1u << i))) continue;
    KSIM_HIP(hipEventRecord(e->side_ev[i], e->side[i]));
    KSIM_HIP(hipStreamWaitEvent(e->stream, e->side_ev[i], 0));
  }
  return KSIM_OK;
}

// A concurrent run's reports: each group's on its own stream, behind its replay -- the groups that finish early
// report while the longest still runs; a timing event pair around each (last_report_ms sums them).  ovl_group (-1:
// none): the group whose replicas report one by one as each ends (overlap_queue), behind the first group on its stream.
static int launch_group_reports(ksim_engine* e, const RunPlan& plan, int ovl_group) {
  const size_t ng = plan.groups.size();
  if (e->grp_rev.size() < 2 * ng) e->grp_rev.resize(2 * ng);
  for (DevEvent& v : e->grp_rev)
    if (v.ensure()) return KSIM_EHIP;
  for (size_t gi = 0; gi < ng; ++gi) {
    const PlanGroup& g = plan.groups[gi];
    const bool ovl = (int)gi == ovl_group;
    hipStream_t rs = group_stream(e, ovl ? plan.groups[0] : g);
    int mev = 0;
    for (int j = g.first; j < g.first + g.count; ++j) mev = std::max(mev, e->n_events[plan.order[j]]);
    if (ovl) KSIM_HIP(hipStreamWaitEvent(rs, e->ev_ovl, 0));
    KSIM_HIP(hipEventRecord(e->grp_rev[2 * gi], rs));
    if (ovl) {
      hipLaunchKernelGGL(ksim_rep::k_report_overlap, dim3(std::min(g.count, std::max(1, e->cus - e->cus / 16))),
                         dim3(ksim_rep::kScanBlock), 0, rs, (const ReplicaDev*)e->d_reps.p, (const TypDev*)e->d_tp.p, e->N,
                         (const int*)(e->d_replist.p + g.first), g.count, e->d_done.p, e->done_epoch, e->d_fail.p);
      KSIM_HIP(hipGetLastError());
    } else {
      const int rc = run_report(e, mev, rs, e->d_replist.p + g.first, g.count);
      if (rc) return rc;
    }
    KSIM_HIP(hipEventRecord(e->grp_rev[2 * gi + 1], rs));
  }
  e->grp_rev_used = (int)ng;
  e->report_done = true;
  return KSIM_OK;
}

// The persistent path: plan, upload the order, fork, launch each group, reports, join.
static int run_persistent(ksim_engine* e, const RunEnv& env, int max_ev) {
  const RunPlan plan = make_run_plan(run_plan_input(e, env));
  int rc = upload_go_states(e, plan);
  if (!rc) rc = upload_wsum_weights(e, plan);
  if (rc) return rc;
  e->stats.launches = (int)plan.groups.size();
  KSIM_HIP(hipMemcpyAsync(e->d_replist.p, plan.order.data(), sizeof(int) * plan.order.size(), hipMemcpyHostToDevice, e->stream));
  KSIM_HIP(hipMemsetAsync(e->d_fail.p, 0, sizeof(int), e->stream));
  if (plan.concurrent && (rc = fork_streams(e, env))) return rc;
  unsigned used = 0u;  // side streams the run has launched on
  int ovl_group = -1;
  for (int gi = 0; gi < (int)plan.groups.size(); ++gi) {
    const PlanGroup& g = plan.groups[gi];
    if ((rc = enter_side_stream(e, g, &used))) return rc;
    hipStream_t gs = group_stream(e, g);
    bool ovl = false;
    switch (g.kernel) {
      case kRunRandomGo: rc = launch_random_go(e, g, gs); break;
      case kRunScan1: rc = launch_scan1(e, env, plan, gi, gs, &ovl); break;
      case kRunMemo: rc = launch_memo_group(e, env, plan, gi, gs, max_ev); break;
      case kRunHmemo: rc = launch_hmemo_group(e, env, plan, gi, gs, max_ev); break;
      case kRunReplay: rc = launch_replay(e, env, plan, gi, gs, max_ev); break;
      case kRunNone: rc = KSIM_ENOTSUP; break;
      case kRunWsum: rc = launch_wsum(e, plan, gi, gs); break;
    }
    if (rc) return rc;
    if (ovl) ovl_group = gi;
  }
  if (plan.concurrent && e->report && (rc = launch_group_reports(e, plan, ovl_group))) return rc;
  if ((rc = record_group_times(e, env, plan, used))) return rc;
  e->stats.streams = __builtin_popcount(used);
  return plan.concurrent ? join_streams(e, used) : KSIM_OK;
}

static int run_graph(ksim_engine* e, int max_ev) {
  int rc = build_graph(e);
  if (rc) return rc;
  KSIM_HIP(hipMemsetAsync(e->d_base.p, 0, sizeof(int), e->stream));
  const int reps = (max_ev + e->K - 1) / e->K;
  for (int i = 0; i < reps; ++i) KSIM_HIP(hipGraphLaunch(e->graph, e->stream));
  return KSIM_OK;
}

int ksim_engine_run(ksim_engine* e) {
  if (!e) return KSIM_EINVAL;
  int max_ev = 0;
  for (int r = 0; r < e->R; ++r) {
    if (!e->d_ev[r].p) return KSIM_ESTATE;
    max_ev = std::max(max_ev, e->n_events[r]);
  }
  KSIM_HIP(hipSetDevice(e->device));
  const RunEnv env = read_env();
  e->report_done = false;
  e->rep_ready = false;
  e->ran = false;
  e->ds.invalidate();
  e->grp_rev_used = 0;
  e->tev_used = 0u;  // KSIM_GROUP_TIMES: only run_persistent's concurrent groups record side-stream ends
  e->stats = RunStats{};
  for (int r = 0; r < e->R; ++r) {  // the weighted combinations: k_wsum on the persistent path of an unsharded engine
    if (e->reps[r].policy != POL_WEIGHTED) continue;
    if (!e->wsum_set[r]) return KSIM_ESTATE;
    if (e->wsum_w[r][POL_PWR] > 0 && !e->pw_set[r]) return KSIM_ESTATE;
    if (e->shard.on() || e->run_mode == 1 || !wsum_selector_ok(e->reps[r].gpusel, e->wsum_w[r].data())) return KSIM_ENOTSUP;
  }
  int rc = prepare_memo(e, env, max_ev);
  if (rc) return rc;
  KSIM_HIP(hipEventRecord(e->ev0, e->stream));
  rc = reset_state(e);
  if (rc) return rc;
  if (e->report) KSIM_HIP(hipMemsetAsync(e->d_last.p, 0xff, sizeof(int32_t) * (size_t)e->N * e->R, e->stream));
  // run_mode 1: the per-pod path (k_step, + k_step_pwr for the PWR policies, hipGraph)
  const bool step_path = e->run_mode == 1;
  for (int r = 0; r < e->R; ++r)
    if (is_pwr_policy(e->reps[r].policy) && !e->pw_set[r]) return KSIM_ESTATE;
  for (int r = 0; r < e->R; ++r)  // Go-stream Random: the persistent path, best / worst / random selectors
    if (go_random(e, r) && (step_path || e->shard.on() ||
                            (e->reps[r].gpusel != SEL_BEST && e->reps[r].gpusel != SEL_WORST && e->reps[r].gpusel != SEL_RANDOM)))
      return KSIM_ENOTSUP;
  if (e->shard.runs_peer()) rc = run_hmemo_peer(e, env, max_ev);
  else if (e->shard.on()) rc = run_sharded(e, max_ev);
  else rc = step_path ? run_graph(e, max_ev) : run_persistent(e, env, max_ev);
  if (!rc && e->shard.on())
    note_kernel(e->stats, e->shard.runs_peer() ? "k_hmemo_wide" : any_pwr(e) ? "k_step+k_step_pwr" : "k_step");
  if (!rc && step_path) note_kernel(e->stats, any_pwr(e) ? "k_step+k_step_pwr" : "k_step");
  if (rc) return rc;
  KSIM_HIP(hipEventRecord(e->ev_mid, e->stream));
  if (e->report && !e->report_done) {
    rc = run_report(e, max_ev, e->stream, nullptr, e->R);
    if (rc) return rc;
  }
  KSIM_HIP(hipEventRecord(e->ev1, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  float ms = 0, rms = 0;
  KSIM_HIP(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  KSIM_HIP(hipEventElapsedTime(&rms, e->ev_mid, e->ev1));
  e->stats.ms = ms;
  e->stats.report_ms = e->report ? rms : 0.0;
  for (int g = 0; g < e->grp_rev_used; ++g) {  // concurrent groups: each group's report on its side stream
    float gms = 0.f;
    KSIM_HIP(hipEventElapsedTime(&gms, e->grp_rev[2 * g], e->grp_rev[2 * g + 1]));
    e->stats.report_ms += gms;
  }
  if (e->tev_used) {  // KSIM_GROUP_TIMES=1
    std::fprintf(stderr, "ksim group times (ms from the fork to each side stream's end):");
    for (int i = 0; i < (int)ksim_engine::kSide; ++i) {
      float gms = 0.f;
      if ((e->tev_used >> i) & 1u && hipEventElapsedTime(&gms, e->tev_fork, e->tev_side[i]) == hipSuccess)
        std::fprintf(stderr, " side%d %.3f;", i, gms);
    }
    for (int g = 0; g < e->grp_rev_used; ++g) {  // each group's replay end (= its report's start) and report end
      float a = 0.f, b = 0.f;
      if (hipEventElapsedTime(&a, e->tev_fork, e->grp_rev[2 * g]) == hipSuccess &&
          hipEventElapsedTime(&b, e->tev_fork, e->grp_rev[2 * g + 1]) == hipSuccess)
        std::fprintf(stderr, " g%d replay %.3f report %.3f;", g, a, b);
    }
    std::fprintf(stderr, " run %.3f\n", ms);
  }
  e->stats.steps = max_ev;
  e->stats.step_path = step_path;
  if (!step_path && e->shard.world == 0) {
    int fail = 0;
    KSIM_HIP(hipMemcpy(&fail, e->d_fail.p, sizeof(int), hipMemcpyDeviceToHost));
    if (fail & 2) return KSIM_ERANGE;  // a raw PWR score outside the 24-bit key field
    if (fail & 60) std::fprintf(stderr, "ksim: a memoised kernel's LDS wait timed out (fail bits 0x%x)\n", fail);
    if (fail & 64) std::fprintf(stderr, "ksim: the overlapped report waited too long for a replay (fail bits 0x%x)\n", fail);
    if (fail) return KSIM_ESTATE;  // a granule poll or an LDS wait timed out
  }
  e->ran = true;
  e->rep_ready = e->report;
  return KSIM_OK;
}

int ksim_shard_comm_id(uint8_t* out) {
  if (!out) return KSIM_EINVAL;
  RcclApi* r = rccl();
  if (!r) return KSIM_ENOTSUP;
  ncclUniqueId id;
  if (r->get_unique_id(&id) != ncclSuccess) return KSIM_EHIP;
  std::memcpy(out, id.internal, KSIM_SHARD_ID_BYTES);
  return KSIM_OK;
}

int ksim_engine_set_shard(ksim_engine* e, int rank, int world, int node_offset, int n_global, const uint8_t* comm_id) {
  if (!e || world < 1 || world > 16 || rank < 0 || rank >= world || node_offset < 0 || n_global < e->N ||
      node_offset + e->N > n_global || n_global > kMaxRank || e->R != 1)
    return KSIM_EINVAL;
  if (e->shard.on()) return KSIM_ESTATE;  // once per engine, before set_nodes
  KSIM_HIP(hipSetDevice(e->device));
  if (comm_id) {
    RcclApi* r = rccl();
    if (!r) return KSIM_ENOTSUP;
    ncclUniqueId id;
    std::memcpy(id.internal, comm_id, KSIM_SHARD_ID_BYTES);
    const ncclResult_t nr = r->comm_init_rank(&e->shard.comm.h, world, id, rank);
    if (nr != ncclSuccess) {
      std::fprintf(stderr, "ksim: ncclCommInitRank failed: %s\n", r->error_string(nr));
      e->shard.comm.h = nullptr;
      return KSIM_EHIP;
    }
  }
  int rc = e->shard.d_send.alloc(4);
  if (!rc) rc = e->shard.d_recv.alloc(4 * (size_t)world);
  if (!rc) rc = e->shard.d_send.zero(e->stream);
  if (rc) return rc;
  e->shard.transport = comm_id ? ShardTransport::rccl : ShardTransport::group;
  e->shard.world = world;
  e->shard.rank = rank;
  e->shard.node_off = node_offset;
  e->shard.n_global = n_global;
  e->reps[0].node_off = node_offset;
  rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

int ksim_engine_set_shard_exchange(ksim_engine* e, ksim_shard_exchange_fn fn, void* user) {
  if (!e) return KSIM_EINVAL;
  ShardState& sh = e->shard;
  if (!sh.takes_exchange_fn()) return KSIM_ESTATE;  // after set_shard, and not beside RCCL
  sh.xfn = fn;
  sh.xuser = user;
  sh.h_send.assign(4, 0);
  sh.h_recv.assign(4 * (size_t)sh.world, 0);
  // a null function takes the host exchange away again; mapped peers stay the transport whatever is installed
  if (!sh.runs_peer()) sh.transport = fn ? ShardTransport::host : ShardTransport::group;
  return KSIM_OK;
}

// ---- one shard per process: device-initiated exchange through IPC-mapped granule buffers ----
constexpr size_t kPeerGranBytes = sizeof(unsigned long long) * 2 * 256 * 2;  // 2 slots x 256 columns x 2
constexpr uint32_t kPeerMagic = 0x4850534bu;  // "KSPH" after the IPC handle (include/ksim_engine.h)

// The device ordinal in this process of the GPU a peer handle names (PCI domain / bus / device), -1 if it
// is not visible here; -2 for a malformed handle.
static int peer_device(const uint8_t* hd) {
  uint32_t tail[5];
  std::memcpy(tail, hd + sizeof(hipIpcMemHandle_t), sizeof tail);
  if (tail[0] != kPeerMagic) return -2;
  char bus[32];
  std::snprintf(bus, sizeof bus, "%04x:%02x:%02x.0", tail[1], tail[2], tail[3]);
  int dev = -1;
  if (hipDeviceGetByPCIBusId(&dev, bus) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return dev;
}

int ksim_shard_peer_handle(ksim_engine* e, uint8_t* out) {
  if (!e || !out) return KSIM_EINVAL;
  ShardState& sh = e->shard;
  if (!sh.in_process()) return KSIM_ESTATE;
  KSIM_HIP(hipSetDevice(e->device));
  if (!sh.d_pgran.p) {
    // uncached device memory: the peers' stores land in it over xGMI and the local polls read it there
    int rc = sh.d_pgran.alloc(kPeerGranBytes / sizeof(unsigned long long), hipDeviceMallocUncached);
    if (!rc) rc = sh.d_pgran.zero(e->stream);
    if (rc) return rc;
    KSIM_HIP(hipStreamSynchronize(e->stream));
  }
  if (sh.pgran_handle.empty()) {
    hipIpcMemHandle_t h;
    KSIM_HIP(hipIpcGetMemHandle(&h, sh.d_pgran.p));
    static_assert(sizeof(hipIpcMemHandle_t) + 20 <= KSIM_SHARD_HANDLE_BYTES, "IPC handle size");
    hipDeviceProp_t prop;
    KSIM_HIP(hipGetDeviceProperties(&prop, e->device));
    const uint32_t tail[5] = {kPeerMagic, (uint32_t)prop.pciDomainID, (uint32_t)prop.pciBusID,
                              (uint32_t)prop.pciDeviceID, (uint32_t)getpid()};
    sh.pgran_handle.assign(KSIM_SHARD_HANDLE_BYTES, 0);
    std::memcpy(sh.pgran_handle.data(), &h, sizeof h);
    std::memcpy(sh.pgran_handle.data() + sizeof h, tail, sizeof tail);
  }
  std::memcpy(out, sh.pgran_handle.data(), KSIM_SHARD_HANDLE_BYTES);
  return KSIM_OK;
}

int ksim_engine_set_shard_peers(ksim_engine* e, const uint8_t* handles) {
  if (!e || !handles) return KSIM_EINVAL;
  ShardState& sh = e->shard;
  if (!sh.can_map_peers()) return KSIM_ESTATE;  // after ksim_shard_peer_handle, once
  KSIM_HIP(hipSetDevice(e->device));
  const int world = sh.world;
  if (const long ep = test_knob("peer_epoch0", 0))  // tests: start the run epoch near its wrap
    sh.peer_epoch = (int)(ep & 0xffffff);
  if (std::memcmp(handles + (size_t)sh.rank * KSIM_SHARD_HANDLE_BYTES, sh.pgran_handle.data(), KSIM_SHARD_HANDLE_BYTES) != 0)
    return KSIM_EINVAL;  // this shard's own handle must sit at its rank
  // every peer's device first: visible here and reachable (xGMI / P2P), or nothing is mapped
  for (int q = 0; q < world; ++q) {
    if (q == sh.rank) continue;
    const int pd = peer_device(handles + (size_t)q * KSIM_SHARD_HANDLE_BYTES);
    int can = pd == e->device ? 1 : 0;
    if (pd >= 0 && pd != e->device) {
      if (hipDeviceCanAccessPeer(&can, e->device, pd) != hipSuccess) {
        (void)hipGetLastError();
        can = 0;
      }
    }
    if (pd < 0 || !can) {
      std::fprintf(stderr, "ksim: shard %d's exchange buffer is %s\n", q,
                   pd == -2 ? "a malformed handle" : pd == -1 ? "on a GPU not visible in this process"
                                                               : "on a GPU without a peer path from this one");
      return pd == -2 ? KSIM_EINVAL : KSIM_EPEER;
    }
  }
  int bad = -1;
  hipError_t why = hipSuccess;
  if (const int rc = sh.peers.open(handles, KSIM_SHARD_HANDLE_BYTES, world, sh.rank, sh.d_pgran.p, &bad, &why)) {
    std::fprintf(stderr, "ksim: hipIpcOpenMemHandle (shard %d): %s\n", bad, hipGetErrorString(why));
    (void)hipGetLastError();
    return rc;
  }
  sh.transport = ShardTransport::peer;
  return KSIM_OK;
}

// ---- the steps the node-sharded runs share ----
// One shard back to its initial state, enqueued on `st`: the node records and tag counts, the report's last-event
// table when the report is on (k_step's; the replay kernels keep theirs in LDS and reset it as they start), and with
// `results` the result records (the replay kernels write a result only where a shard has one to report).
static int reset_shard_state(ksim_engine* e, hipStream_t st, bool results) {
  KSIM_HIP(hipMemcpyAsync(e->d_nodes.p, e->d_nodes_init.p, sizeof(NodeRec) * (size_t)e->N, hipMemcpyDeviceToDevice, st));
  KSIM_HIP(hipMemcpyAsync(e->d_tags.p, e->d_tags_init.p, sizeof(uint16_t) * e->tags_stride, hipMemcpyDeviceToDevice, st));
  if (results)
    KSIM_HIP(hipMemsetAsync(e->d_res[0].p, 0xff, sizeof(ResultDev) * (size_t)std::max(e->n_events[0], 1), st));
  if (e->report) KSIM_HIP(hipMemsetAsync(e->d_last.p, 0xff, sizeof(int32_t) * (size_t)e->N, st));
  return KSIM_OK;
}

// The end of a node-sharded replay on e's stream: the closing event, the wait, the fail word of its one launch
// (fail_word false: the per-pod k_step path has none) -- KSIM_ESTATE for a replay that gave up, KSIM_ERANGE for
// a raw PWR score outside the key field -- and the time from ev0 to the closing event into e->stats.
static int end_replay(ksim_engine* e, hipEvent_t closing, bool fail_word) {
  KSIM_HIP(hipEventRecord(closing, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  int fail = 0;
  if (fail_word) KSIM_HIP(hipMemcpy(&fail, e->d_fail.p, sizeof(int), hipMemcpyDeviceToHost));
  if (fail & 2) return KSIM_ERANGE;  // a raw PWR score outside the 24-bit key field (as ksim_engine_run)
  if (fail) return KSIM_ESTATE;
  float ms = 0;
  KSIM_HIP(hipEventElapsedTime(&ms, e->ev0, closing));
  e->stats.ms = ms;
  return KSIM_OK;
}

// The end of an in-process group's run on engine 0's stream: end_replay, then the run's time and diagnostics on every
// engine.  K = 0: the per-pod k_step path, which has no fail word and no width.
//
// With the cluster report on (every shard or none: ksim_shard_group_run checks), the report follows the replay once
// its fail word is read clean (a replay that gave up leaves events without a snapshot): every shard's own report
// (run_report: its nodes' terms, the arrivals on shard 0) and the merge of the shards' records into engine 0's
// d_rmerge (k_report_merge), all on the group's stream.  last_report_ms on every engine is the time of all of that;
// last_ms includes it, as ksim_engine_run's does.  Without the report the run ends as it always did.
static int finish_group_run(ksim_engine* const* engines, int world, int max_ev, int K, const char* kernel, bool hmemo) {
  ksim_engine* e0 = engines[0];
  hipStream_t st = e0->stream;
  const bool report = e0->report;
  int rc = end_replay(e0, report ? e0->ev_mid : e0->ev1, K > 0);
  if (rc) return rc;
  RunStats& s = e0->stats;
  if (report) {
    ksim_rep::MergeArgs ma{};
    for (int k = 0; k < world; ++k) {
      if ((rc = run_report(engines[k], max_ev, st, nullptr, 1))) return rc;
      ma.part[k] = engines[k]->d_rep[0].p;
    }
    if ((rc = e0->shard.group.d_rmerge.ensure((size_t)std::max(max_ev, 1)))) return rc;
    const bool times = read_env().group_times;  // KSIM_GROUP_TIMES=1: the merge's share of the report, on stderr
    if (times) {
      if ((rc = e0->tev_fork.ensure())) return rc;
      KSIM_HIP(hipEventRecord(e0->tev_fork, st));
    }
    if (max_ev > 0) {
      const long long lanes = (long long)max_ev * ksim_rep::kMergeLanes;
      hipLaunchKernelGGL(ksim_rep::k_report_merge, dim3((unsigned)((lanes + ksim_rep::kMergeBlock - 1) / ksim_rep::kMergeBlock)),
                         dim3(ksim_rep::kMergeBlock), 0, st, ma, world, max_ev, e0->shard.group.d_rmerge.p);
      KSIM_HIP(hipGetLastError());
    }
    KSIM_HIP(hipEventRecord(e0->ev1, st));
    KSIM_HIP(hipStreamSynchronize(st));
    float rms = 0, ms = 0;
    KSIM_HIP(hipEventElapsedTime(&rms, e0->ev_mid, e0->ev1));
    KSIM_HIP(hipEventElapsedTime(&ms, e0->ev0, e0->ev1));  // the run's time takes the report in
    s.report_ms = rms;
    s.ms = ms;
    e0->shard.group.rmerge_n = max_ev;
    float mms = 0;
    if (times && hipEventElapsedTime(&mms, e0->tev_fork, e0->ev1) == hipSuccess)
      std::fprintf(stderr, "ksim group report times (ms): %d shards' reports %.3f; merge %.3f\n", world, rms - mms, mms);
  }
  s.steps = max_ev;
  s.K = K;
  s.hmemo = hmemo ? 1 : 0;
  s.kernels = kernel;
  for (int k = 0; k < world; ++k) {  // one run: the same diagnostics on every engine of the group
    if (k > 0) engines[k]->stats = s;
    engines[k]->rep_ready = report;
    engines[k]->ran = true;  // (a descheduling plan may follow: ksim_shard_group_deschedule)
  }
  return KSIM_OK;
}

// One shard's k_hmemo launch arguments, for its K slices of S ranks among the Kt columns of the exchange through
// `gran`, the shard's first column being wbase: the replica list and the plan on the shard's own stream (the plan is
// not the unsharded one: the cache is dropped), then on `st` the shard back to its initial state and the keys, and the
// bind history when the stream deletes.  KSIM_OK with *planned = false: no plan for these slices, nothing enqueued on st.
static int shard_hmemo_args(ksim_engine* e, const RunEnv& env, int max_ev, int K, int S, int Kt, int wbase,
                            unsigned long long* gran, hipStream_t st, ksim_hmemo::HMemoArgs* a, bool* planned) {
  const int stride = std::max(max_ev, 1);
  const int zero = 0;
  KSIM_HIP(hipMemcpyAsync(e->d_replist.p, &zero, sizeof(int), hipMemcpyHostToDevice, e->stream));
  int rc = prepare_hmemo(e, env, std::vector<int>{0}, max_ev, K, S);
  if (rc) return rc;
  if (!(*planned = e->hmemo.ok)) return KSIM_OK;
  e->mplan_dirty = true;
  if (st != e->stream) KSIM_HIP(hipStreamSynchronize(e->stream));  // the group's stream is engine 0's
  if ((rc = reset_shard_state(e, st, true))) return rc;
  if ((rc = hmemo_init_keys(e, 1, 0, st, e->shard.node_off))) return rc;
  *a = hmemo_args(e, env, 0, stride);
  a->roff = e->shard.node_off;
  a->wbase = wbase;
  a->Ktot = Kt;
  a->gran = gran;
  if (e->has_delete[0]) {
    if ((rc = e->hmemo.hist.ensure((size_t)K * stride))) return rc;
    a->hist = e->hmemo.hist.p;
  }
  return KSIM_OK;
}

// ksim_engine_run of a shard with peers: k_hmemo over this shard's slices, the exchange spanning every
// shard's workgroups (K per shard, the same K and S on every rank: from n_global and world only).
static int run_hmemo_peer(ksim_engine* e, const RunEnv& env, int max_ev) {
  using namespace ksim_hmemo;
  if (e->R != 1 || e->reps[0].policy != POL_FGD || go_random(e, 0) || !score_table()) return KSIM_ENOTSUP;
  ShardState& sh = e->shard;
  const int world = sh.world;
  const ShardSlices sl = hmemo_peer_slices(sh.n_global, world, e->N);
  if (!sl.ok) return KSIM_ENOTSUP;
  const int K = sl.K, Kt = world * K;
  hipStream_t st = e->stream;
  HMemoArgs a;
  bool planned = false;
  int rc = shard_hmemo_args(e, env, max_ev, K, sl.S, Kt, sh.rank * K, sh.d_pgran.p, st, &a, &planned);
  if (rc) return rc;
  if (!planned) return KSIM_ENOTSUP;
  a.npeer = world;
  sh.peer_epoch = (sh.peer_epoch + 1) & 0xffffff;  // every rank runs the same runs: the same epoch (24 bits)
  if (sh.peer_epoch == 0) sh.peer_epoch = 1;
  a.epoch = sh.peer_epoch;
  for (int q = 0; q < world; ++q) a.peer[q] = sh.peers.ptr[q];
  KSIM_HIP(hipMemsetAsync(e->d_fail.p, 0, sizeof(int), st));
  const void* f = hmemo_kernel(hmemo_form(kHPeer, Kt, false, a.delay, false));
  if (K > resident_cap(e, f, e->hmemo.plan.lds)) return KSIM_ERANGE;
  KSIM_HIP(hipEventRecord(e->ev0, st));
  const TypDev* tpp = e->d_tp.p;
  // a plain launch: K <= 64 one-per-CU workgroups are resident (checked above), and a cooperative launch
  // takes the device's one global-wave-sync resource, which a second shard process on the same device
  // would wait for behind the first's persistent kernel
  if ((rc = launch_persistent(f, K, kHBlock, e->hmemo.plan.lds, st, false, a, tpp))) return rc;
  if ((rc = end_replay(e, e->ev1, true))) return rc;  // (ksim_engine_run's tail times the run to the end of its report)
  e->stats.K = K;
  e->stats.hmemo = 1;
  return KSIM_OK;
}

// ---- a node-sharded FGD cluster on k_hmemo (one launch for the whole in-process group) ----
// Every shard engine keeps its own plan, keys, L1 and node records; the launch's workgroups are the
// shards' slices (K per shard, S ranks each), and each pod step's slice maxima go through ONE exchange of
// world x K granule columns: selectHost over the union (generic_scheduler.go:187-212), the owner of the
// winner binds.  Results carry global ranks as the k_step shards' do (ksim/shard.py merge_results).
static bool hmemo_group_eligible(ksim_engine* const* engines, int world, const RunEnv& env) {
  if (!env.shard_hmemo) return false;
  if (!score_table()) return false;
  for (int k = 0; k < world; ++k) {
    const ksim_engine* e = engines[k];
    if (e->R != 1 || e->reps[0].policy != POL_FGD || e->run_mode == 1 || e->run_mode == 2 || go_random(e, 0))
      return false;
  }
  return true;
}

// The cheap policies' node-sharded group on k_replay slices (r06, round-5 verdict item 7): every shard's K slices in
// ONE launch, one exchange of Kt = world x K columns per pod step (the keys carry global name ranks, so the max is
// selectHost over the union, generic_scheduler.go:187-212; BestFit's NormalizeScore range rides in the same granules
// as in the unsharded k_replay, plugin_utils.go:48-74).  One replica per shard, a create-only stream, no profile;
// with the cluster report on, the general instantiation (its report stores) where its layout fits.
static bool replay_group_eligible(ksim_engine* const* engines, int world, const RunEnv& env) {
  const int pol = engines[0]->reps[0].policy;
  // the PWR policies too: plain PWR's one key round (the argmax of NormalizeScore is the argmax of the raw score) and
  // PWR+FGD's round of A totals and guessed-range keys, with its miss round, span the shards' columns as a cheap
  // policy's round does -- the cluster's raw range comes out of the same granules
  if (((pol < POL_BESTFIT || pol > POL_RANDOM) && !is_pwr_policy(pol)) || variant("shard_replay", 1) == 0) return false;
  for (int k = 0; k < world; ++k) {
    const ksim_engine* e = engines[k];
    if (e->R != 1 || e->reps[0].policy != pol || e->run_mode == 1 || e->has_delete[0] || go_random(e, 0)) return false;
  }
  return env.profile == 0;
}

// KSIM_OK with *done = false: the group does not fit (the caller keeps the per-pod k_step path).
static int run_replay_group(ksim_engine* const* engines, int world, const RunEnv& env, int max_ev, bool* done) {
  using namespace ksim_replay;
  *done = false;
  ksim_engine* e0 = engines[0];
  int N = 1;  // slices cover the largest shard
  for (int k = 0; k < world; ++k) N = std::max(N, engines[k]->N);
  const int pol = e0->reps[0].policy;
  const ShardSlices sl = replay_group_slices(N, world, e0->cus, pol, env.group_k);
  if (!sl.ok) return KSIM_OK;
  const int K = sl.K, S = sl.S, Kt = world * K;
  const bool general = e0->report;  // the report stores (snap / prev) are the general instantiation's
  const void* f = replay_kernel(pol, Kt, general);
  const size_t lds = replay::replay_lds(S, pol, general);
  if (lds > kLdsMax || Kt > resident_cap(e0, f, lds)) return KSIM_OK;
  hipStream_t st = e0->stream;
  KSIM_HIP(hipSetDevice(e0->device));
  int rc;
  if ((rc = e0->shard.group.d_rgran.ensure((size_t)2 * 256 * kGranW))) return rc;
  if ((rc = e0->shard.group.d_rgreps.ensure(16))) return rc;
  if (!e0->shard.group.d_rglist.p) {
    std::vector<int> id(16);
    std::iota(id.begin(), id.end(), 0);
    if ((rc = e0->shard.group.d_rglist.upload(id, st))) return rc;
    KSIM_HIP(hipStreamSynchronize(st));  // `id` is pageable
  }
  bool skip = true;
  for (int k = 0; k < world; ++k) {
    ksim_engine* e = engines[k];
    KSIM_HIP(hipStreamSynchronize(e->stream));
    if ((rc = reset_shard_state(e, st, true))) return rc;
    KSIM_HIP(hipMemcpyAsync(e0->shard.group.d_rgreps.p + k, e->d_reps.p, sizeof(ReplicaDev), hipMemcpyDeviceToDevice, st));
    skip = skip && dead_skip(e, env, std::vector<int>{0});
  }
  ReplayArgs ra =
      replay_args(e0->shard.group.d_rgreps.p, e0->shard.group.d_rglist.p, N, K, S, e0->shard.group.d_rgran.p, nullptr, max_ev, e0->d_fail.p, skip, Kt);
  ra.pf_guess = env.pf_guess ? 1 : 0;  // (PWR+FGD; its per-class memo stays off in a group: pm_c = 0)
  KSIM_HIP(hipMemsetAsync(e0->shard.group.d_rgran.p, 0, sizeof(unsigned long long) * 2 * (size_t)Kt * kGranW, st));
  KSIM_HIP(hipMemsetAsync(e0->d_fail.p, 0, sizeof(int), st));
  KSIM_HIP(hipEventRecord(e0->ev0, st));
  const TypDev* tp = e0->d_tp.p;  // (the cheap policies and PWR read no typical table)
  if (pol == POL_PWR_FGD) {  // the kernel reads replica r's table at tp + r * kMaxTypical, r the shard's place in the list
    if ((rc = e0->shard.group.d_rgtp.ensure((size_t)16 * kMaxTypical))) return rc;
    for (int k = 0; k < world; ++k)
      KSIM_HIP(hipMemcpyAsync(e0->shard.group.d_rgtp.p + (size_t)k * kMaxTypical, engines[k]->d_tp.p,
                              sizeof(TypDev) * kMaxTypical, hipMemcpyDeviceToDevice, st));
    tp = e0->shard.group.d_rgtp.p;
  }
  if ((rc = launch_persistent(f, Kt, kRBlock, lds, st, e0->coop, ra, tp))) return rc;
  if ((rc = finish_group_run(engines, world, max_ev, K, "k_replay_group", false))) return rc;
  *done = true;
  return KSIM_OK;
}

// KSIM_OK with *done = false: the group does not fit k_hmemo (the caller keeps the per-pod k_step path).
static int run_hmemo_group(ksim_engine* const* engines, int world, const RunEnv& env, int max_ev, bool* done) {
  using namespace ksim_hmemo;
  *done = false;
  ksim_engine* e0 = engines[0];
  ShardState::Group& grp = e0->shard.group;
  int nmax = 1;
  for (int k = 0; k < world; ++k) nmax = std::max(nmax, engines[k]->N);
  const ShardSlices sl = hmemo_group_slices(nmax, world, e0->cus);
  if (!sl.ok) return KSIM_OK;
  const int K = sl.K, Kt = world * K;
  hipStream_t st = e0->stream;
  KSIM_HIP(hipSetDevice(e0->device));
  int rc;
  if ((rc = grp.d_ggran.ensure((size_t)2 * 256 * 2))) return rc;
  if ((rc = grp.d_hgargs.ensure(16))) return rc;
  std::vector<HMemoArgs> args(world);
  size_t lds = 0;
  for (int k = 0; k < world; ++k) {
    bool planned = false;
    if ((rc = shard_hmemo_args(engines[k], env, max_ev, K, sl.S, Kt, k * K, grp.d_ggran.p, st, &args[k], &planned))) return rc;
    if (!planned) return KSIM_OK;  // (the fall-back resets the shards already prepared again)
    args[k].fail = e0->d_fail.p;
    lds = std::max(lds, engines[k]->hmemo.plan.lds);
  }
  const void* f = hmemo_kernel(hmemo_form(kHGroup, Kt, false, env.hdelay, false));
  if (Kt > resident_cap(e0, f, lds)) return KSIM_OK;
  KSIM_HIP(hipMemcpyAsync(grp.d_hgargs.p, args.data(), sizeof(HMemoArgs) * world, hipMemcpyHostToDevice, st));
  KSIM_HIP(hipMemsetAsync(grp.d_ggran.p, 0, sizeof(unsigned long long) * 2 * (size_t)Kt * 2, st));
  KSIM_HIP(hipMemsetAsync(e0->d_fail.p, 0, sizeof(int), st));
  KSIM_HIP(hipStreamSynchronize(st));  // `args` is pageable
  KSIM_HIP(hipEventRecord(e0->ev0, st));
  KSIM_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const HMemoArgs* ap = grp.d_hgargs.p;
  int Kk = K;
  void* params[] = {(void*)&ap, (void*)&Kk};
  const hipError_t lr = e0->coop ? hipLaunchCooperativeKernel(f, dim3(Kt), dim3(kHBlock), params, (unsigned)lds, st)
                                 : hipLaunchKernel(f, dim3(Kt), dim3(kHBlock), params, lds, st);
  if (lr == hipErrorCooperativeLaunchTooLarge) {
    (void)hipGetLastError();
    return KSIM_OK;
  }
  KSIM_HIP(lr);
  if ((rc = finish_group_run(engines, world, max_ev, K, "k_hmemo_group", true))) return rc;
  *done = true;
  return KSIM_OK;
}

// Engine k of the `world` given to a group entry point: rank k of that world, exchanging in this process, on engine
// 0's device.
static bool group_member_ok(ksim_engine* const* engines, int world, int k) {
  const ksim_engine* e = engines[k];
  return e && engines[0] && e->shard.world == world && e->shard.rank == k && e->shard.in_process() &&
         e->device == engines[0]->device;
}

int ksim_shard_group_run(ksim_engine* const* engines, int world) {
  if (!engines || world < 1 || world > 16) return KSIM_EINVAL;
  ksim_engine* e0 = engines[0];
  int max_ev = 0;
  for (int k = 0; k < world; ++k) {
    ksim_engine* e = engines[k];
    if (!group_member_ok(engines, world, k) || !e->d_ev[0].p) return KSIM_EINVAL;
    if (e->n_events[0] != e0->n_events[0]) return KSIM_EINVAL;  // every shard sees the same events
    if (e->report != e0->report) return KSIM_EINVAL;            // and reports, or none does: the records are merged
    max_ev = std::max(max_ev, e->n_events[0]);
  }
  for (int k = 0; k < world; ++k) {
    // every shard takes the same rounds per pod; as ksim_engine_run, a PWR policy scores with the shard's power model
    if (is_pwr_policy(engines[k]->reps[0].policy) != is_pwr_policy(e0->reps[0].policy)) return KSIM_EINVAL;
    if (is_pwr_policy(engines[k]->reps[0].policy) && !engines[k]->pw_set[0]) return KSIM_ESTATE;
    if (engines[k]->reps[0].policy == POL_WEIGHTED) return KSIM_ENOTSUP;  // k_wsum holds the whole cluster in one workgroup
  }
  KSIM_HIP(hipSetDevice(e0->device));
  for (int k = 0; k < world; ++k) {
    engines[k]->rep_ready = false;
    engines[k]->stats = RunStats{};
    engines[k]->ran = false;
    engines[k]->ds.invalidate();
  }
  e0->shard.group.rmerge_n = -1;
  const RunEnv env = read_env();
  if (hmemo_group_eligible(engines, world, env)) {
    bool done = false;
    const int rc = run_hmemo_group(engines, world, env, max_ev, &done);
    if (rc || done) return rc;
  }
  if (replay_group_eligible(engines, world, env)) {
    bool done = false;
    const int rc = run_replay_group(engines, world, env, max_ev, &done);
    if (rc || done) return rc;
  }
  // a PWR policy: two rounds per pod (the raw score range, then the keys under the cluster's range)
  const bool pwr = any_pwr(e0);
  const char* path = pwr ? "k_step+k_step_pwr" : "k_step";
  for (int k = 0; k < world; ++k) engines[k]->stats.kernels = path;  // (named first: a failed run names its path too)
  if (int rc = e0->shard.group.d_ptrs.ensure(32)) return rc;
  std::vector<unsigned long long*> ptrs(32, nullptr);
  for (int k = 0; k < world; ++k) {
    ptrs[k] = engines[k]->shard.d_send.p;
    ptrs[16 + k] = engines[k]->shard.d_recv.p;
  }
  hipStream_t st = e0->stream;
  KSIM_HIP(hipMemcpyAsync(e0->shard.group.d_ptrs.p, ptrs.data(), sizeof(unsigned long long*) * 32, hipMemcpyHostToDevice, st));
  int rc;
  for (int k = 0; k < world; ++k) {
    KSIM_HIP(hipStreamSynchronize(engines[k]->stream));
    if ((rc = reset_shard_state(engines[k], st, false))) return rc;
  }
  KSIM_HIP(hipEventRecord(e0->ev0, st));
  auto gather = [&]() -> int {
    hipLaunchKernelGGL(k_shard_gather, dim3(1), dim3(1024), 0, st, (unsigned long long* const*)e0->shard.group.d_ptrs.p,
                       (unsigned long long* const*)(e0->shard.group.d_ptrs.p + 16), world);
    KSIM_HIP(hipGetLastError());
    return KSIM_OK;
  };
  for (int s = 0; s < max_ev; ++s) {
    for (int k = 0; k < world; ++k)
      if ((rc = shard_local(engines[k], st, nullptr, s))) return rc;
    if ((rc = gather())) return rc;
    if (pwr) {
      for (int k = 0; k < world; ++k)
        if ((rc = shard_pwr(engines[k], st, nullptr, s))) return rc;
      if ((rc = gather())) return rc;
    }
    for (int k = 0; k < world; ++k)
      if ((rc = shard_commit(engines[k], st, nullptr, s))) return rc;
  }
  return finish_group_run(engines, world, max_ev, 0, path, false);
}

int ksim_engine_set_report(ksim_engine* e, int enable) {
  if (!e) return KSIM_EINVAL;
  e->report = enable != 0;
  KSIM_HIP(hipSetDevice(e->device));
  for (int r = 0; r < e->R; ++r) {
    int rc = alloc_report(e, r);
    if (rc) return rc;
  }
  int rc = upload_reps(e);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

// The exact records (ksim_report_part is RepAcc byte for byte; ksim_report_host.hpp turns them into reports).
static_assert(sizeof(ksim_report_part) == sizeof(RepAcc) && offsetof(ksim_report_part, cnt) == offsetof(RepAcc, cnt),
              "ksim_report_part must match RepAcc");
static_assert(ksim_rep::kMaxWorld == ksim_rep_host::kMaxWorld && ksim_rep::kFx == ksim_rep_host::kFx, "report limits");

// n records of `src` (device) into out, cnt[7] = total_gpus on each.
static int fetch_parts(ksim_engine* e, const RepAcc* src, ksim_report_part* out, int n, int64_t total_gpus) {
  if (n == 0) return KSIM_OK;
  KSIM_HIP(hipSetDevice(e->device));
  KSIM_HIP(hipMemcpyAsync(out, src, sizeof(RepAcc) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  for (int i = 0; i < n; ++i) out[i].cnt[7] = total_gpus;
  return KSIM_OK;
}

int ksim_engine_get_reports(ksim_engine* e, int replica, ksim_report* out, int n) {
  if (!e || !out || replica < 0 || replica >= e->R || n < 0 || n > e->n_events[replica]) return KSIM_EINVAL;
  if (e->shard.world > 1) return KSIM_ENOTSUP;  // one shard's nodes only: ksim_engine_get_report_parts, merged
  if (!e->report || !e->d_rep[replica].p) return KSIM_ESTATE;
  std::vector<ksim_report_part> h((size_t)n);
  if (int rc = fetch_parts(e, e->d_rep[replica].p, h.data(), n, e->total_gpus[replica])) return rc;
  for (int i = 0; i < n; ++i) ksim_rep_host::part_reports(h[i], out + i, nullptr);
  return KSIM_OK;
}

int ksim_engine_get_power_reports(ksim_engine* e, int replica, ksim_power_report* out, int n) {
  if (!e || !out || replica < 0 || replica >= e->R || n < 0 || n > e->n_events[replica]) return KSIM_EINVAL;
  if (e->shard.world > 1) return KSIM_ENOTSUP;
  if (!e->report || !e->d_rep[replica].p || !e->pw_set[replica]) return KSIM_ESTATE;
  std::vector<ksim_report_part> h((size_t)n);
  if (int rc = fetch_parts(e, e->d_rep[replica].p, h.data(), n, e->total_gpus[replica])) return rc;
  for (int i = 0; i < n; ++i) ksim_rep_host::part_reports(h[i], nullptr, out + i);
  return KSIM_OK;
}

int ksim_engine_get_report_parts(ksim_engine* e, int replica, ksim_report_part* out, int n) {
  if (!e || !out || replica < 0 || replica >= e->R || n < 0 || n > e->n_events[replica]) return KSIM_EINVAL;
  if (!e->report || !e->rep_ready || !e->d_rep[replica].p) return KSIM_ESTATE;
  return fetch_parts(e, e->d_rep[replica].p, out, n, e->total_gpus[replica]);
}

int ksim_report_merge(const ksim_report_part* const* parts, int world, int n, ksim_report* out,
                      ksim_power_report* power_out) {
  return ksim_rep_host::merge(parts, world, n, out, power_out);
}

int ksim_shard_group_get_reports(ksim_engine* const* engines, int world, ksim_report* out, ksim_power_report* power_out,
                                 int n) {
  if (!engines || !out || world < 1 || world > 16 || n < 0) return KSIM_EINVAL;
  ksim_engine* e0 = engines[0];
  int64_t total = 0;
  bool ready = true, pw = true;
  for (int k = 0; k < world; ++k) {
    const ksim_engine* e = engines[k];
    if (!group_member_ok(engines, world, k)) return KSIM_EINVAL;
    ready = ready && e->report && e->rep_ready;
    pw = pw && e->pw_set[0];
    total += e->total_gpus[0];
  }
  if (!ready || e0->shard.group.rmerge_n < 0 || (power_out && !pw)) return KSIM_ESTATE;
  if (n > e0->shard.group.rmerge_n) return KSIM_EINVAL;
  std::vector<ksim_report_part> h((size_t)n);
  if (int rc = fetch_parts(e0, e0->shard.group.d_rmerge.p, h.data(), n, total)) return rc;
  for (int i = 0; i < n; ++i) ksim_rep_host::part_reports(h[i], out + i, power_out ? power_out + i : nullptr);
  return KSIM_OK;
}

int ksim_engine_last_report_ms(ksim_engine* e, double* ms) {
  if (!e || !ms) return KSIM_EINVAL;
  *ms = e->stats.report_ms;
  return KSIM_OK;
}

int ksim_engine_last_run_launches(ksim_engine* e, int* launches, int* side_streams) {
  if (!e || !launches || !side_streams) return KSIM_EINVAL;
  *launches = e->stats.launches;
  *side_streams = e->stats.streams;
  return KSIM_OK;
}

int ksim_engine_last_run_kernels(ksim_engine* e, char* out, int cap) {
  if (!e || !out || cap <= 0) return KSIM_EINVAL;
  const std::string& names = e->stats.kernels;
  if ((int)names.size() >= cap) return KSIM_ERANGE;
  std::memcpy(out, names.c_str(), names.size() + 1);
  return KSIM_OK;
}

int ksim_engine_last_run_gate(ksim_engine* e, int* gate, long long* timeouts) {
  if (!e || !gate || !timeouts) return KSIM_EINVAL;
  *gate = e->stats.gate;
  *timeouts = e->gate_timeouts;
  return KSIM_OK;
}

int ksim_engine_last_run_report_overlap(ksim_engine* e, int* replicas) {
  if (!e || !replicas) return KSIM_EINVAL;
  *replicas = e->stats.ovl;
  return KSIM_OK;
}

int ksim_engine_last_run_wgs(ksim_engine* e, int* wgs_per_replica) {
  if (!e || !wgs_per_replica) return KSIM_EINVAL;
  *wgs_per_replica = e->run_mode == 1 ? e->bpr : e->stats.K;
  return KSIM_OK;
}

int ksim_engine_last_run_path(ksim_engine* e, int* path) {
  if (!e || !path) return KSIM_EINVAL;
  *path = run_path(e->stats, e->R, e->run_mode, e->shard.on());
  return KSIM_OK;
}

int ksim_engine_time_steps(ksim_engine* e, int n_steps, double* mean_kernel_us) {
  if (!e || !mean_kernel_us || n_steps <= 0) return KSIM_EINVAL;
  for (int r = 0; r < e->R; ++r)
    if (e->reps[r].policy == POL_WEIGHTED) return KSIM_ENOTSUP;  // k_step has no weighted combination but PWR+FGD
  KSIM_HIP(hipSetDevice(e->device));
  std::vector<DevEvent> evs(2 * n_steps);
  for (DevEvent& x : evs)
    if (x.ensure()) return KSIM_EHIP;
  int rc = reset_state(e);
  if (rc) return rc;
  StepArgs a = base_args(e);
  a.rep_first = 0;
  a.base = nullptr;
  for (int i = 0; i < n_steps; ++i) {
    a.step_off = i;
    KSIM_HIP(hipEventRecord(evs[2 * i], e->stream));
    hipLaunchKernelGGL(k_step, dim3(e->bpr * e->R), dim3(kBlock), 0, e->stream, a, (const TypDev*)e->d_tp.p);
    if (any_pwr(e)) hipLaunchKernelGGL(k_step_pwr<false>, dim3(e->bpr * e->R), dim3(kBlock), 0, e->stream, a);
    KSIM_HIP(hipEventRecord(evs[2 * i + 1], e->stream));
  }
  KSIM_HIP(hipStreamSynchronize(e->stream));
  double tot = 0;
  for (int i = 0; i < n_steps; ++i) {
    float ms = 0;
    KSIM_HIP(hipEventElapsedTime(&ms, evs[2 * i], evs[2 * i + 1]));
    tot += ms;
  }
  *mean_kernel_us = tot * 1000.0 / n_steps;
  return KSIM_OK;
}

int ksim_engine_last_run_ms(ksim_engine* e, double* ms) {
  if (!e || !ms) return KSIM_EINVAL;
  *ms = e->stats.ms;
  return KSIM_OK;
}

int ksim_engine_last_run_steps(ksim_engine* e, int64_t* steps) {
  if (!e || !steps) return KSIM_EINVAL;
  *steps = e->stats.steps;
  return KSIM_OK;
}

int ksim_engine_get_results(ksim_engine* e, int replica, ksim_result* out, int n) {
  if (!e || !out || replica < 0 || replica >= e->R || n < 0 || n > e->n_events[replica]) return KSIM_EINVAL;
  if (n == 0) return KSIM_OK;
  KSIM_HIP(hipSetDevice(e->device));
  KSIM_HIP(hipMemcpyAsync(out, e->d_res[replica].p, sizeof(ResultDev) * n, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

int ksim_engine_get_nodes(ksim_engine* e, int replica, ksim_node* out) {
  if (!e || !out || replica < 0 || replica >= e->R) return KSIM_EINVAL;
  KSIM_HIP(hipSetDevice(e->device));
  std::vector<NodeRec> h(e->N);
  std::vector<uint16_t> tags(e->tags_stride);
  KSIM_HIP(hipMemcpyAsync(h.data(), e->reps[replica].nodes, sizeof(NodeRec) * e->N, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipMemcpyAsync(tags.data(), e->d_tags.p + (size_t)replica * e->tags_stride, sizeof(uint16_t) * e->tags_stride,
                          hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  if (e->h_nodes[replica].size() != (size_t)e->N) return KSIM_ESTATE;
  for (int i = 0; i < e->N; ++i) {
    ksim_node& o = out[i];
    const NodeRec& n = h[i];
    o = e->h_nodes[replica][i];  // static fields as given to set_nodes
    o.cpu_used_milli = o.cpu_alloc_milli - n.cpu_left;
    o.mem_used_mib = o.mem_alloc_mib - n.mem_left;
    o.pods_used = o.pods_alloc - n.pods_left;
    for (int g = 0; g < kMaxGpu; ++g) o.gpu_used_milli[g] = g < n.gpu_cnt ? kMilli - (int)n.gl[g] : 0;
    for (int k = 0; k < kNumTags; ++k) o.tag_count[k] = tags[(size_t)i * kTagStride + k];
  }
  return KSIM_OK;
}

}  // extern "C"

// What a descheduling policy kind gives the plan driver below: the tag of its plan, the bytes per node of its select
// kernel's tables, its victim record and where the plan (DeschedState) and a group's merge (ShardState::Group) keep
// those, its kernel arguments with its own fields set, its per-event and victim buffers of tot elements with their
// pointers in the arguments, the launch of its eval kernel, and its select kernel.
struct FragPolicy {
  using Args = ksim_ds::DsArgs;
  using V = ksim_victim;
  static constexpr DsPlan tag = kDsFrag;
  static constexpr int node_bytes = ksim_ds::kSelNodeBytes;
  static constexpr DevBuf<V> DeschedState::*vict = &DeschedState::vict;
  static constexpr DevBuf<V> ShardState::Group::*merged = &ShardState::Group::d_vmerge;
  static constexpr void (*select)(Args) = ksim_ds::k_desched_select;
  int policy;
  Args args() const {
    Args a = {};
    a.policy = policy;
    return a;
  }
  int ensure(DeschedState& ds, size_t tot, Args& a) const {
    int rc = ds.eval.ensure(tot);
    if (!rc) rc = ds.plist.ensure(tot);
    if (!rc) rc = ds.vict.ensure(tot);
    a.eval = ds.eval.p, a.plist = ds.plist.p, a.vict = ds.vict.p;
    return rc;
  }
  void eval(ksim_engine* e, dim3 grid, const Args& a) const {
    hipLaunchKernelGGL(ksim_ds::k_desched_eval, grid, dim3(ksim_ds::kEvalBlock), 0, e->stream, a, (const TypDev*)e->d_tp.p);
  }
};
struct CosPolicy {
  using Args = ksim_ds::CosArgs;
  using V = ksim_cos_victim;
  static constexpr DsPlan tag = kDsCos;
  static constexpr int node_bytes = ksim_ds::kCosNodeBytes;
  static constexpr DevBuf<V> DeschedState::*vict = &DeschedState::cvict;
  static constexpr DevBuf<V> ShardState::Group::*merged = &ShardState::Group::d_cmerge;
  static constexpr void (*select)(Args) = ksim_ds::k_cos_select;
  long long cpu_bar, gpu_bar;
  Args args() const {
    Args a = {};
    a.cpu_bar = cpu_bar;
    a.gpu_bar = gpu_bar;
    return a;
  }
  int ensure(DeschedState& ds, size_t tot, Args& a) const {
    int rc = ds.cos.ensure(tot);
    if (!rc) rc = ds.cvict.ensure(tot);
    a.rec = ds.cos.p, a.vict = ds.cvict.p;
    return rc;
  }
  void eval(ksim_engine* e, dim3 grid, const Args& a) const {
    hipLaunchKernelGGL(ksim_ds::k_cos_eval, grid, dim3(ksim_ds::kEvalBlock), 0, e->stream, a);
  }
};

// The descheduling plan of every replica from the last run's results and final node records (ksim_desched.hpp), for
// every policy, in three steps on the engine's stream, so that the shards of a group can take each step together
// (group_plan) and an engine by itself takes them in a row (desched_plan):
//   plan_eval    the buffers, mark, evaluate, and the bound-pod counts on their way to the host (no wait);
//   plan_select  once the stream has been waited for: the budgets on the host (ksim_desched_host.hpp), select, and
//                the victim counts on their way to the host;
//   plan_finish  the wait, the plan's time and its tag.
// A node-sharded engine makes its part: mark and eval under the ownership rule (eval_bound_node), so the bound pods
// are those on its own nodes, and select capped at budget(ratio, creation events of its stream) -- the same number on
// every shard and, bound <= creations, never below the cluster's budget, which no shard knows: its list then holds
// every entry the merge can take from it (DESIGN.md "Descheduling on shards").
template <class P>
static int plan_eval(ksim_engine* e, const P& pol, typename P::Args& a) {
  if (!e->ran) return KSIM_ESTATE;
  DeschedState& ds = e->ds;
  ds.invalidate();
  KSIM_HIP(hipSetDevice(e->device));
  const int R = e->R;
  const int max_ev = ksim_ds_host::event_offsets(e->n_events.data(), R, ds.eoff);
  const size_t tot = (size_t)ds.eoff[R];
  int rc = pol.ensure(ds, tot, a);
  if (!rc) rc = ds.gone.ensure(tot);
  if (!rc) rc = ds.cnt.ensure((size_t)3 * R);
  if (!rc) rc = ds.d_eoff.upload(ds.eoff, e->stream);
  const size_t tab = (size_t)e->N * P::node_bytes;
  const bool in_lds = tab <= (size_t)ksim_ds::kSelLdsBytes;
  if (!rc && !in_lds) rc = ds.tab.ensure(ksim_ds::tab_stride(e->N, P::node_bytes) * R);
  if (rc) return rc;
  if (ds.ev0.ensure() || ds.ev1.ensure()) return KSIM_EHIP;
  a.reps = e->d_reps.p;
  a.eoff = ds.d_eoff.p;
  a.gone = ds.gone.p;
  a.bound = ds.cnt.p;
  a.budget = ds.cnt.p + R;
  a.n_vict = ds.cnt.p + 2 * R;
  a.tab = in_lds ? nullptr : ds.tab.p;
  a.N = e->N;
  a.node_off = e->shard.on() ? e->shard.node_off : 0;
  a.sharded = e->shard.on() ? 1 : 0;
  KSIM_HIP(hipEventRecord(ds.ev0, e->stream));
  if (tot) KSIM_HIP(hipMemsetAsync(ds.gone.p, 0, tot, e->stream));
  KSIM_HIP(hipMemsetAsync(ds.cnt.p, 0, sizeof(int32_t) * 3 * R, e->stream));
  if (max_ev > 0) {
    const dim3 grid((unsigned)((max_ev + ksim_ds::kEvalBlock - 1) / ksim_ds::kEvalBlock), (unsigned)R);
    hipLaunchKernelGGL(ksim_ds::k_desched_mark, grid, dim3(ksim_ds::kEvalBlock), 0, e->stream, (ksim_ds::PlanArgs)a);
    KSIM_HIP(hipGetLastError());
    pol.eval(e, grid, a);
    KSIM_HIP(hipGetLastError());
  }
  ds.bound.assign((size_t)R, 0);
  KSIM_HIP(hipMemcpyAsync(ds.bound.data(), a.bound, sizeof(int32_t) * R, hipMemcpyDeviceToHost, e->stream));
  return KSIM_OK;
}

template <class P>
static int plan_select(ksim_engine* e, double ratio, const typename P::Args& a) {
  DeschedState& ds = e->ds;
  KSIM_HIP(hipSetDevice(e->device));
  const int R = e->R;
  ds.ratio = ratio;
  ds.budget.assign((size_t)R, 0);
  for (int r = 0; r < R; ++r) ds.budget[r] = ksim_ds_host::budget(ratio, e->shard.on() ? e->n_create[r] : ds.bound[r]);
  KSIM_HIP(hipMemcpyAsync(ds.cnt.p + R, ds.budget.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, e->stream));
  const size_t tab = (size_t)e->N * P::node_bytes;
  hipLaunchKernelGGL(P::select, dim3((unsigned)R), dim3(ksim_ds::kSelBlock), a.tab ? (size_t)0 : tab, e->stream, a);
  KSIM_HIP(hipGetLastError());
  ds.nv.assign((size_t)R, 0);
  KSIM_HIP(hipMemcpyAsync(ds.nv.data(), a.n_vict, sizeof(int32_t) * R, hipMemcpyDeviceToHost, e->stream));
  KSIM_HIP(hipEventRecord(ds.ev1, e->stream));
  return KSIM_OK;
}

static int plan_finish(ksim_engine* e, DsPlan tag) {
  DeschedState& ds = e->ds;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  float ms = 0;
  KSIM_HIP(hipEventElapsedTime(&ms, ds.ev0, ds.ev1));
  ds.last_ms = ms;
  ds.plan = tag;
  return KSIM_OK;
}

template <class P>
static int desched_plan(ksim_engine* e, const P& pol, double ratio) {
  typename P::Args a = pol.args();
  int rc = plan_eval(e, pol, a);
  if (rc) return rc;
  KSIM_HIP(hipStreamSynchronize(e->stream));
  if ((rc = plan_select<P>(e, ratio, a))) return rc;
  return plan_finish(e, P::tag);
}

// A replica's victims of the plan of P's kind, which the engine must hold.  `part`: the engine's own list with the
// pods bound on its nodes (ksim_engine_get_victim_part: on a shard its part, else the plan itself); otherwise the
// plan with its budget, which a shard does not have -- its list is not the cluster's plan and may run past the
// cluster's budget (KSIM_ENOTSUP).
template <class P>
static int plan_victims(ksim_engine* e, int replica, typename P::V* out, int cap, int* n_out, int* budget_out,
                        int64_t* bound_out, bool part) {
  if (!e || replica < 0 || replica >= e->R || cap < 0 || !n_out) return KSIM_EINVAL;
  if (!part && e->shard.on()) return KSIM_ENOTSUP;
  const DeschedState& ds = e->ds;
  if (ds.plan != P::tag) return KSIM_ESTATE;
  const int n = ds.nv[replica];
  *n_out = n;
  if (budget_out) *budget_out = ds.budget[replica];
  if (bound_out) *bound_out = ds.bound[replica];
  if (cap < n) return KSIM_ERANGE;
  if (n == 0) return KSIM_OK;
  if (!out) return KSIM_EINVAL;
  KSIM_HIP(hipSetDevice(e->device));
  KSIM_HIP(hipMemcpyAsync(out, (ds.*P::vict).p + ds.eoff[replica], sizeof(typename P::V) * n, hipMemcpyDeviceToHost,
                          e->stream));
  KSIM_HIP(hipStreamSynchronize(e->stream));
  return KSIM_OK;
}

static int group_check(ksim_engine* const* engines, int world) {
  if (!engines || world < 1 || world > 16) return KSIM_EINVAL;
  for (int k = 0; k < world; ++k)
    if (!group_member_ok(engines, world, k)) return KSIM_EINVAL;
  return KSIM_OK;
}

// The plan of an in-process group: every shard's part, each step of the driver on all shards before the next (the
// shards' kernels are independent and sit on their own streams), the bound counts summed on the host, the cluster's
// budget, then the merge of the shards' lists into engine 0's merged list (k_victim_merge) on engine 0's stream.
// Engine 0's plan time spans the parts and the merge; KSIM_GROUP_TIMES=1 prints the merge's share on stderr.
template <class P>
static int group_plan(ksim_engine* const* engines, int world, const P& pol, double ratio) {
  using V = typename P::V;
  ksim_engine* e0 = engines[0];
  ShardState::Group& g = e0->shard.group;
  g.dplan = kDsNone;
  for (int k = 0; k < world; ++k)
    if (!engines[k]->ran) return KSIM_ESTATE;
  std::vector<typename P::Args> as((size_t)world, pol.args());
  int rc;
  for (int k = 0; k < world; ++k)
    if ((rc = plan_eval(engines[k], pol, as[k]))) return rc;
  for (int k = 0; k < world; ++k) KSIM_HIP(hipStreamSynchronize(engines[k]->stream));
  for (int k = 0; k < world; ++k)
    if ((rc = plan_select<P>(engines[k], ratio, as[k]))) return rc;
  for (int k = 0; k < world; ++k)
    if ((rc = plan_finish(engines[k], P::tag))) return rc;
  ksim_ds::MergeArgs<V> ma = {};
  int64_t bound = 0, total = 0;
  for (int k = 0; k < world; ++k) {
    const DeschedState& ds = engines[k]->ds;
    const int n = (int)std::min<long long>(std::max(ds.nv[0], 0), ds.eoff[1]);  // inside the shard's victim buffer
    ma.part[k] = (ds.*P::vict).p;
    ma.n[k] = n;
    bound += ds.bound[0];
    total += n;
  }
  if (bound > (int64_t)std::numeric_limits<int32_t>::max()) return KSIM_ERANGE;
  const int32_t budget = ksim_ds_host::budget(ratio, (int32_t)bound);
  const int take = (int)std::min<int64_t>(total, budget);
  DevBuf<V>& merged = g.*P::merged;
  if ((rc = merged.ensure((size_t)std::max(take, 1)))) return rc;
  if ((rc = g.d_nmerge.ensure(1))) return rc;
  if ((rc = g.d_margs.ensure(sizeof ma))) return rc;
  ma.world = world;
  ma.budget = budget;
  ma.out = merged.p;
  ma.out_cap = take;
  ma.n_out = g.d_nmerge.p;
  KSIM_HIP(hipSetDevice(e0->device));
  hipStream_t st = e0->stream;
  const bool times = read_env().group_times;
  if (times) {
    if ((rc = e0->tev_fork.ensure())) return rc;
    KSIM_HIP(hipEventRecord(e0->tev_fork, st));
  }
  const unsigned blocks = (unsigned)std::max<int64_t>(1, (total + ksim_ds::kMergeBlock - 1) / ksim_ds::kMergeBlock);
  KSIM_HIP(hipMemcpyAsync(g.d_margs.p, &ma, sizeof ma, hipMemcpyHostToDevice, st));  // (ma lives past the wait below)
  hipLaunchKernelGGL((ksim_ds::k_victim_merge<V>), dim3(blocks), dim3(ksim_ds::kMergeBlock), 0, st,
                     (const ksim_ds::MergeArgs<V>*)g.d_margs.p);
  KSIM_HIP(hipGetLastError());
  int32_t n_merged = -1;
  KSIM_HIP(hipMemcpyAsync(&n_merged, g.d_nmerge.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  KSIM_HIP(hipEventRecord(e0->ds.ev1, st));
  KSIM_HIP(hipStreamSynchronize(st));
  if (n_merged != take) return KSIM_ESTATE;
  float ms = 0, mms = 0;
  KSIM_HIP(hipEventElapsedTime(&ms, e0->ds.ev0, e0->ds.ev1));
  e0->ds.last_ms = ms;
  if (times && hipEventElapsedTime(&mms, e0->tev_fork, e0->ds.ev1) == hipSuccess)
    std::fprintf(stderr, "ksim group deschedule times (ms): %d shards' parts %.3f; merge %.3f\n", world, ms - mms, mms);
  g.dgen.resize((size_t)world);
  for (int k = 0; k < world; ++k) g.dgen[k] = engines[k]->ds.gen;
  g.dmerge_n = take;
  g.dbudget = budget;
  g.dplan = P::tag;
  return KSIM_OK;
}

// The merged list of the group's last plan, which must be of P's kind and made from the plans the shards still hold.
template <class P>
static int group_victims(ksim_engine* const* engines, int world, typename P::V* out, int cap, int* n_out,
                         int* budget_out) {
  if (int rc = group_check(engines, world)) return rc;
  if (cap < 0 || !n_out) return KSIM_EINVAL;
  ksim_engine* e0 = engines[0];
  const ShardState::Group& g = e0->shard.group;
  if (g.dplan != P::tag || g.dgen.size() != (size_t)world) return KSIM_ESTATE;
  for (int k = 0; k < world; ++k)
    if (engines[k]->ds.plan != P::tag || engines[k]->ds.gen != g.dgen[k]) return KSIM_ESTATE;
  const int n = g.dmerge_n;
  *n_out = n;
  if (budget_out) *budget_out = g.dbudget;
  if (cap < n) return KSIM_ERANGE;
  if (n == 0) return KSIM_OK;
  if (!out) return KSIM_EINVAL;
  KSIM_HIP(hipSetDevice(e0->device));
  KSIM_HIP(hipMemcpyAsync(out, (g.*P::merged).p, sizeof(typename P::V) * n, hipMemcpyDeviceToHost, e0->stream));
  KSIM_HIP(hipStreamSynchronize(e0->stream));
  return KSIM_OK;
}

static bool frag_policy_ok(int policy) {
  return policy == KSIM_DESCHED_FRAG_ONE_POD || policy == KSIM_DESCHED_FRAG_MULTI_POD;
}

extern "C" {

int ksim_engine_deschedule(ksim_engine* e, int policy, double ratio) {
  if (check_gfx950(e ? e->device : 0)) return KSIM_ENODEV;
  if (!e) return KSIM_EINVAL;
  if (!frag_policy_ok(policy)) return KSIM_EINVAL;
  if (!(ratio >= 0.0)) return KSIM_EINVAL;  // negative or NaN
  return desched_plan(e, FragPolicy{policy}, ratio);
}

int ksim_engine_get_victims(ksim_engine* e, int replica, ksim_victim* out, int cap, int* n_out, int* budget_out) {
  return plan_victims<FragPolicy>(e, replica, out, cap, n_out, budget_out, nullptr, false);
}

int ksim_engine_get_victim_part(ksim_engine* e, ksim_victim* out, int cap, int* n_out, int64_t* bound_out) {
  return plan_victims<FragPolicy>(e, 0, out, cap, n_out, nullptr, bound_out, true);
}

int ksim_engine_deschedule_cossim(ksim_engine* e, double ratio, int64_t cpu_bar_milli, int64_t gpu_bar_milli) {
  if (check_gfx950(e ? e->device : 0)) return KSIM_ENODEV;
  if (!e) return KSIM_EINVAL;
  if (!(ratio >= 0.0) || cpu_bar_milli < 0 || gpu_bar_milli < 0) return KSIM_EINVAL;
  return desched_plan(e, CosPolicy{(long long)cpu_bar_milli, (long long)gpu_bar_milli}, ratio);
}

int ksim_engine_get_cos_victims(ksim_engine* e, int replica, ksim_cos_victim* out, int cap, int* n_out,
                                int* budget_out) {
  return plan_victims<CosPolicy>(e, replica, out, cap, n_out, budget_out, nullptr, false);
}

int ksim_engine_get_cos_victim_part(ksim_engine* e, ksim_cos_victim* out, int cap, int* n_out, int64_t* bound_out) {
  return plan_victims<CosPolicy>(e, 0, out, cap, n_out, nullptr, bound_out, true);
}

int ksim_engine_last_deschedule_ms(ksim_engine* e, double* ms) {
  if (!e || !ms) return KSIM_EINVAL;
  *ms = e->ds.last_ms;
  return KSIM_OK;
}

int ksim_desched_merge(const ksim_victim* const* parts, const int* n, const int64_t* bound, int world, double ratio,
                       ksim_victim* out, int cap, int* n_out, int* budget_out) {
  return ksim_ds_host::merge_victims(parts, n, bound, world, ratio, out, cap, n_out, budget_out);
}

int ksim_cos_merge(const ksim_cos_victim* const* parts, const int* n, const int64_t* bound, int world, double ratio,
                   ksim_cos_victim* out, int cap, int* n_out, int* budget_out) {
  return ksim_ds_host::merge_cos_victims(parts, n, bound, world, ratio, out, cap, n_out, budget_out);
}

int ksim_shard_group_deschedule(ksim_engine* const* engines, int world, int policy, double ratio) {
  if (int rc = group_check(engines, world)) return rc;
  if (!frag_policy_ok(policy) || !(ratio >= 0.0)) return KSIM_EINVAL;
  if (check_gfx950(engines[0]->device)) return KSIM_ENODEV;
  return group_plan(engines, world, FragPolicy{policy}, ratio);
}

int ksim_shard_group_deschedule_cossim(ksim_engine* const* engines, int world, double ratio, int64_t cpu_bar_milli,
                                       int64_t gpu_bar_milli) {
  if (int rc = group_check(engines, world)) return rc;
  if (!(ratio >= 0.0) || cpu_bar_milli < 0 || gpu_bar_milli < 0) return KSIM_EINVAL;
  if (check_gfx950(engines[0]->device)) return KSIM_ENODEV;
  return group_plan(engines, world, CosPolicy{(long long)cpu_bar_milli, (long long)gpu_bar_milli}, ratio);
}

int ksim_shard_group_get_victims(ksim_engine* const* engines, int world, ksim_victim* out, int cap, int* n_out,
                                 int* budget_out) {
  return group_victims<FragPolicy>(engines, world, out, cap, n_out, budget_out);
}

int ksim_shard_group_get_cos_victims(ksim_engine* const* engines, int world, ksim_cos_victim* out, int cap, int* n_out,
                                     int* budget_out) {
  return group_victims<CosPolicy>(engines, world, out, cap, n_out, budget_out);
}

}  // extern "C"
