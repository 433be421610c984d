// ksim_wsum.hpp -- weighted combinations of score plugins, replayed on the device (k_wsum).
//
// The reference's harness gives every score plugin an integer weight (generate_config_and_run.py:74-75,243-245) and
// the framework scores every feasible node with every enabled plugin, runs each plugin's NormalizeScore, range-checks
// the result to 0..100, multiplies by the weight and sums (framework.go:635-710, generic_scheduler.go:511-519).
// k_wsum replays a replica under any such weight vector over FGD, BestFit, DotProduct, GpuPacking, GpuClustering and
// PWR (POL_WEIGHTED; Random's PreScore pick is not reproducible and stays out of combinations).
//
// One 1024-thread workgroup per replica (K = 1: no cross-workgroup exchange, a plain launch), the whole cluster's
// node records in LDS, the whole event stream in one launch.  Thread t owns the node slots t, t + 1024, ...
// Per creation event:
//   1. scan: Filter (filter_node) and the raw Score of every enabled plugin on the thread's slots, with the device
//      functions every other kernel uses (bestfit_score, dotprod_cfg_score / dotprod_merge_max, packing_score,
//      clustering_score, pwr_score; FGD: frag_F of the node's current state -- cached per slot, a Bind or a delete
//      invalidates it -- and of one candidate per GPU value class or the NodeResource.Sub state, fgd_frag_score,
//      the lowest GPU index reaching the max: emit_fgd_items' candidates and finalize_fgd's rule).  The raw scores
//      of a slot wait in LDS (sc[slot]);
//   2. block reduction (DPP within the waves, one LDS partial per wave): the feasible count, the any-Score-error
//      flag, and the min / max raw score of BestFit and of PWR over the feasible nodes -- both NormalizeScores need
//      the cluster's range before any node's total exists;
//   3. barrier; every thread forms its slots' totals with wsum_total (ksim_device.hpp: the same function the CPU
//      tests run), packs the key (total, name rank, the selector's GPU, slot) and the block takes the max:
//      selectHost, ties to the smallest node name (generic_scheduler.go:187-212);
//   4. barrier; wave 0 takes the cycle's decision as finish_cycle does -- no feasible node: unschedulable; one: it
//      wins with score 0 whatever its plugins say (generic_scheduler.go:158-164); a Score error or a score outside
//      0..100 on any feasible node: KSIM_ERROR, nothing bound (framework.go:650-667, 686-704) -- then Reserve's GPU
//      selector on the winner (select_gpus), the Bind (apply_bind), the result row and the report's stores;
//   5. barrier (the winner's slot belongs to another thread's next scan).
// Delete events (kGeneral) undo the creation's Bind from its own result row; a delete of a failed creation changes
// nothing.  With the cluster report on, a Bind / delete stores the node's new record and the previous event that
// changed the node (snap / prev), as k_replay's general form does, so k_report_delta / k_report_scan run unchanged.
//
// Templated on what is expensive to carry when absent: kFgd (some replica of the launch weighs FGD: the F cache
// and the fp64 evaluation), kPwr (the energy model), kGeneral (deletes, report stores).  The cheap plugins are a
// runtime mask.  The weights travel in the kernel's own argument table, not in ReplicaDev.
#pragma once

namespace ksim_wsum {

using namespace ksim;
using ksim_plan::wsum::kBlock;
using ksim_plan::wsum::WLayout;
using ksim_plan::wsum::wsum_layout;
constexpr int kWaves = kBlock / 64;
constexpr int kEvBuf = 128;
constexpr int kWStride = 8;  // ints per replica in WsumArgs::w: the kNumPlugins weights, then the plugin mask

struct WsumArgs {
  ReplicaDev* reps;
  const int* rep_list;  // replica of each workgroup
  const int* w;         // [R][kWStride] by replica id
  int N;
  unsigned lmask;       // the union of the launch's plugin masks: the LDS layout (wsum_layout)
};

struct __align__(16) WsumPart {  // one wave's share of a step
  unsigned long long key;        // its best packed key (0: nothing feasible)
  int cnt, err;                  // feasible nodes; a feasible node's Score failed or left 0..100
  int bf_lo, bf_hi, pw_lo, pw_hi;  // raw score ranges over the feasible nodes (the two NormalizeScores)
};

struct __align__(16) WsumShared {
  PodDev ev[kEvBuf];
  WsumPart part[kWaves];
  PowerDev pw;  // kPwr: the replica's energy model
};
static_assert(sizeof(WsumShared) % 16 == 0, "keep the node records 16-B aligned");
static_assert(sizeof(WsumShared) == ksim_plan::wsum::kSharedBytes,
              "wsum_layout (ksim_plan.hpp) starts the regions after WsumShared");

// sc[slot].x: FGD score [0,7) | GpuPacking score [7,14) | GpuClustering score [14,21) | feasible 21 | Score error 22 |
// the selector's GPU + 1 [23,27); .y DotProduct's score; .z BestFit's raw score; .w PWR's raw score
constexpr int kScFeas = 1 << 21, kScErr = 1 << 22;

template <bool kFgd, bool kPwr, bool kGeneral>
__global__ __launch_bounds__(kBlock) void k_wsum(WsumArgs a, const TypDev* __restrict__ tp_all) {
  using namespace ksim_replay;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int r = a.rep_list[blockIdx.x];
  const ReplicaDev rp = a.reps[r];
  const TypDev* __restrict__ tp = tp_all + (size_t)r * kMaxTypical;
  const int N = a.N;
  const bool ltags = (a.lmask >> POL_CLUSTERING) & 1u;  // the tag counts live in LDS (else in HBM, by atomics)
  const WLayout L = wsum_layout(N, a.lmask, kGeneral);
  WsumShared& sh = *reinterpret_cast<WsumShared*>(smem);
  NodeRec* s_nodes = reinterpret_cast<NodeRec*>(smem + L.nodes);
  int4* s_sc = reinterpret_cast<int4*>(smem + L.sc);
  uint16_t* s_tags = reinterpret_cast<uint16_t*>(smem + L.tags);
  double* s_F0 = reinterpret_cast<double*>(smem + L.F0);
  int* s_last = reinterpret_cast<int*>(smem + L.last);
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;

  int w[kNumPlugins];
#pragma unroll
  for (int p = 0; p < kNumPlugins; ++p) w[p] = __builtin_amdgcn_readfirstlane(a.w[(size_t)r * kWStride + p]);
  const bool on_fgd = kFgd && w[POL_FGD] > 0, on_bf = w[POL_BESTFIT] > 0, on_dp = w[POL_DOTPROD] > 0;
  const bool on_pk = w[POL_PACKING] > 0, on_cl = w[POL_CLUSTERING] > 0, on_pw = kPwr && w[POL_PWR] > 0;
  const bool dp_mm = rp.dpcfg == (DIM_MERGE | NORM_MAX << 4);
  const bool dp_cap = dp_norm(rp.dpcfg) == NORM_NODE;

  for (int i = tid; i < N; i += kBlock) store_node(&s_nodes[i], load_node(rp.nodes + i));
  if (ltags)
    for (int i = tid; i < N * (kTagStride / 2); i += kBlock)
      reinterpret_cast<uint32_t*>(s_tags)[i] = reinterpret_cast<const uint32_t*>(rp.tags)[i];
  if (kFgd)
    for (int i = tid; i < N; i += kBlock) s_F0[i] = -1.0;
  if (kGeneral)
    for (int i = tid; i < N; i += kBlock) s_last[i] = -1;
  if (kPwr)
    for (int i = tid; i < (int)(sizeof(PowerDev) / 4); i += kBlock)
      reinterpret_cast<uint32_t*>(&sh.pw)[i] = reinterpret_cast<const uint32_t*>(rp.pw)[i];
  __syncthreads();

  for (int step = 0; step < rp.n_events; ++step) {
    const int eb = step & (kEvBuf - 1);
    if (eb == 0) {
      const int nl = min(kEvBuf, rp.n_events - step) * 2;
      const uint4* src = reinterpret_cast<const uint4*>(rp.ev + step);
      for (int i = tid; i < nl; i += kBlock) reinterpret_cast<uint4*>(sh.ev)[i] = src[i];
      __syncthreads();  // (the step's last barrier keeps the old window until every wave has left it)
    }
    const PodDev p = uniform_pod(&sh.ev[eb]);

    if (kGeneral && (p.flags & kPodDelete)) {
      // simulator.go:416-422 deletePod -> removePod: undo the creation's Bind from its own result row (thread 0
      // writes every result row, so it reads its own store); a delete of a failed creation changes nothing
      if (tid == 0) {
        ResultDev out{-1, 0, 0, 0, ST_DELETED};
        if (p.ref >= 0 && p.ref < step) {
          const ResultDev c = rp.res[p.ref];
          if (c.node >= 0 && c.node < N && c.status == ST_OK) {
            PodDev cp = rp.ev[p.ref];
            if (!ltags && cp.tag >= 0) {  // the HBM counts: an atomic, not a read-modify-write
              tag_add(rp.tags + (size_t)c.node * kTagStride, cp.tag, -1);
              cp.tag = -1;
            }
            apply_bind(&s_nodes[c.node], ltags ? &s_tags[(size_t)c.node * kTagStride] : nullptr, cp, c.gpu_mask, -1);
            if (kFgd) s_F0[c.node] = -1.0;
            if (rp.snap) {
              store_node(rp.snap + step, load_node(&s_nodes[c.node]));
              rp.prev[step] = s_last[c.node];
              s_last[c.node] = step;
            }
            out.node = c.node;
            out.gpu_mask = c.gpu_mask;
          }
        }
        rp.res[step] = out;
      }
      __syncthreads();
      continue;
    }

    // ---- 1. scan: Filter and the raw scores of this thread's slots
    const bool share = is_share_pod(p);
    int cnt = 0, bf_lo = 0x7fffffff, bf_hi = (int)0x80000000, pw_lo = 0x7fffffff, pw_hi = (int)0x80000000;
    bool err = false;
    for (int i = tid; i < N; i += kBlock) {
      const NodeV n = load_node(&s_nodes[i]);
      if (!filter_node(n, p)) {
        s_sc[i] = make_int4(0, 0, 0, 0);
        continue;
      }
      const int total = n.total();
      bool e1 = false;
      int s_fgd = 0, s_pk = 0, s_cl = 0, s_dp = 0, s_bf = 0, s_pw = 0, g_fgd = -1, g_pw = -1;
      if (on_bf) {  // getBestFitScore: -1 is its Score error (best_fit_score.go:48-51)
        s_bf = bestfit_score(n, p, total);
        e1 = e1 || s_bf == -1;
      }
      if (on_dp) {  // no Score error of its own: the framework's range check decides (wsum_total)
        int gid = 0;
        s_dp = dp_mm ? dotprod_merge_max(n, p) : dotprod_cfg_score(n, p, dp_cap ? rp.cap[i] : 0, rp.dpcfg, &gid);
      }
      if (on_pk) {
        bool perr = false;
        s_pk = p.milli <= 0 ? 0 : packing_score(n, p, &perr);
        e1 = e1 || perr;
      }
      if (on_cl) {
        if (p.tag == -2) e1 = true;  // the reference panics on the pod's GPU request
        else s_cl = clustering_score(&s_tags[(size_t)i * kTagStride], p.tag, total);
      }
      if (kPwr && on_pw) {
        bool perr = false;
        s_pw = pwr_score(n, p, rp.cap[i], rp.cpum[i], sh.pw, &g_pw, &perr);  // *err: no energy model for the node
        e1 = e1 || perr;
      }
      if (kFgd && on_fgd) {
        // fgd_score.go:99-149: F of the current state and of every candidate placement -- one per DISTINCT
        // milli-left value among the fitting GPUs (share pods; frag.go reads the multiset only) or the
        // NodeResource.Sub state -- the max sigmoid score, the lowest GPU index reaching it
        int gl[kMaxGpu];
        unpack_gl(n, gl);
        const int gcnt = n.gpu_cnt();
        const uint32_t tb = 1u << n.gpu_type();
        double F0 = s_F0[i];
        unsigned todo = (F0 < 0 ? 1u : 0u) | (share ? first_of_class(n, p.milli) << 1 : 1u << 9);
        int best = -1, bs = 0;
#pragma unroll 1
        while (todo) {
          const int code = __builtin_ctz(todo);  // 0 current state, 1..8 the share on GPU code-1, 9 Sub
          todo &= todo - 1;
          int cpuL = n.cpu_left;
          unsigned m = code >= 1 && code <= 8 ? 1u << (code - 1) : 0u;
          if (code == 9) {
            bool ok = false;
            m = sub_gpu_mask(gl, gcnt, cpuL, p, &ok);
            if (!ok) m = 0u;
            if (ok) cpuL -= p.cpu_nz;
          } else if (code != 0) {
            cpuL -= p.cpu_nz;
          }
          int c[kMaxGpu];
#pragma unroll
          for (int h = 0; h < kMaxGpu; ++h) c[h] = gl[h] - (((m >> h) & 1u) ? (int)p.milli : 0);
          const double F = rp.typed ? frag_F<true>(cpuL, c, tb, tp, rp.ncpu, rp.nt) : frag_F<false>(cpuL, c, tb, tp, rp.ncpu, rp.nt);
          if (code == 0) {
            F0 = F;
            s_F0[i] = F;
          } else {
            const int fs = fgd_frag_score(F0, F);
            if (best < 0 || fs > bs) { bs = fs; best = code - 1; }
          }
        }
        s_fgd = bs;
        g_fgd = share ? best : -1;
      }
      const int gsel = rp.gpusel == SEL_FGD ? g_fgd : rp.gpusel == SEL_PWR ? g_pw : -1;
      s_sc[i] = make_int4(s_fgd | s_pk << 7 | s_cl << 14 | kScFeas | (e1 ? kScErr : 0) | ((gsel + 1) & 15) << 23, s_dp, s_bf, s_pw);
      ++cnt;
      err = err || e1;
      bf_lo = min(bf_lo, s_bf); bf_hi = max(bf_hi, s_bf);
      pw_lo = min(pw_lo, s_pw); pw_hi = max(pw_hi, s_pw);
    }
    // ---- 2. block reduction of the counts and the two raw ranges
    cnt = wave_sum_dpp(cnt);
    const bool werr = __any(err);
    bf_lo = wave_min_dpp(bf_lo); bf_hi = wave_max_dpp(bf_hi);
    pw_lo = wave_min_dpp(pw_lo); pw_hi = wave_max_dpp(pw_hi);
    if (lane == 0) {
      WsumPart& q = sh.part[wv];
      q.cnt = cnt; q.err = werr ? 1 : 0;
      q.bf_lo = bf_lo; q.bf_hi = bf_hi; q.pw_lo = pw_lo; q.pw_hi = pw_hi;
    }
    __syncthreads();
    int nfeas = 0;  // (err is read in step 4 only: step 3 may still add to it)
    bf_lo = pw_lo = 0x7fffffff;
    bf_hi = pw_hi = (int)0x80000000;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const WsumPart& q = sh.part[k];
      nfeas += q.cnt;
      bf_lo = min(bf_lo, q.bf_lo); bf_hi = max(bf_hi, q.bf_hi);
      pw_lo = min(pw_lo, q.pw_lo); pw_hi = max(pw_hi, q.pw_hi);
    }
    // ---- 3. the totals (NormalizeScore, range check, weights: wsum_total) and the block argmax
    unsigned long long best = 0ull;
    bool rerr = false;
    if (nfeas > 0) {
      for (int i = tid; i < N; i += kBlock) {
        const int4 v = s_sc[i];
        if (!(v.x & kScFeas)) continue;
        const int raw[kNumPlugins] = {v.x & 127, v.z, v.y, (v.x >> 7) & 127, (v.x >> 14) & 127, 0, v.w};
        bool e2 = false;
        int tot = wsum_total(raw, bf_lo, bf_hi, pw_lo, pw_hi, w, &e2);
        if (e2 || (v.x & kScErr)) tot = 0;  // (the cycle aborts unless this is the only feasible node)
        rerr = rerr || e2;
        const unsigned long long k = pack_key((unsigned)tot, s_nodes[i].name_rank, ((v.x >> 23) & 15) - 1, i);
        best = k > best ? k : best;
      }
    }
    best = wave_max_u64_dpp(best);
    const bool wrerr = __any(rerr);
    if (lane == 0) {
      sh.part[wv].key = best;
      if (wrerr) sh.part[wv].err = 1;
    }
    __syncthreads();
    // ---- 4. the decision and the winner: wave 0 (uniform values; lane 0 stores)
    if (wv == 0) {
      unsigned long long W = 0ull;
      int gerr = 0;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) {
        W = sh.part[k].key > W ? sh.part[k].key : W;
        gerr |= sh.part[k].err;
      }
      ResultDev out{-1, 0, 0, nfeas, ST_UNSCHED};
      if (nfeas > 0) {
        out.status = (nfeas > 1 && gerr) ? ST_ERROR : ST_OK;  // framework.go:650-667, 686-704: the cycle aborts
        if (out.status == ST_OK) {
          out.score = nfeas <= 1 ? 0 : (long long)key_score(W);  // generic_scheduler.go:158-164: one node, score 0
          const int loc = key_loc(W);
          NodeRec* nr = &s_nodes[loc];
          const NodeV wn = uniform_node(nr);
          const int mask = select_gpus(wn, p, rp.gpusel, sel_arg(rp, wn, p, loc, key_gpu(W)), rp.seed, step);
          if (mask < 0) {  // Reserve failed: allocateGpuId returned "" / panicked
            out.status = ST_ERROR;
            out.score = 0;
          } else {
            if (lane == 0) {
              PodDev bp = p;
              if (!ltags && bp.tag >= 0) {
                tag_add(rp.tags + (size_t)loc * kTagStride, bp.tag, +1);
                bp.tag = -1;
              }
              apply_bind(nr, ltags ? &s_tags[(size_t)loc * kTagStride] : nullptr, bp, mask, +1);
              if (kFgd) s_F0[loc] = -1.0;
              if (kGeneral && rp.snap) {  // cluster report: the state this event left, the previous change of the node
                store_node(rp.snap + step, load_node(nr));
                rp.prev[step] = s_last[loc];
                s_last[loc] = step;
              }
            }
            out.node = loc;
            out.gpu_mask = mask;
          }
        }
      }
      if (lane == 0) rp.res[step] = out;
    }
    __syncthreads();
  }
  for (int i = tid; i < N; i += kBlock) store_node(rp.nodes + i, load_node(&s_nodes[i]));
  if (ltags)
    for (int i = tid; i < N * (kTagStride / 2); i += kBlock)
      reinterpret_cast<uint32_t*>(rp.tags)[i] = reinterpret_cast<const uint32_t*>(s_tags)[i];
}

}  // namespace ksim_wsum
