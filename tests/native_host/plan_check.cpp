// plan_check -- the FGD memo planners of ksim_plan.hpp on the CPU: invariants of memo_plan / hmemo_plan / memo_events
// over seeded random inputs, the plans of the bench's C2 job and C5's slices against the values the engine printed on
// the GPU (profiles/r08/memo/parent_memo_prof.log, profiles/r04/hmemo/prof_rm5_gkey.log, profiles/r05/hmemo/), the
// slice geometry against the formulas the three call sites had, and memo_form / hmemo_form over every input against
// the nested conditionals they replaced.  The run plan (make_run_plan): the nine cases of tests/test_gpu_run_plan.py
// as inputs with their plans written out, invariants over seeded random inputs, and choose_wgs / replay_fit /
// replay_narrow / the node-sharded runs' slices against the formulas the engine had.  Host code only: no device, no
// HIP call.  Aborts on the first broken expectation; prints one tally line per group, then "ok".
//
// usage: plan_check <node csv> <pod csv>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <tuple>

#include "ksim_plan.hpp"
#include "ksim_trace.h"

using namespace ksim_plan;

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::fprintf(stderr, "plan_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::abort();                                                           \
    }                                                                         \
  } while (0)

namespace {

using Rng = std::mt19937_64;
int pick(Rng& g, int lo, int hi) { return lo + (int)(g() % (uint64_t)(hi - lo + 1)); }  // lo..hi

bool same(const PodDev& a, const PodDev& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
bool same_score(const PodDev& a, const PodDev& b) { return a.cpu_nz == b.cpu_nz && a.milli == b.milli && a.num == b.num; }

// One replica's planner inputs, owned.
struct Replica {
  std::vector<PodDev> ev, cls;
  std::vector<int> cn, ev_cls;
  std::vector<NodeRec> rec;
  std::vector<TypDev> tp;
  int typed = 0, ncpu = 0;
  ReplicaView view() const { return {&cls, &ev_cls, &rec, &tp, typed, ncpu, (int)tp.size()}; }
};

PlanInput input_of(const std::vector<Replica>& reps, int N) {
  PlanInput in;
  for (const Replica& r : reps) in.reps.push_back(r.view());
  in.N = N;
  in.cus = 256;
  in.score_table = true;
  in.resident = [](size_t) { return 1 << 20; };
  return in;
}

// A random event stream: `nreq` score requests of 1..70 classes each (at most `maxcls` classes in all), every class
// created at least once, a few deletes of earlier creations.
void fuzz_events(Rng& g, Replica& r, int maxcls) {
  std::vector<PodDev> proto;
  const int nreq = pick(g, 1, 6);
  for (int q = 0; q < nreq && (int)proto.size() < maxcls; ++q) {
    ksim_pod s{};
    s.cpu_nz_milli = 100 * (64 * q + pick(g, 1, 64));  // (distinct requests)
    s.gpu_count = pick(g, 0, 8);
    s.gpu_milli = s.gpu_count == 0 ? 0 : s.gpu_count == 1 ? pick(g, 1, 1000) : 1000;
    const int sz = std::min(pick(g, 0, 3) == 0 ? pick(g, 30, 70) : pick(g, 1, 12), maxcls - (int)proto.size());
    for (int k = 0; k < sz; ++k) {  // classes of one score request differ in their Filter part
      s.cpu_milli = s.cpu_nz_milli + k;
      s.mem_mib = 1024 * pick(g, 1, 4);
      s.type_mask = pick(g, 0, 1) ? KSIM_TYPE_ANY : 1u << pick(g, 0, 5);
      PodDev d;
      CHECK(to_pod_dev(s, &d) == KSIM_OK);
      proto.push_back(d);
    }
  }
  std::shuffle(proto.begin(), proto.end(), g);
  r.ev = proto;
  const int extra = pick(g, 0, 300);
  for (int k = 0; k < extra; ++k) {
    if (pick(g, 0, 9) == 0) {
      PodDev d{};
      d.flags = kPodDelete;
      d.ref = pick(g, 0, (int)r.ev.size() - 1);
      r.ev.push_back(d);
    } else {
      r.ev.push_back(proto[(size_t)pick(g, 0, (int)proto.size() - 1)]);
    }
  }
  classify_events(r.ev, r.cls, r.cn, r.ev_cls);
  // classify_events: one class per distinct request, ids in order of first appearance, counts
  CHECK(r.cls.size() == proto.size() && r.ev_cls.size() == r.ev.size());
  int seen = 0, total = 0;
  for (size_t i = 0; i < r.ev.size(); ++i) {
    const int c = r.ev_cls[i];
    CHECK(c == r.ev[i].pad);
    if (r.ev[i].flags & kPodDelete) { CHECK(c == -1); continue; }
    CHECK(c >= 0 && c <= seen && r.cls[c].pad == c);
    if (c == seen) ++seen;
    PodDev a = r.ev[i], b = r.cls[c];
    CHECK(same(a, b));
    ++total;
  }
  CHECK(seen == (int)r.cls.size());
  int sum = 0;
  for (int n : r.cn) sum += n;
  CHECK(sum == total);
}

// A random cluster: N nodes of a few distinct initial states over a few GPU models, ranks a permutation from node_off.
void fuzz_nodes(Rng& g, Replica& r, int N, int node_off) {
  const bool many = pick(g, 0, 2) == 0;  // many GPU models: per-model tables past their 12-bit offsets
  const int nst = many ? pick(g, 20, 40) : pick(g, 1, 12);
  std::vector<NodeRec> st(nst);
  for (NodeRec& n : st) {
    std::memset(&n, 0, sizeof n);
    n.cpu_left = 1000 * pick(g, 1, 128);
    n.mem_left = 1024 * pick(g, 1, 512);
    n.pods_left = 110;
    n.gpu_cnt = (uint8_t)pick(g, 0, 8);
    n.gpu_type = (uint8_t)pick(g, 0, many ? 31 : 7);
    for (int k = 0; k < n.gpu_cnt; ++k) n.gl[k] = (uint16_t)(pick(g, 0, 3) ? 1000 : pick(g, 0, 1000));
  }
  std::vector<uint32_t> rank(N);
  std::iota(rank.begin(), rank.end(), (uint32_t)node_off);
  std::shuffle(rank.begin(), rank.end(), g);
  r.rec.resize(N);
  for (int j = 0; j < N; ++j) {
    r.rec[j] = st[(size_t)pick(g, 0, nst - 1)];
    r.rec[j].name_rank = rank[j];
  }
}

void fuzz_typical(Rng& g, Replica& r) {
  const int nt = pick(g, 0, 3) == 0 ? pick(g, 200, 256) : pick(g, 1, 40);
  r.ncpu = pick(g, 0, nt / 2);
  r.tp.assign(nt, TypDev{});
  r.typed = 0;
  const bool wide = pick(g, 0, 2) == 0;  // many entries accept many models: long per-model tables
  for (int t = r.ncpu; t < nt; ++t) {
    r.tp[t].milli = 1000;
    r.tp[t].tmask = wide || pick(g, 0, 1) ? KSIM_TYPE_ANY : 1u << pick(g, 0, 7);
    r.typed |= r.tp[t].tmask != KSIM_TYPE_ANY;
  }
  if (wide && nt > r.ncpu) { r.tp[nt - 1].tmask = 1u; r.typed = 1; }
}

// ---- memo_plan + memo_events ----
void check_memo_plan(const PlanInput& in, const std::vector<Replica>& reps, const MemoPlan& pl) {
  using namespace memo;
  const int Rg = (int)reps.size();
  CHECK(pl.decider == in.decider && !(pl.decider && pl.hkeys));
  CHECK((int)pl.Kr.size() == Rg && (int)pl.wgoff.size() == Rg);
  int sum = 0, kmax = 0, cmax = 1;
  for (int i = 0; i < Rg; ++i) {
    CHECK(pl.wgoff[i] == sum && pl.Kr[i] >= 1 && pl.Kr[i] <= 64);
    sum += pl.Kr[i];
    kmax = std::max(kmax, pl.Kr[i]);
    cmax = std::max(cmax, (int)reps[i].cls.size());
  }
  CHECK(pl.nwg == sum && pl.K == kmax && pl.Cmax == cmax && pl.nwg <= in.cus);
  CHECK(pl.Cw >= 1 && pl.Cw <= kMaxCw && (pl.nfw == 16 || pl.nfw == 12));
  CHECK(pl.lds == memo_layout(in.N, pl.Cw, pl.nfw, pl.hkeys).total && pl.lds <= kLdsMax);
  const MemoLayout L = memo_layout(in.N, pl.Cw, pl.nfw, pl.hkeys);
  {  // the regions as k_memo carves them (the top of the kernel, ksim_memo.hpp)
    const size_t N = (size_t)in.N, Cw = (size_t)pl.Cw;
    CHECK(L.nodes == kSharedBytes && L.keys == L.nodes + N * sizeof(NodeRec));
    CHECK(L.fold == L.keys + (pl.hkeys ? 0 : (std::max(Cw * N * 4, kDeciderBytes) + 15) & ~(size_t)15));
    CHECK(L.last == L.fold + std::max((size_t)pl.nfw * kFoldBuf * 8, (N * 8 + 15) & ~(size_t)15));
    CHECK(L.fold % 16 == 0 && L.last % 16 == 0 && L.total == L.last + N * 4);
  }
  CHECK(pl.wgcls.size() == (size_t)pl.nwg * pl.Cw && pl.wgref.size() == pl.wgcls.size() && pl.wggrp.size() == pl.wgcls.size());
  for (int i = 0; i < Rg; ++i) {
    const std::vector<PodDev>& cls = reps[i].cls;
    std::vector<int> owned(cls.size(), 0);
    for (int w = 0; w < pl.Kr[i]; ++w) {
      const size_t o = ((size_t)pl.wgoff[i] + w) * pl.Cw;
      for (int j = 0; j < pl.Cw; ++j) {
        const int c = pl.wgcls[o + j];
        if (c < 0) { CHECK(c == -1 && pl.wggrp[o + j] == 0ull); continue; }
        CHECK(c < (int)cls.size());
        ++owned[c];
        CHECK(pl.owner[(size_t)i * pl.Cmax + c] == ((w << 8) | j));  // the one (workgroup, slot) of the class
        CHECK(!(pl.decider && w == 0));                                // the decider owns nothing
        int ref = j;  // the first slot of the workgroup with the same score request
        for (int j2 = j - 1; j2 >= 0; --j2)
          if (pl.wgcls[o + j2] >= 0 && same_score(cls[pl.wgcls[o + j2]], cls[c])) ref = j2;
        CHECK(pl.wgref[o + j] == ref);
        if (ref == j) {  // its bits: exactly the slots of the group
          unsigned long long bits = 0ull;
          for (int j2 = 0; j2 < pl.Cw; ++j2)
            if (pl.wgcls[o + j2] >= 0 && same_score(cls[pl.wgcls[o + j2]], cls[c])) bits |= 1ull << j2;
          CHECK(pl.wggrp[o + j] == bits);
        } else {
          CHECK(pl.wggrp[o + j] == 0ull);
        }
      }
    }
    for (size_t c = 0; c < cls.size(); ++c) {
      CHECK(owned[c] == 1);
      PodDev a = pl.pod[(size_t)i * pl.Cmax + c], b = cls[c];
      CHECK(same(a, b));
      if (!pl.hkeys)  // only the keys-in-HBM packing splits a score group over workgroups
        for (size_t c2 = 0; c2 < c; ++c2)
          if (same_score(cls[c], cls[c2]))
            CHECK(pl.owner[(size_t)i * pl.Cmax + c] >> 8 == pl.owner[(size_t)i * pl.Cmax + c2] >> 8);
    }
    for (size_t c = cls.size(); c < (size_t)pl.Cmax; ++c) CHECK(pl.owner[(size_t)i * pl.Cmax + c] == -1);
  }
}

void check_memo_events(const PlanInput& in, const std::vector<Replica>& reps, const MemoPlan& pl, int stride) {
  const MemoEvents t = memo_events(in, pl, stride);
  const int Rg = (int)reps.size();
  CHECK(t.evo.size() == (size_t)Rg * stride && t.evcls.size() == t.evo.size() && (int)t.wgmap.size() == pl.nwg);
  for (int gi = 0; gi < Rg; ++gi) {
    const std::vector<int>& ec = reps[gi].ev_cls;
    for (int k = 0; k < stride; ++k) {
      const int code = t.evo[(size_t)gi * stride + k], c = k < (int)ec.size() ? ec[k] : -1;
      CHECK(t.evcls[(size_t)gi * stride + k] == c);
      if (c < 0) { CHECK(code == -1); continue; }  // deletes and the padding
      const int w = code >> 16, ref = (code >> 8) & 0xff, slot = code & 0xff;
      CHECK(code >= 0 && pl.owner[(size_t)gi * pl.Cmax + c] == ((w << 8) | slot));
      CHECK(ref == pl.wgref[((size_t)pl.wgoff[gi] + w) * pl.Cw + slot]);
    }
    for (int w = 0; w < pl.Kr[gi]; ++w) CHECK(t.wgmap[(size_t)pl.wgoff[gi] + w] == ((gi << 8) | w));
  }
}

void fuzz_memo(int cases) {
  int planned = 0, refused = 0, hk = 0, dec = 0, gated = 0;
  for (int n = 0; n < cases; ++n) {
    Rng g(1000 + n);
    const int Rg = pick(g, 1, 4), K = pick(g, 1, 8);
    static const int sizes[] = {1, 37, 64, 500, 1213, 4096};
    const int N = sizes[pick(g, 0, 5)];
    std::vector<Replica> reps(Rg);
    int stride = 1;
    for (Replica& r : reps) {
      fuzz_events(g, r, pick(g, 0, 2) ? pick(g, 1, 40) : pick(g, 1, 200));
      stride = std::max(stride, (int)r.ev.size());
    }
    PlanInput in = input_of(reps, N);
    in.decider = pick(g, 0, 3) == 0;
    const int mode = pick(g, 0, 2);  // the engine's three ways to a width: its own, the run's, each replica's hint
    std::vector<int> kr;
    for (int i = 0; i < Rg; ++i) kr.push_back(pick(g, 1, 8));
    in.wgs_req = mode == 1 ? K : 0;
    const bool hkeys_ok = pick(g, 0, 1) == 1;
    MemoPlan pl;
    const bool ok = memo_plan(in, pl, 0, hkeys_ok, mode == 2 ? &kr : nullptr);
    if (!ok) { ++refused; continue; }
    ++planned;
    hk += pl.hkeys;
    dec += pl.decider;
    if (mode == 1) for (int k : pl.Kr) CHECK(k == K);
    if (mode == 2) CHECK(pl.Kr == kr);
    CHECK(hkeys_ok || !pl.hkeys);
    check_memo_plan(in, reps, pl);
    check_memo_events(in, reps, pl, stride + pick(g, 0, 3));
    // fewer resident workgroups than the launch has: refused when they exchange granules (K > 1)
    PlanInput tight = in;
    const int nwg = pl.nwg;
    tight.resident = [nwg](size_t) { return nwg - 1; };
    MemoPlan pl2;
    const bool ok2 = memo_plan(tight, pl2, 0, hkeys_ok, mode == 2 ? &kr : nullptr);
    if (pl.K > 1) { CHECK(!ok2); ++gated; }
    else CHECK(ok2 && pl2.nwg == nwg);
  }
  CHECK(planned > cases / 2 && refused > 0 && hk > 0 && dec > 0 && gated > 0);
  std::printf("memo_plan: cases=%d planned=%d refused=%d hkeys=%d decider=%d residency_refusals=%d\n", cases, planned,
              refused, hk, dec, gated);
}

// ---- hmemo_plan ----
void check_hmemo_plan(const PlanInput& in, const std::vector<Replica>& reps, const HPlan& pl, int stride) {
  using namespace hmemo;
  const int Rg = (int)reps.size(), N = in.N;
  CHECK(pl.Npad % kFan == 0 && pl.Npad >= N && pl.Npad < N + kFan && pl.nb == pl.Npad / kFan);
  CHECK(pl.K >= 1 && pl.K * pl.S >= N && pl.nbw == (pl.K == 1 ? pl.nb : pl.S / kFan));
  CHECK(pl.lds == hmemo_layout(pl.S, pl.Cmax, pl.Gmax, pl.nbw, pl.l2, pl.Mtab).total && pl.lds <= kLdsMax);
  int Mraw = 0;  // the longest concatenation of per-model tables, worked out independently below
  for (int i = 0; i < Rg; ++i) {
    const Replica& r = reps[i];
    const int nc = (int)r.cls.size();
    CHECK(pl.cg[2 * i] == nc);
    const int ng = pl.cg[2 * i + 1];
    // cls: a permutation of the classes, sorted by group; groups numbered by first appearance
    std::vector<int> slot_of(nc, -1);
    for (int k = 0; k < nc; ++k) {
      const PodDev& p = pl.cls[(size_t)i * pl.Cmax + k];
      CHECK(p.pad >= 0 && p.pad < nc && slot_of[p.pad] < 0);
      PodDev a = p, b = r.cls[p.pad];
      CHECK(same(a, b));
      slot_of[p.pad] = k;
      const int gk = pl.cgrp[(size_t)i * pl.Cmax + k];
      CHECK(gk < ng && (k == 0 || gk >= pl.cgrp[(size_t)i * pl.Cmax + k - 1]));
      CHECK(same_score(p, pl.gpod[(size_t)i * pl.Gmax + gk]));
    }
    for (int a = 0; a < ng; ++a)
      for (int b = 0; b < a; ++b) CHECK(!same_score(pl.gpod[(size_t)i * pl.Gmax + a], pl.gpod[(size_t)i * pl.Gmax + b]));
    CHECK(nc <= pl.Cmax && ng <= pl.Gmax);
    // gpod: the least demanding Filter part of the group
    for (int gk = 0; gk < ng; ++gk) {
      int cpu = INT32_MAX, mem = INT32_MAX;
      uint32_t tm = 0u;
      for (int k = 0; k < nc; ++k)
        if (pl.cgrp[(size_t)i * pl.Cmax + k] == gk) {
          const PodDev& p = pl.cls[(size_t)i * pl.Cmax + k];
          cpu = std::min(cpu, p.cpu_req);
          mem = std::min(mem, p.mem);
          tm |= p.tmask;
        }
      const PodDev& gp = pl.gpod[(size_t)i * pl.Gmax + gk];
      CHECK(gp.cpu_req == cpu && gp.mem == mem && gp.tmask == tm);
    }
    // evc: each event to the slot of its class
    for (int k = 0; k < stride; ++k) {
      const int c = k < (int)r.ev_cls.size() ? r.ev_cls[k] : -1;
      CHECK(pl.evc[(size_t)i * stride + k] == (c < 0 ? -1 : slot_of[c]));
    }
    // nstate: every rank 0..N-1 once, the state the node of that rank starts in; -1 padding
    CHECK(pl.ns[i] >= 1 && pl.ns[i] <= pl.Smax);
    std::vector<int> hit(pl.Npad, 0);
    for (const NodeRec& n : r.rec) {
      const int rank = (int)(n.name_rank - (uint32_t)in.node_off);
      CHECK(rank >= 0 && rank < N);
      ++hit[rank];
      const int s = pl.nstate[(size_t)i * pl.Npad + rank];
      CHECK(s >= 0 && s < pl.ns[i] && std::memcmp(&pl.st[(size_t)i * pl.Smax + s], &n, 28) == 0);
    }
    for (int k = 0; k < pl.Npad; ++k) CHECK(k < N ? hit[k] == 1 : pl.nstate[(size_t)i * pl.Npad + k] == -1);
    for (int a = 0; a < pl.ns[i]; ++a)
      for (int b = 0; b < a; ++b)
        CHECK(std::memcmp(&pl.st[(size_t)i * pl.Smax + a], &pl.st[(size_t)i * pl.Smax + b], 28) != 0);
    // the per-model tables this replica would have
    if (in.hmodel && pl.K == 1 && r.typed) {
      uint32_t models = 0u;
      for (const NodeRec& n : r.rec) models |= 1u << n.gpu_type;
      int len = 0;
      for (int m = 0; m < KSIM_MAX_TYPES; ++m)
        for (int t = 0; ((models >> m) & 1u) && t < (int)r.tp.size(); ++t) len += t < r.ncpu || ((r.tp[t].tmask >> m) & 1u);
      Mraw = std::max(Mraw, len);
    }
  }
  if (Mraw > 4095 || hmemo_layout(pl.S, pl.Cmax, pl.Gmax, pl.nbw, pl.l2, Mraw).total > kLdsMax) {  // the whole-table form
    Mraw = 0;
    for (int f : pl.mtoff) CHECK(f == 0);
  }
  CHECK(pl.Mtab == Mraw);
  int slots = 0;
  for (int i = 0; pl.Mtab > 0 && i < Rg; ++i) {  // (without tables nothing reads mtoff)
    const Replica& r = reps[i];
    uint32_t models = 0u;
    for (const NodeRec& n : r.rec) models |= 1u << n.gpu_type;
    int slot = 0, off = 0;
    for (int m = 0; m < KSIM_MAX_TYPES; ++m) {
      const uint32_t f = (uint32_t)pl.mtoff[(size_t)i * KSIM_MAX_TYPES + m];
      if (!r.typed || !((models >> m) & 1u)) { CHECK(f == 0u); continue; }
      CHECK((f & kMtPresent) && (int)((f >> 21) & 0x3ffu) == slot && (int)(f & 0xfffu) == off);
      const int len = (int)((f >> 12) & 0x1ffu);
      int k = 0;
      for (int t = 0; t < (int)r.tp.size(); ++t)
        if (t < r.ncpu || ((r.tp[t].tmask >> m) & 1u)) {
          CHECK(k < len && pl.mtab[(size_t)i * pl.Mtab + off + k] == t);
          ++k;
        }
      CHECK(k == len);
      off += len;
      ++slot;
    }
    CHECK(off <= pl.Mtab);
    slots = std::max(slots, slot);
  }
  CHECK(pl.Mtab == 0 || pl.Mslots == slots);
}

void fuzz_hmemo(int cases) {
  int planned = 0, refused = 0, wide = 0, tables = 0, whole = 0;
  for (int n = 0; n < cases; ++n) {
    Rng g(5000 + n);
    const int Rg = pick(g, 1, 4);
    static const int sizes[] = {1, 63, 64, 65, 700, 1213, 4096, 4097, 9000};
    const int N = sizes[pick(g, 0, 8)], node_off = pick(g, 0, 1) ? 0 : pick(g, 1, 100000);
    std::vector<Replica> reps(Rg);
    int stride = 1;
    for (Replica& r : reps) {
      fuzz_events(g, r, pick(g, 1, 200));
      fuzz_nodes(g, r, N, node_off);
      fuzz_typical(g, r);
      stride = std::max(stride, (int)r.ev.size());
    }
    PlanInput in = input_of(reps, N);
    in.node_off = node_off;
    in.hl2 = pick(g, 0, 1) == 1;
    in.hmodel = pick(g, 0, 3) != 0;
    if (pick(g, 0, 3) == 0) { in.run_mode = 5; in.wgs_req = pick(g, 0, 8); }
    HPlan pl;
    if (!hmemo_plan(in, stride, pl)) { ++refused; continue; }
    ++planned;
    check_hmemo_plan(in, reps, pl, stride);
    CHECK(!pl.l2 || (in.hl2 && pl.K == 1));
    wide += pl.K > 1;
    tables += pl.Mtab > 0;
    for (const Replica& r : reps) whole += in.hmodel && pl.K == 1 && r.typed && pl.Mtab == 0;
  }
  CHECK(planned > cases / 2 && wide > 0 && tables > 0 && whole > 0);
  PlanInput none = input_of(std::vector<Replica>(1), 1);
  none.score_table = false;  // no score steps: no k_hmemo
  HPlan pl;
  CHECK(!hmemo_plan(none, 1, pl));
  std::printf("hmemo_plan: cases=%d planned=%d refused=%d wide=%d per_model_tables=%d whole_table_fallbacks=%d\n", cases,
              planned, refused, wide, tables, whole);
}

// ---- the plans the engine printed on the GPU ----
void check_recorded(const char* node_csv, const char* pod_csv) {
  ksim_trace* t = nullptr;
  CHECK(ksim_trace_load_openb(node_csv, pod_csv, &t) == KSIM_OK);
  const int N = ksim_trace_num_nodes(t);
  CHECK(N == 1213);
  // the bench's typical table (GetTypicalPods with the paper's configuration), split as ksim_engine_set_typical does
  const ksim_typical_cfg tcfg = {1, 95, 1, 0, 0.0};
  std::vector<ksim_typical> typ(4096);
  int nt = 0;
  CHECK(ksim_trace_typical(t, &tcfg, typ.data(), (int)typ.size(), &nt) == KSIM_OK);
  std::vector<TypDev> cpu, gpu;
  int typed = 0;
  for (int i = 0; i < nt; ++i) {
    if (typ[i].freq < 0 || typ[i].freq > 1) continue;
    TypDev d{};
    d.cpu = (int32_t)typ[i].cpu_milli;
    d.milli = typ[i].gpu_milli;
    d.num_eff = std::max(typ[i].gpu_count, 1);
    d.tmask = typ[i].type_mask;
    d.freq = typ[i].freq;
    if (d.milli == 0) cpu.push_back(d);
    else { typed |= d.tmask != KSIM_TYPE_ANY; gpu.push_back(d); }
  }
  // C2: seeds 42..51, tune 1.3, shuffled; the empty cluster's records as ksim_engine_set_nodes makes them
  std::vector<Replica> reps(10);
  for (int s = 0; s < 10; ++s) {
    Replica& r = reps[s];
    const ksim_replay_cfg rcfg = {(uint64_t)(42 + s), 1.3, 1, -1};
    int ne = 0;
    std::vector<ksim_node> nodes(N);
    std::vector<ksim_pod> ev(1);
    CHECK(ksim_trace_replay(t, &rcfg, ev.data(), 1, &ne, nullptr, nodes.data(), nullptr) == KSIM_ERANGE);
    ev.resize(ne);
    CHECK(ksim_trace_replay(t, &rcfg, ev.data(), ne, &ne, nullptr, nodes.data(), nullptr) == KSIM_OK);
    r.ev.resize(ne);
    for (int i = 0; i < ne; ++i) CHECK(to_pod_dev(ev[i], &r.ev[i]) == KSIM_OK);
    classify_events(r.ev, r.cls, r.cn, r.ev_cls);
    r.rec.assign(N, NodeRec{});
    for (int i = 0; i < N; ++i) {
      const ksim_node& s2 = nodes[i];
      NodeRec& n = r.rec[i];
      n.cpu_left = (int32_t)(s2.cpu_alloc_milli - s2.cpu_used_milli);
      n.mem_left = (int32_t)(s2.mem_alloc_mib - s2.mem_used_mib);
      n.pods_left = (int16_t)(s2.pods_alloc - s2.pods_used);
      n.gpu_cnt = (uint8_t)s2.gpu_count;
      n.gpu_type = (uint8_t)s2.gpu_type;
      n.name_rank = s2.name_rank;
      for (int k = 0; k < s2.gpu_count; ++k) n.gl[k] = (uint16_t)(1000 - s2.gpu_used_milli[k]);
    }
    r.tp = cpu;
    r.tp.insert(r.tp.end(), gpu.begin(), gpu.end());
    r.ncpu = (int)cpu.size();
    r.typed = typed;
  }
  ksim_trace_free(t);
  PlanInput in = input_of(reps, N);
  in.resident = [](size_t) { return 256; };  // one workgroup per CU
  MemoPlan mp;
  CHECK(memo_plan(in, mp));
  std::printf("recorded: C2 k_memo K=%d Cw=%d nfw=%d workgroups=%d LDS=%zu", mp.K, mp.Cw, mp.nfw, mp.nwg, mp.lds);
  CHECK(mp.K == 25 && mp.Cw == 9 && mp.nfw == 16 && mp.nwg == 250 && mp.lds == 163124 && !mp.hkeys);
  check_memo_plan(in, reps, mp);
  int stride = 1;
  for (const Replica& r : reps) stride = std::max(stride, (int)r.ev.size());
  check_memo_events(in, reps, mp, stride);
  in.run_mode = 5;  // k_hmemo at one workgroup per replica
  HPlan hp;
  CHECK(hmemo_plan(in, stride, hp));
  std::printf("; k_hmemo K=%d S=%d Cmax=%d Gmax=%d Smax=%d LDS=%zu", hp.K, hp.S, hp.Cmax, hp.Gmax, hp.Smax, hp.lds);
  CHECK(hp.K == 1 && hp.S == 1213 && hp.Cmax == 151 && hp.Gmax == 91 && hp.Smax == 15 && hp.lds == 92576);
  check_hmemo_plan(in, reps, hp, stride);
  // C5: 100 000 nodes (bench.py), the engine's own width
  const hmemo::HSlices c5 = hmemo::hmemo_slices(100000, 64, hmemo::kNoClamp);
  std::printf("; C5 slices K=%d S=%d\n", c5.K, c5.S);
  CHECK(c5.K == 63 && c5.S == 1600);
}

// ---- the slice geometry against the three call sites' formulas ----
void check_slices() {
  using namespace hmemo;
  long n = 0;
  for (int world = 1; world <= 16; ++world)
    for (int nmax = 64; nmax <= 200000; ++nmax) {
      {  // one shard per process (ksim_engine_run of a shard with peers)
        int K = std::max(1, 64 / world);
        int S = std::max(kFan, (nmax + K - 1) / K + kFan - 1) / kFan * kFan;
        if (S > kMaxNb * kFan) {
          S = kMaxNb * kFan;
          K = (nmax + S - 1) / S;
        }
        const HSlices sl = hmemo_slices(nmax, std::max(1, 64 / world), kClampKeepK);
        CHECK(sl.S == S && sl.K == K);
      }
      for (int cus : {8, 256, 304}) {  // the in-process shard group
        const int want = std::max(1, std::min(64, cus / world));
        int S = std::max(kFan, (nmax + want - 1) / want + kFan - 1) / kFan * kFan;
        S = std::min(S, kMaxNb * kFan);
        const int K = (nmax + S - 1) / S;
        const HSlices sl = hmemo_slices(nmax, want, kClamp);
        CHECK(sl.S == S && sl.K == K);
      }
      {  // the unsharded wide form (hmemo_plan), at the widths a run can ask for
        const int want = world == 1 ? 64 : world;
        const int S = std::max(kFan, (nmax + want - 1) / want + kFan - 1) / kFan * kFan;
        const int K = (nmax + S - 1) / S;
        const HSlices sl = hmemo_slices(nmax, want, kNoClamp);
        CHECK(sl.S == S && sl.K == K);
      }
      n += 5;
    }
  std::printf("slices: compared=%ld\n", n);
}

// ---- the form tables against the conditionals they replaced ----
// k_memo<decider, general, stress, report, hkeys> as launch_memo chose it
std::tuple<bool, bool, bool, bool, bool> memo_was(bool decider, bool hkeys, bool general, int delay, bool report) {
  using T = std::tuple<bool, bool, bool, bool, bool>;
  return decider ? T{true, true, false, false, false}
         : hkeys ? (general ? T{false, true, false, false, true}
                            : report ? T{false, false, false, true, true} : T{false, false, false, false, true})
         : general ? T{false, true, false, false, false}
         : delay ? T{false, false, true, false, false}
         : report ? T{false, false, false, true, false} : T{false, false, false, false, false};
}

void check_forms() {
  int nm = 0, nh = 0;
  std::set<int> mcodes, hcodes;
  for (int bits = 0; bits < 128; ++bits)
    for (int hdelay : {0, 1, 0xff}) {
      const bool decider = bits & 1, hkeys = bits & 2, profile = bits & 4, tracing = bits & 8, table = bits & 16,
                 any_delete = bits & 32, report = bits & 64;
      const MemoForm f = memo_form(decider, hkeys, profile, tracing, table, any_delete, report, hdelay);
      const bool general = profile || tracing || !table || any_delete;
      CHECK(std::make_tuple(f.decider, f.general, f.stress, f.report, f.hkeys) == memo_was(decider, hkeys, general, hdelay, report));
      switch ((MemoFormCode)f.code()) {  // one of the forms the engine has an instantiation for
        case kMemoLean: case kMemoDecider: case kMemoGeneral: case kMemoStress: case kMemoReport: case kMemoHKeysLean:
        case kMemoHKeysGeneral: case kMemoHKeysReport: break;
        default: CHECK(!"memo_form returned a form without an instantiation");
      }
      mcodes.insert(f.code());
      ++nm;
    }
  CHECK(mcodes.size() == 8);
  // report + hdelay on a create-only stream: the stress form, which has none of the report's stores (kept as it is)
  CHECK(memo_form(false, false, false, false, true, false, true, 1).code() == kMemoStress);
  for (int Ktot = 1; Ktot <= 256; ++Ktot)
    for (int bits = 0; bits < 4; ++bits)
      for (int hdelay : {0, 1, 0xff}) {
        const bool profile = bits & 1, model = bits & 2;
        // launch_hmemo: k_hmemo<sub, gen, model>
        {
          const bool gen = profile || hdelay != 0;
          const std::tuple<int, bool, bool> was = Ktot == 1 ? std::make_tuple(0, gen, model)
                                                  : Ktot <= 64 ? std::make_tuple(1, gen, false) : std::make_tuple(4, gen, false);
          const HMemoForm f = hmemo_form(kHLocal, Ktot, profile, hdelay, model);
          CHECK(std::make_tuple(f.sub, f.prof, f.model) == was && !f.group);
          hcodes.insert(f.code());
        }
        // a shard with peers: k_hmemo<sub, gen>; an in-process group: k_hmemo_group<sub, gen>; gen from hdelay alone
        for (HMemoWhere where : {kHPeer, kHGroup}) {
          const bool gen = hdelay != 0;
          const HMemoForm f = hmemo_form(where, Ktot, profile, hdelay, model);
          CHECK(f.sub == (Ktot <= 64 ? 1 : 4) && f.prof == gen && !f.model && f.group == (where == kHGroup));
          hcodes.insert(f.code());
        }
        nh += 3;
      }
  for (int c : hcodes)
    switch ((HMemoFormCode)c) {
      case kHMemoOne: case kHMemoOneProf: case kHMemoOneModel: case kHMemoOneProfModel: case kHMemoWide: case kHMemoWideProf:
      case kHMemoWide4: case kHMemoWide4Prof: case kHMemoGroup: case kHMemoGroupProf: case kHMemoGroup4: case kHMemoGroup4Prof:
        break;
      default: CHECK(!"hmemo_form returned a form without an instantiation");
    }
  CHECK(hcodes.size() == 12);
  std::printf("forms: memo_inputs=%d memo_forms=%zu hmemo_inputs=%d hmemo_forms=%zu\n", nm, mcodes.size(), nh, hcodes.size());
}

// ---- the run plan (make_run_plan) ----
// What the last_run_* getters would show of a plan: the kernel names (each once, in launch order), the launches, the
// side streams used.
struct Seen {
  std::vector<std::string> kernels;
  int launches, streams;
};
Seen seen_of(const RunPlanInput& in, const RunPlan& pl) {
  Seen s{{}, (int)pl.groups.size(), 0};
  std::set<int> sides;
  for (const PlanGroup& g : pl.groups) {
    const char* nm = g.kernel == kRunRandomGo ? "k_random_go"
                     : g.kernel == kRunScan1  ? (g.kind == scan1::kPolMix ? "k_scan1_mix" : "k_scan1")
                     : g.kernel == kRunMemo   ? "k_memo"
                     : g.kernel == kRunHmemo  ? (in.hmemo_K == 1 ? "k_hmemo" : "k_hmemo_wide")
                     : g.kernel == kRunReplay ? "k_replay" : "none";
    if (std::find(s.kernels.begin(), s.kernels.end(), nm) == s.kernels.end()) s.kernels.push_back(nm);
    if (g.side >= 0) sides.insert(g.side);
  }
  s.streams = (int)sides.size();
  return s;
}

struct WantGroup {
  int kind, count;
  GroupKernel kernel;
  int side, K;
};
RunReplica rr(int policy, int n_events = 300, bool go = false, bool del = false) { return {policy, go, n_events, del, 0}; }

// The nine cases of tests/test_gpu_run_plan.py (the openb default cluster: 1213 nodes, 256 CUs, wgs_per_replica = 1
// unless the case says otherwise, four hardware queues) as planner inputs, with the plans written out.  The FGD plans
// are what prepare_memo makes there: at one workgroup per replica k_memo has no plan and k_hmemo has one at K = 1.
void check_run_plan_cases() {
  const int mix = scan1::kPolMix;
  auto base = [](std::vector<RunReplica> reps) {
    RunPlanInput in;
    in.reps = std::move(reps);
    in.N = 1213;
    in.cus = 256;
    in.wgs_req = 1;
    in.scan1 = 2;
    in.side_streams = 4;
    return in;
  };
  auto hmemo1 = [](RunPlanInput in, std::vector<int> reps) {
    in.hmemo_ok = true;
    in.hmemo_K = 1;
    in.hmemo_reps = std::move(reps);
    return in;
  };
  struct Case {
    const char* name;
    RunPlanInput in;
    std::vector<int> order;
    std::vector<WantGroup> groups;
    Seen want;  // the `want` tuple of the GPU test: kernels, launches, side streams
    bool concurrent;
  };
  std::vector<Case> cases;
  const std::vector<RunReplica> sweep = {rr(POL_FGD), rr(POL_FGD, 260), rr(POL_BESTFIT, 280), rr(POL_PACKING)};
  cases.push_back({"a-fgd-beside-mix", hmemo1(base(sweep), {0, 1}), {0, 1, 3, 2},
                   {{POL_FGD, 2, kRunHmemo, 0, 1}, {mix, 2, kRunScan1, 1, 1}}, {{"k_hmemo", "k_scan1_mix"}, 2, 2}, true});
  {
    RunPlanInput in = hmemo1(base(sweep), {0, 1});
    in.report = true;
    cases.push_back({"b-overlapped-report", in, {0, 1, 3, 2},
                     {{POL_FGD, 2, kRunHmemo, 0, 1}, {mix, 2, kRunScan1, 1, 1}}, {{"k_hmemo", "k_scan1_mix"}, 2, 2}, true});
  }
  {
    RunPlanInput in = base({rr(POL_FGD), rr(POL_BESTFIT)});
    in.wgs_req = 0;
    in.memo_ok = true;  // k_memo at K = 64
    in.memo_nwg = 64;
    in.memo_reps = {0};
    cases.push_back({"c-memo-back-to-back", in, {0, 1},
                     {{POL_FGD, 1, kRunMemo, -1, 1}, {POL_BESTFIT, 1, kRunReplay, -1, 64}}, {{"k_memo", "k_replay"}, 2, 0}, false});
  }
  {
    RunPlanInput in = hmemo1(base(sweep), {1});  // replica 0 hinted to six workgroups: the split
    in.split_fgd = in.memo_ok = true;
    in.memo_nwg = 6;
    in.memo_reps = {0};
    cases.push_back({"d-split-fgd", in, {0, 1, 3, 2},
                     {{POL_FGD, 1, kRunMemo, -1, 1}, {kPolFgdH, 1, kRunHmemo, 0, 1}, {mix, 2, kRunScan1, 1, 1}},
                     {{"k_memo", "k_hmemo", "k_scan1_mix"}, 3, 2}, true});
  }
  cases.push_back({"e-deletes-general-replay", base({rr(POL_PACKING, 299, false, true), rr(POL_BESTFIT)}), {1, 0},
                   {{POL_BESTFIT, 1, kRunReplay, 0, 1}, {POL_PACKING, 1, kRunReplay, 1, 1}}, {{"k_replay"}, 2, 2}, true});
  cases.push_back({"f-random-go-last", base({rr(POL_RANDOM, 300, true), rr(POL_BESTFIT, 280), rr(POL_PACKING)}), {2, 1, 0},
                   {{mix, 2, kRunScan1, 0, 1}, {kPolRandomGo, 1, kRunRandomGo, 1, 1}}, {{"k_scan1_mix", "k_random_go"}, 2, 2},
                   true});
  for (int nq : {1, 2}) {
    RunPlanInput in = base({rr(POL_BESTFIT), rr(POL_DOTPROD, 260), rr(POL_PACKING, 280), rr(POL_CLUSTERING, 240), rr(POL_RANDOM)});
    in.scan1_mix = false;
    in.side_streams = nq;
    const int s = nq - 1;  // every group after the first on the last side stream
    cases.push_back({nq == 1 ? "g-round-robin-1" : "g-round-robin-2", in, {0, 1, 2, 3, 4},
                     {{POL_BESTFIT, 1, kRunScan1, 0, 1}, {POL_DOTPROD, 1, kRunScan1, s, 1}, {POL_PACKING, 1, kRunScan1, s, 1},
                      {POL_CLUSTERING, 1, kRunScan1, s, 1}, {POL_RANDOM, 1, kRunScan1, s, 1}},
                     {{"k_scan1"}, 5, nq}, true});
  }
  {
    RunPlanInput in = base({rr(POL_PWR_FGD)});
    in.run_mode = 2;
    cases.push_back({"h-pwr-fgd-replay", in, {0}, {{POL_PWR_FGD, 1, kRunReplay, -1, 1}}, {{"k_replay"}, 1, 0}, false});
  }
  CHECK(cases.size() == 9);
  for (const Case& c : cases) {
    const RunPlan pl = make_run_plan(c.in);
    if (pl.order != c.order || pl.groups.size() != c.groups.size() || pl.concurrent != c.concurrent) {
      std::fprintf(stderr, "plan_check: run plan case %s\n", c.name);
      CHECK(!"the plan's order, group count or concurrency differs");
    }
    int first = 0;
    for (size_t i = 0; i < c.groups.size(); ++i) {
      const PlanGroup& g = pl.groups[i];
      const WantGroup& w = c.groups[i];
      if (g.kind != w.kind || g.count != w.count || g.kernel != w.kernel || g.side != w.side || g.K != w.K || g.first != first) {
        std::fprintf(stderr, "plan_check: run plan case %s group %zu\n", c.name, i);
        CHECK(!"the group differs");
      }
      first += g.count;
    }
    const Seen s = seen_of(c.in, pl);
    CHECK(s.kernels == c.want.kernels && s.launches == c.want.launches && s.streams == c.want.streams);
  }
  // what the launchers read beside the groups
  const RunPlan a = make_run_plan(cases[0].in), b = make_run_plan(cases[1].in), c = make_run_plan(cases[2].in),
                d = make_run_plan(cases[3].in), e = make_run_plan(cases[4].in);
  CHECK(a.reg1 && !a.general && a.fgd_cus == 2 && a.groups[1].lds == 7296 && a.groups[1].S == 1213);
  CHECK(b.general && b.groups[1].lds == 7296 + 4 * 1213);  // the report's last-event table
  CHECK(c.fgd_cus == 64 && c.groups[1].S == 19 && c.groups[1].lds == replay::replay_lds(19, POL_BESTFIT, false));
  CHECK(d.fgd_cus == 7);
  CHECK(e.any_delete && e.general && e.groups[0].lds == replay::replay_lds(1213, POL_BESTFIT, true));
}

// The formulas the planner's arithmetic had in the engine, restated.
int old_choose_wgs(int cus, int N, int wgs_req, int R) {
  int K = wgs_req;
  if (K <= 0) {
    K = std::min(cus / R, 64);
    K = std::max(K, std::min(cus / R, (N + 383) / 384));
  }
  K = std::max(1, std::min(K, 256));
  K = std::min(K, N);
  if (R * K > cus) K = 1;
  return K;
}
size_t old_replay_lds(int S, int pol, bool general) { return replay::replay_layout(S, pol, general).total; }

long check_run_formulas() {
  long n = 0;
  static const int Ns[] = {1, 2, 63, 384, 385, 1213, 4095, 4096, 5000, 24576, 100000};
  static const int wgs[] = {0, 1, 7, 64, 300};
  for (int cus : {64, 256, 304})
    for (int R = 1; R <= 40; ++R)
      for (int N : Ns)
        for (int wr : wgs) {
          const int K0 = old_choose_wgs(cus, N, wr, R);
          CHECK(choose_wgs(cus, N, wr, R) == K0);
          ++n;
          for (int pol = POL_FGD; pol <= POL_PWR_FGD; ++pol)
            for (bool general : {false, true}) {
              // replay_fit as it stood
              int K = K0, S = (N + K - 1) / K;
              while (old_replay_lds(S, pol, general) > 160 * 1024 && K < 256 && R * (K + 1) <= cus) {
                ++K;
                S = (N + K - 1) / K;
              }
              RunPlanInput in;
              in.N = N;
              in.cus = cus;
              in.wgs_req = wr;
              PlanGroup g;
              g.kind = pol;
              g.count = R;
              CHECK(replay_fit(in, general, g) == K0 && g.K == K && g.S == S && g.lds == old_replay_lds(S, pol, general));
              ++n;
              if (K == 1 || g.lds > 160 * 1024) continue;  // (the launcher queries no occupancy, or has refused)
              // launch_replay's narrowing as it stood, at the residencies around the grid's size
              for (int cap : {0, 1, R - 1, R, R * K / 2, R * K - 1, R * K, 2 * cus}) {
                int K2 = K, S2 = S, rc = 0;  // rc 1: the silent refusal, 2: the one with the message
                if (R * K2 > cap) {
                  if (wr > 0 && cap < R) rc = 1;
                  else {
                    K2 = std::max(1, std::min(K2, cap / R));
                    S2 = (N + K2 - 1) / K2;
                    if (old_replay_lds(S2, pol, general) > 160 * 1024) rc = 2;
                  }
                }
                const ReplayNarrow nw = replay_narrow(K, cap, R, N, wr, [&](int s) { return old_replay_lds(s, pol, general); });
                CHECK(nw.refused == (rc == 0 ? kNarrowOk : rc == 1 ? kNarrowAsked : kNarrowLds));
                if (rc != 1) CHECK(nw.K == K2 && nw.S == S2);
                ++n;
              }
            }
        }
  return n;
}

// Invariants of make_run_plan over seeded random inputs.
void fuzz_run_plan(int cases) {
  std::set<int> kernels;
  int conc = 0, b2b = 0, split = 0, mixed = 0;
  for (int n = 0; n < cases; ++n) {
    Rng g(9000 + n);
    RunPlanInput in;
    const int R = pick(g, 1, 40);
    const bool cheap = pick(g, 0, 2) == 0;  // the paper sweep's shape: few FGD replicas among cheap ones
    std::vector<int> fgd;
    for (int r = 0; r < R; ++r) {
      RunReplica v;
      v.policy = cheap && pick(g, 0, 5) ? pick(g, POL_BESTFIT, POL_RANDOM) : pick(g, POL_FGD, POL_PWR_FGD);
      v.go_random = v.policy == POL_RANDOM && pick(g, 0, 2) == 0;
      v.n_events = pick(g, 0, 400);
      v.has_delete = pick(g, 0, 40) == 0;
      v.dpcfg = pick(g, 0, 3) ? (DIM_MERGE | NORM_MAX << 4) : (pick(g, 0, 3) | pick(g, 0, 2) << 4);
      if (v.policy == POL_FGD) fgd.push_back(r);
      in.reps.push_back(v);
    }
    in.N = pick(g, 0, 1) ? pick(g, 1, 1300) : pick(g, 1, 5000);
    static const int cus[] = {64, 256, 304}, wgs[] = {0, 1, 7, 64};
    in.cus = cus[pick(g, 0, 2)];
    in.wgs_req = wgs[pick(g, 0, 3)];
    in.run_mode = pick(g, 0, 2) ? 0 : pick(g, 0, 5);
    in.report = pick(g, 0, 1) == 1;
    in.scan1 = pick(g, 0, 2);
    in.timers = pick(g, 0, 9) == 0;
    in.scan1_mix = pick(g, 0, 4) != 0;
    in.side_streams = pick(g, 1, 6);
    // the FGD plans as prepare_memo leaves them: none, k_memo for all, k_hmemo for all, or (run_mode 0) the split
    const int how = fgd.empty() || in.run_mode == 1 || in.run_mode == 2 ? 0 : pick(g, 0, in.run_mode == 0 && fgd.size() >= 2 ? 3 : 2);
    if (how == 1) {
      in.memo_ok = true;
      in.memo_reps = fgd;
      in.memo_nwg = pick(g, (int)fgd.size(), std::max((int)fgd.size(), in.cus));
    } else if (how == 2) {
      in.hmemo_ok = true;
      in.hmemo_reps = fgd;
      in.hmemo_K = pick(g, 0, 2) ? 1 : pick(g, 2, 64);
    } else if (how == 3) {
      in.split_fgd = in.memo_ok = in.hmemo_ok = true;
      const int nw = pick(g, 1, (int)fgd.size() - 1);
      in.memo_reps.assign(fgd.begin(), fgd.begin() + nw);
      in.hmemo_reps.assign(fgd.begin() + nw, fgd.end());
      in.memo_nwg = 2 * nw;
      in.hmemo_K = 1;
    }
    const RunPlan pl = make_run_plan(in);
    // order: a permutation, tiled by the groups
    std::vector<int> sorted = pl.order;
    std::sort(sorted.begin(), sorted.end());
    for (int r = 0; r < R; ++r) CHECK((int)sorted.size() == R && sorted[r] == r);
    int first = 0, nmix = 0;
    bool all_engine = true, any_delete = false;
    for (const RunReplica& v : in.reps) any_delete = any_delete || v.has_delete;
    CHECK(pl.any_delete == any_delete && pl.general == (in.timers || in.report || any_delete));
    for (size_t gi = 0; gi < pl.groups.size(); ++gi) {
      const PlanGroup& q = pl.groups[gi];
      CHECK(q.first == first && q.count > 0);
      first += q.count;
      std::set<int> pols;
      for (int j = q.first; j < q.first + q.count; ++j) {
        const RunReplica& v = in.reps[pl.order[j]];
        pols.insert(v.policy);
        if (q.kind == kPolRandomGo) CHECK(v.go_random);
        else if (q.kind == kPolFgdH) CHECK(v.policy == POL_FGD && in.split_fgd);
        else if (q.kind == scan1::kPolMix)
          CHECK(!v.go_random && v.policy >= POL_BESTFIT && v.policy <= POL_RANDOM &&
                (v.policy != POL_DOTPROD || v.dpcfg == (DIM_MERGE | NORM_MAX << 4)));
        else CHECK(v.policy == q.kind && !v.go_random);
        // the mixed launch: longest stream first
        if (q.kind == scan1::kPolMix && j > q.first) CHECK(in.reps[pl.order[j - 1]].n_events >= v.n_events);
      }
      if (q.kind == kPolRandomGo) CHECK(gi + 1 == pl.groups.size() && q.kernel == kRunRandomGo);  // Go's stream last
      else CHECK(q.kernel != kRunRandomGo);
      if (q.kind == scan1::kPolMix) {
        ++nmix;
        CHECK(pols.size() >= 2 && q.kernel == kRunScan1 && pl.concurrent && in.scan1_mix);
      }
      CHECK(q.side >= -1 && q.side < in.side_streams);
      all_engine = all_engine && q.side == -1;
      if (!pl.concurrent) CHECK(q.side == -1);
      if (q.kernel == kRunScan1 || q.kernel == kRunReplay) {
        CHECK(q.K >= 1 && (long)q.K * q.S >= in.N);
        if (pl.concurrent) CHECK(q.K == 1);
        CHECK(q.count * q.K <= in.cus || q.K == 1);
      }
      if (q.kernel == kRunScan1) {
        CHECK(!any_delete && !in.timers && in.scan1 && in.N <= kMaxSlice && q.K == 1 && q.S == in.N && q.lds <= kLdsMax);
        CHECK(q.lds == scan1::scan1_lds(in.N, q.kind, in.report, pl.reg1) && (q.kind == scan1::kPolMix || scan1::scan1_serves(q.kind)));
      }
      if (q.kernel == kRunReplay) CHECK(q.lds == replay::replay_lds(q.S, q.kind, pl.general));
      if (q.kernel == kRunMemo) CHECK(q.kind == POL_FGD && in.memo_ok && (!pl.concurrent || in.split_fgd));
      if (q.kernel == kRunHmemo) CHECK((q.kind == POL_FGD || q.kind == kPolFgdH) && in.hmemo_ok && (!pl.concurrent || in.hmemo_K == 1));
      if (q.kernel == kRunNone) CHECK(q.kind == POL_FGD && in.run_mode >= 3 && in.run_mode <= 5);
      kernels.insert((int)q.kernel);
    }
    CHECK(first == R && nmix <= 1);
    CHECK(all_engine == !pl.concurrent);
    CHECK(pl.reg1 == (in.scan1 == 2 && in.N <= 1280));
    if (in.timers || pl.groups.size() < 2) CHECK(!pl.concurrent || nmix == 1);
    conc += pl.concurrent;
    b2b += !pl.concurrent;
    split += in.split_fgd && pl.concurrent;
    mixed += nmix;
  }
  CHECK(kernels.size() == 6 && conc > 0 && b2b > 0 && split > 0 && mixed > 0);
  check_run_plan_cases();
  const long formulas = check_run_formulas();
  std::printf("run_plan: cases=9 fuzz=%d concurrent=%d back_to_back=%d split=%d mix=%d kernels=%zu formulas=%ld\n", cases, conc,
              b2b, split, mixed, kernels.size(), formulas);
}

// ---- the node-sharded runs' slices against what their call sites computed ----
void check_shard_slices() {
  long n = 0;
  for (int world = 1; world <= 16; ++world)
    for (int nmax = 64; nmax <= 200000; ++nmax) {
      for (int cus : {8, 256, 304}) {
        for (int pol : {(int)POL_BESTFIT, (int)POL_CLUSTERING}) {  // (the cheap policies' layouts differ in the tags only)
          // run_replay_group: slices of about 384 nodes, at most 256 columns in all, widened until the layout fits
          int K = std::max(1, std::min(256 / world, (nmax + 383) / 384));
          K = std::min(K, std::max(1, cus / world));
          int S = (nmax + K - 1) / K;
          while (old_replay_lds(S, pol, false) > 160 * 1024 && (K + 1) * world <= std::min(256, cus)) {
            ++K;
            S = (nmax + K - 1) / K;
          }
          const bool fits = !(world * K < 2 || old_replay_lds(S, pol, false) > 160 * 1024);
          const ShardSlices sl = replay_group_slices(nmax, world, cus, pol);
          CHECK(sl.K == K && sl.S == S && sl.ok == fits);
          ++n;
        }
        {  // run_hmemo_group
          const hmemo::HSlices h = hmemo::hmemo_slices(nmax, std::max(1, std::min(64, cus / world)), hmemo::kClamp);
          const ShardSlices sl = hmemo::hmemo_group_slices(nmax, world, cus);
          CHECK(sl.K == h.K && sl.S == h.S && sl.ok == !(h.K < 1 || world * h.K > 256 || h.K * h.S < nmax));
          ++n;
        }
      }
      // run_hmemo_peer: the shard sizes a cluster of about world x nmax nodes is cut into
      for (int n_global : {world * nmax, world * nmax - world + 1})
        for (int N : {nmax, nmax - 1, nmax + 4096}) {
          const int nm = (n_global + world - 1) / world;
          const hmemo::HSlices h = hmemo::hmemo_slices(nm, std::max(1, 64 / world), hmemo::kClampKeepK);
          const ShardSlices sl = hmemo::hmemo_peer_slices(n_global, world, N);
          CHECK(sl.K == h.K && sl.S == h.S && sl.ok == !(world * h.K > 256 || N > h.K * h.S));
          ++n;
        }
    }
  // replay_group_slices with a requested width (KSIM_TEST group_k), written out: the request replaces the 384-node
  // rule only -- the clamps (256 / world, cus / world, nmax), the LDS widening and `ok` stay
  const int BF = (int)POL_BESTFIT, CL = (int)POL_CLUSTERING;
  const struct { int nmax, world, cus, pol, k_req, K, S; bool ok; } want[] = {
      {300, 2, 256, BF, 0, 1, 300, true},       // no request: one slice per shard, two columns
      {300, 2, 256, BF, 33, 33, 10, true},      // 66 columns
      {200, 3, 256, CL, 43, 43, 5, true},       // 129
      {120, 5, 256, BF, 51, 51, 3, true},       // 255
      {300, 2, 256, BF, 128, 128, 3, true},     // 256
      {300, 2, 304, BF, 200, 128, 3, true},     // above 256 / world
      {200, 3, 304, BF, 1000, 85, 3, true},     // above 256 / world, which is not a power of two
      {300, 2, 64, BF, 100, 32, 10, true},      // above cus / world
      {40, 2, 256, CL, 100, 40, 1, true},       // above nmax: one node per slice
      {250, 1, 256, BF, 250, 250, 1, true},     // a world of one, wide
      {250, 1, 256, BF, 1, 1, 250, false},      // a single column: not ok, as without a request
      {50, 16, 256, BF, 64, 16, 4, true},       // sixteen shards
      // the LDS widening still applies: 32 B per slot beside the 5248 B of shared state, so S + 1 <= 4956
      {100000, 2, 256, BF, 2, 21, 4762, true},
  };
  for (const auto& c : want) {
    const ShardSlices sl = replay_group_slices(c.nmax, c.world, c.cus, c.pol, c.k_req);
    CHECK(sl.K == c.K && sl.S == c.S && sl.ok == c.ok);
    CHECK(c.world * sl.K <= 256 && (long)sl.K * sl.S >= c.nmax);
  }
  std::printf("shard_slices: compared=%ld\n", n);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <node csv> <pod csv>\n", argv[0]);
    return 2;
  }
  fuzz_memo(400);
  fuzz_hmemo(300);
  check_recorded(argv[1], argv[2]);
  check_slices();
  check_forms();
  fuzz_run_plan(3000);
  check_shard_slices();
  std::printf("ok\n");
  return 0;
}
