// Host-only check of k_wsum's LDS layout (ksim_plan.hpp wsum_layout / wsum_lds / wsum_fits) and of the run plan with
// KSIM_POLICY_WEIGHTED replicas (make_run_plan).  No GPU, no HIP runtime: hipcc's host pass over the planner's header.
// It aborts on the first broken expectation and prints its tallies; tests/test_wsum_plan_cpu.py reads them.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ksim_plan.hpp"

using namespace ksim_plan;

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::fprintf(stderr, "wsum_plan_check:%d: %s\n", __LINE__, #c);         \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

static const unsigned kAll = (1u << POL_FGD) | (1u << POL_BESTFIT) | (1u << POL_DOTPROD) | (1u << POL_PACKING) |
                             (1u << POL_CLUSTERING) | (1u << POL_PWR);

// ---- the layout: regions in order, 16-B aligned, sized by the mask; monotone in N; the refusal bound ----
static void check_layout() {
  long cases = 0;
  int max_all = 0, max_lean = 0;
  for (unsigned mask = 0; mask < 128; ++mask) {
    if (mask & (1u << POL_RANDOM)) continue;
    for (int general = 0; general < 2; ++general) {
      size_t prev = 0;
      int largest = 0;
      for (int N = 1; N <= 4200; ++N) {
        const wsum::WLayout L = wsum::wsum_layout(N, mask, general);
        CHECK(L.nodes == wsum::kSharedBytes && L.sc == L.nodes + (size_t)N * 32 && L.tags == L.sc + (size_t)N * 16);
        CHECK(L.F0 == L.tags + (((mask >> POL_CLUSTERING) & 1u) ? (size_t)N * 32 : 0));
        CHECK(L.last == L.F0 + (((mask >> POL_FGD) & 1u) ? (size_t)N * 8 : 0));
        CHECK(L.total >= L.last + (general ? (size_t)N * 4 : 0) && L.total < L.last + (general ? (size_t)N * 4 : 0) + 16);
        CHECK(L.nodes % 16 == 0 && L.sc % 16 == 0 && L.tags % 16 == 0 && L.F0 % 8 == 0 && L.last % 4 == 0);
        CHECK(L.total == wsum::wsum_lds(N, mask, general) && L.total > prev);  // strictly monotone in N
        prev = L.total;
        const bool fits = wsum::wsum_fits(N, mask, general);
        CHECK(fits == (N <= wsum::kMaxNodes && L.total <= kLdsMax));
        if (fits) {
          CHECK(largest == N - 1);  // the sizes that fit are 1 .. largest
          largest = N;
        }
        ++cases;
      }
      CHECK(largest >= 1213);  // the openb cluster fits under every mask, with the report's record too
      if (mask == kAll && general) max_all = largest;
      if (mask == ((1u << POL_BESTFIT) | (1u << POL_PACKING)) && !general) max_lean = largest;
      // more plugins never need less
      CHECK(wsum::wsum_lds(1213, mask, general) <= wsum::wsum_lds(1213, kAll, general));
    }
  }
  CHECK(!wsum::wsum_fits(0, kAll, true) && !wsum::wsum_fits(max_all + 1, kAll, true));
  // the bounds in closed form: 92 B per node with everything on (record 32, scores 16, tags 32, F0 8, last 4), 48 B
  // with the cheap plugins alone; one workgroup's LDS ends before the packed key's slot field (kMaxNodes) would
  CHECK(max_all == (int)((kLdsMax - wsum::kSharedBytes) / 92) && max_lean == (int)((kLdsMax - wsum::kSharedBytes) / 48));
  CHECK(max_lean <= wsum::kMaxNodes);
  std::printf("layout: cases=%ld lds_1213_all_report=%zu max_all_report=%d max_lean=%d\n", cases,
              wsum::wsum_lds(1213, kAll, true), max_all, max_lean);
  const int32_t w[7] = {700, 300, 0, 0, 0, 0, 5};
  CHECK(wsum::plugin_mask(w) == ((1u << POL_FGD) | (1u << POL_BESTFIT) | (1u << POL_PWR)));
}

// ---- the run plan ----
static RunReplica rr(int policy, int n_events = 300, bool go = false, bool del = false) { return {policy, go, n_events, del, 0}; }
static RunReplica ww(unsigned mask, int n_events = 300, bool del = false) {
  RunReplica r = rr(POL_WEIGHTED, n_events, false, del);
  r.wmask = mask;
  return r;
}
static RunPlanInput base(std::vector<RunReplica> reps) {  // the openb default cluster, 256 CUs, one workgroup per replica
  RunPlanInput in;
  in.reps = std::move(reps);
  in.N = 1213;
  in.cus = 256;
  in.wgs_req = 1;
  in.scan1 = 2;
  in.side_streams = 4;
  return in;
}
static RunPlanInput hmemo1(RunPlanInput in, std::vector<int> reps) {
  in.hmemo_ok = true;
  in.hmemo_K = 1;
  in.hmemo_reps = std::move(reps);
  return in;
}

// The inputs of the nine cases of tests/test_gpu_run_plan.py, by value.
static std::vector<RunPlanInput> nine() {
  std::vector<RunPlanInput> v;
  const std::vector<RunReplica> sweep = {rr(POL_FGD), rr(POL_FGD, 260), rr(POL_BESTFIT, 280), rr(POL_PACKING)};
  v.push_back(hmemo1(base(sweep), {0, 1}));
  v.push_back(hmemo1(base(sweep), {0, 1}));
  v.back().report = true;
  v.push_back(base({rr(POL_FGD), rr(POL_BESTFIT)}));
  v.back().wgs_req = 0;
  v.back().memo_ok = true;
  v.back().memo_nwg = 64;
  v.back().memo_reps = {0};
  v.push_back(hmemo1(base(sweep), {1}));
  v.back().split_fgd = v.back().memo_ok = true;
  v.back().memo_nwg = 6;
  v.back().memo_reps = {0};
  v.push_back(base({rr(POL_PACKING, 299, false, true), rr(POL_BESTFIT)}));
  v.push_back(base({rr(POL_RANDOM, 300, true), rr(POL_BESTFIT, 280), rr(POL_PACKING)}));
  for (int nq : {1, 2}) {
    v.push_back(base({rr(POL_BESTFIT), rr(POL_DOTPROD, 260), rr(POL_PACKING, 280), rr(POL_CLUSTERING, 240), rr(POL_RANDOM)}));
    v.back().scan1_mix = false;
    v.back().side_streams = nq;
  }
  v.push_back(base({rr(POL_PWR_FGD)}));
  v.back().run_mode = 2;
  return v;
}

struct Want {
  std::vector<int> order;
  std::vector<std::vector<int>> groups;  // kind, count, kernel, side, K
  bool concurrent;
};

static void check_plans() {
  const int mix = scan1::kPolMix;
  // today's plans of the nine inputs (what tests/native_host/plan_check.cpp holds them to)
  const std::vector<Want> want = {
      {{0, 1, 3, 2}, {{POL_FGD, 2, kRunHmemo, 0, 1}, {mix, 2, kRunScan1, 1, 1}}, true},
      {{0, 1, 3, 2}, {{POL_FGD, 2, kRunHmemo, 0, 1}, {mix, 2, kRunScan1, 1, 1}}, true},
      {{0, 1}, {{POL_FGD, 1, kRunMemo, -1, 1}, {POL_BESTFIT, 1, kRunReplay, -1, 64}}, false},
      {{0, 1, 3, 2}, {{POL_FGD, 1, kRunMemo, -1, 1}, {kPolFgdH, 1, kRunHmemo, 0, 1}, {mix, 2, kRunScan1, 1, 1}}, true},
      {{1, 0}, {{POL_BESTFIT, 1, kRunReplay, 0, 1}, {POL_PACKING, 1, kRunReplay, 1, 1}}, true},
      {{2, 1, 0}, {{mix, 2, kRunScan1, 0, 1}, {kPolRandomGo, 1, kRunRandomGo, 1, 1}}, true},
      {{0, 1, 2, 3, 4},
       {{POL_BESTFIT, 1, kRunScan1, 0, 1}, {POL_DOTPROD, 1, kRunScan1, 0, 1}, {POL_PACKING, 1, kRunScan1, 0, 1},
        {POL_CLUSTERING, 1, kRunScan1, 0, 1}, {POL_RANDOM, 1, kRunScan1, 0, 1}}, true},
      {{0, 1, 2, 3, 4},
       {{POL_BESTFIT, 1, kRunScan1, 0, 1}, {POL_DOTPROD, 1, kRunScan1, 1, 1}, {POL_PACKING, 1, kRunScan1, 1, 1},
        {POL_CLUSTERING, 1, kRunScan1, 1, 1}, {POL_RANDOM, 1, kRunScan1, 1, 1}}, true},
      {{0}, {{POL_PWR_FGD, 1, kRunReplay, -1, 1}}, false},
  };
  const std::vector<RunPlanInput> ins = nine();
  CHECK(ins.size() == 9 && want.size() == 9);
  int unchanged = 0, with_weighted = 0, side = 0;
  for (size_t c = 0; c < ins.size(); ++c) {
    // without a WEIGHTED replica: exactly today's plan, and no k_wsum group
    const RunPlan pl = make_run_plan(ins[c]);
    CHECK(pl.order == want[c].order && pl.groups.size() == want[c].groups.size() && pl.concurrent == want[c].concurrent);
    int first = 0;
    for (size_t i = 0; i < pl.groups.size(); ++i) {
      const PlanGroup& g = pl.groups[i];
      const std::vector<int>& w = want[c].groups[i];
      CHECK(g.kind == w[0] && g.count == w[1] && g.kernel == w[2] && g.side == w[3] && g.K == w[4] && g.first == first);
      CHECK(g.kernel != kRunWsum && g.wmask == 0u);
      first += g.count;
    }
    ++unchanged;
    // with two WEIGHTED replicas appended: one more group, after the policies' and before Go's Random; the other
    // groups keep their kind, replicas, kernel and width
    RunPlanInput in = ins[c];
    const int R0 = (int)in.reps.size();
    const unsigned m0 = (1u << POL_FGD) | (1u << POL_BESTFIT), m1 = (1u << POL_PWR) | (1u << POL_PACKING);
    in.reps.push_back(ww(m0));
    in.reps.push_back(ww(m1, 250));
    const RunPlan pw = make_run_plan(in);
    CHECK(pw.groups.size() == pl.groups.size() + 1 && pw.general == pl.general && pw.any_delete == pl.any_delete);
    const bool go_last = pl.groups.back().kind == kPolRandomGo;
    const size_t at = go_last ? pl.groups.size() - 1 : pl.groups.size();
    const PlanGroup& g = pw.groups[at];
    CHECK(g.kind == POL_WEIGHTED && g.kernel == kRunWsum && g.count == 2 && g.K == 1 && g.S == in.N);
    CHECK(g.wmask == (m0 | m1) && g.lds == wsum::wsum_lds(in.N, m0 | m1, pw.general));
    CHECK(pw.order[g.first] == R0 && pw.order[g.first + 1] == R0 + 1);
    std::vector<int> rest;
    for (int r : pw.order)
      if (r < R0) rest.push_back(r);
    CHECK(rest == pl.order);
    first = 0;
    for (size_t i = 0, j = 0; i < pw.groups.size(); ++i) {
      CHECK(pw.groups[i].first == first);
      first += pw.groups[i].count;
      if (i == at) continue;
      const PlanGroup &a = pw.groups[i], &b = pl.groups[j++];
      CHECK(a.kind == b.kind && a.count == b.count && a.kernel == b.kernel && a.K == b.K && a.lds == b.lds);
    }
    // K = 1 and no exchange: it never takes a run off the side streams, and runs on one when the run is concurrent
    if (pl.concurrent) CHECK(pw.concurrent);
    CHECK((g.side >= 0) == pw.concurrent && g.side < in.side_streams);
    side += g.side >= 0;
    ++with_weighted;
  }
  // WEIGHTED replicas alone: one launch on the engine stream; two kinds: side streams; deletes / the report make the
  // general instantiation's layout
  {
    const RunPlan pl = make_run_plan(base({ww(kAll), ww(1u << POL_BESTFIT)}));
    CHECK(pl.groups.size() == 1 && pl.groups[0].kernel == kRunWsum && pl.groups[0].side == -1 && !pl.concurrent);
    CHECK(pl.order == (std::vector<int>{0, 1}) && pl.groups[0].lds == wsum::wsum_lds(1213, kAll, false));
    RunPlanInput in = base({ww(kAll, 300, true), rr(POL_FGD)});
    in.report = true;
    const RunPlan pg = make_run_plan(in);
    CHECK(pg.general && pg.groups.size() == 2 && pg.groups[1].kind == POL_WEIGHTED && pg.order == (std::vector<int>{1, 0}));
    CHECK(pg.groups[1].lds == wsum::wsum_lds(1213, kAll, true) && pg.groups[1].lds <= kLdsMax);
    in.timers = true;  // the profile timers keep every launch on the engine stream
    const RunPlan pt = make_run_plan(in);
    CHECK(!pt.concurrent && pt.groups[1].side == -1);
  }
  std::printf("run_plan: unchanged=%d with_weighted=%d on_side_stream=%d\n", unchanged, with_weighted, side);
}

int main() {
  check_layout();
  check_plans();
  std::printf("ok\n");
  return 0;
}
