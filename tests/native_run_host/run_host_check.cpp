// ksim_run_host.hpp on the CPU: the per-run diagnostics record, note_kernel, run_path against a literal copy of the
// if-chain ksim_engine_last_run_path had before the record existed, and the transport predicates against the
// entry point x transport table of DESIGN.md, held here as data.
// Exit status 0 and a line of tallies per check when everything holds; the first broken expectation aborts.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ksim_run_host.hpp"

#define CHECK(x)                                                          \
  do {                                                                    \
    if (!(x)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      std::abort();                                                       \
    }                                                                     \
  } while (0)

static void check_zero() {
  const RunStats s{};
  CHECK(s.K == 0 && s.memo == 0 && s.hmemo == 0 && s.rgo == 0 && s.scan1 == 0);
  CHECK(s.launches == 0 && s.streams == 0 && s.ovl == 0 && s.gate == 0);
  CHECK(s.kernels.empty() && !s.step_path && s.steps == 0 && s.ms == 0.0 && s.report_ms == 0.0);
  RunStats used;
  used.K = 7, used.memo = 1, used.hmemo = 2, used.rgo = 3, used.scan1 = 4, used.launches = 5, used.streams = 6, used.ovl = 8;
  used.gate = -1, used.kernels = "k_memo+k_replay", used.step_path = true, used.steps = 99, used.ms = 1.5, used.report_ms = 0.5;
  used = RunStats{};  // what every run starts with
  CHECK(used.K == 0 && used.memo == 0 && used.hmemo == 0 && used.rgo == 0 && used.scan1 == 0 && used.launches == 0);
  CHECK(used.streams == 0 && used.ovl == 0 && used.gate == 0 && used.kernels.empty() && !used.step_path);
  CHECK(used.steps == 0 && used.ms == 0.0 && used.report_ms == 0.0);
  std::printf("zero: fields=14\n");
}

static void check_note_kernel() {
  RunStats s;
  note_kernel(s, "k_memo");
  CHECK(s.kernels == "k_memo");
  note_kernel(s, "k_memo");  // each name once
  CHECK(s.kernels == "k_memo");
  note_kernel(s, "k_scan1_mix");
  note_kernel(s, "k_replay");
  note_kernel(s, "k_scan1_mix");
  note_kernel(s, "k_memo");
  note_kernel(s, "k_replay");
  CHECK(s.kernels == "k_memo+k_scan1_mix+k_replay");  // launch order
  note_kernel(s, "k_scan1");  // a prefix of a name already there is another name
  note_kernel(s, "k_memo_hkeys");
  note_kernel(s, "k_step+k_step_pwr");  // a joined pair goes in as given
  CHECK(s.kernels == "k_memo+k_scan1_mix+k_replay+k_scan1+k_memo_hkeys+k_step+k_step_pwr");
  note_kernel(s, "k_step");
  CHECK(s.kernels == "k_memo+k_scan1_mix+k_replay+k_scan1+k_memo_hkeys+k_step+k_step_pwr");
  std::printf("note_kernel: names=7\n");
}

// ksim_engine_last_run_path as it was written over the loose last_* members
static int parent_path(int shard_world, int run_mode, bool last_step_path, int last_rgo, int last_scan1, int last_memo,
                       int last_hmemo, int R) {
  int path;
  if (shard_world > 0) path = KSIM_PATH_SHARDED;
  else if (run_mode == 1 || last_step_path) path = KSIM_PATH_STEP;
  else if (last_rgo == R) path = KSIM_PATH_RANDOM_GO;
  else if (last_scan1 == R) path = KSIM_PATH_SCAN1;
  else if (last_memo == 0 && last_hmemo == 0) path = KSIM_PATH_REPLAY;
  else if (last_memo == R) path = KSIM_PATH_MEMO;
  else if (last_hmemo == R) path = KSIM_PATH_HMEMO;
  else path = KSIM_PATH_MIXED;
  return path;
}

static void check_run_path() {
  long cases = 0;
  int seen[8] = {0};
  for (int R = 1; R <= 3; ++R)
    for (int memo = 0; memo <= R; ++memo)
      for (int hmemo = 0; memo + hmemo <= R; ++hmemo)
        for (int rgo = 0; memo + hmemo + rgo <= R; ++rgo)
          for (int scan1 = 0; memo + hmemo + rgo + scan1 <= R; ++scan1)
            for (int mode = 0; mode <= 3; ++mode)
              for (int step = 0; step <= 1; ++step)
                for (int sharded = 0; sharded <= 1; ++sharded) {
                  RunStats s;
                  s.memo = memo, s.hmemo = hmemo, s.rgo = rgo, s.scan1 = scan1, s.step_path = step != 0;
                  const int got = run_path(s, R, mode, sharded != 0);
                  CHECK(got == parent_path(sharded ? 2 : 0, mode, step != 0, rgo, scan1, memo, hmemo, R));
                  CHECK(got >= 0 && got < 8);
                  ++seen[got];
                  ++cases;
                }
  for (int p = 0; p < 8; ++p) CHECK(seen[p] > 0);  // every KSIM_PATH_* value is reached
  std::printf("run_path: cases=%ld paths=8\n", cases);
}

// ---- the entry point x transport table (node-sharded runs) ----
enum { kOk = KSIM_OK, kEInval = KSIM_EINVAL, kEState = KSIM_ESTATE };
enum Route { kUnsharded, kStep, kPeer, kRefused };  // ksim_engine_run: the path taken, or KSIM_ESTATE
struct Row {
  const char* what;
  ShardTransport t;
  int world;
  bool fn;        // an exchange function is installed
  bool exported;  // ksim_shard_peer_handle has exported the own buffer
  int set_shard, set_exchange, peer_handle, set_peers;
  Route run;
  int group;  // ksim_shard_group_run / ksim_shard_group_get_reports, the membership test (rank, world and device right)
};
static const Row kTable[] = {
    // what                          transport              world fn     exported set_shard set_exch peer_hdl set_peers run         group
    {"unsharded",                    ShardTransport::none,  0,    false, false,   kOk,       kEState,  kEState,  kEState,   kUnsharded, kEInval},
    {"group, world 1",               ShardTransport::group, 1,    false, false,   kEState,   kOk,      kOk,      kEState,   kStep,      kOk},
    {"group, world 4",               ShardTransport::group, 4,    false, false,   kEState,   kOk,      kOk,      kEState,   kRefused,   kOk},
    {"group, buffer exported",       ShardTransport::group, 4,    false, true,    kEState,   kOk,      kOk,      kOk,       kRefused,   kOk},
    {"rccl, world 1",                ShardTransport::rccl,  1,    false, false,   kEState,   kEState,  kEState,  kEState,   kStep,      kEInval},
    {"rccl, world 4",                ShardTransport::rccl,  4,    false, false,   kEState,   kEState,  kEState,  kEState,   kStep,      kEInval},
    {"host, world 1",                ShardTransport::host,  1,    true,  false,   kEState,   kOk,      kEState,  kEState,   kStep,      kEInval},
    {"host, world 4",                ShardTransport::host,  4,    true,  false,   kEState,   kOk,      kEState,  kEState,   kStep,      kEInval},
    {"host, buffer exported before", ShardTransport::host,  4,    true,  true,    kEState,   kOk,      kEState,  kOk,       kStep,      kEInval},
    {"peer, world 1",                ShardTransport::peer,  1,    false, true,    kEState,   kOk,      kOk,      kEState,   kPeer,      kOk},
    {"peer, world 4",                ShardTransport::peer,  4,    false, true,    kEState,   kOk,      kOk,      kEState,   kPeer,      kOk},
    {"peer, a function installed",   ShardTransport::peer,  4,    true,  true,    kEState,   kOk,      kEState,  kEState,   kPeer,      kEInval},
};

// what each entry point does with the predicates, and nothing else
static int rc_set_shard(const Row& r) { return shard_on(r.t) ? kEState : kOk; }
static int rc_set_exchange(const Row& r) { return takes_exchange_fn(r.t) ? kOk : kEState; }
static int rc_peer_handle(const Row& r) { return in_process(r.t, r.fn) ? kOk : kEState; }
static int rc_set_peers(const Row& r) { return can_map_peers(r.t, r.exported) ? kOk : kEState; }
static Route route_run(const Row& r) {
  if (runs_peer(r.t)) return kPeer;
  if (!shard_on(r.t)) return kUnsharded;
  if (exchanges_on_host(r.t)) return kStep;
  if (needs_group_run(r.t, r.world)) return kRefused;
  return kStep;  // over RCCL, or a world of one
}
static int rc_group(const Row& r) { return in_process(r.t, r.fn) ? kOk : kEInval; }

static void check_transport_table() {
  int rows = 0;
  for (const Row& r : kTable) {
    if (rc_set_shard(r) != r.set_shard || rc_set_exchange(r) != r.set_exchange || rc_peer_handle(r) != r.peer_handle ||
        rc_set_peers(r) != r.set_peers || route_run(r) != r.run || rc_group(r) != r.group) {
      std::fprintf(stderr, "transport table: row '%s' does not hold\n", r.what);
      std::abort();
    }
    // one transport at a time: the collective only on rccl, the host function only called on host
    CHECK(exchanges_by_rccl(r.t) == (r.t == ShardTransport::rccl));
    CHECK(exchanges_on_host(r.t) == (r.t == ShardTransport::host));
    ++rows;
  }
  std::printf("transport: rows=%d entry_points=6\n", rows);
}

int main() {
  check_zero();
  check_note_kernel();
  check_run_path();
  check_transport_table();
  std::printf("ok\n");
  return 0;
}
