// ksim_run_host.hpp -- what a run leaves for the diagnostics getters, and which transport a node-sharded engine uses.
//
// Host-only (no HIP type, no device call): the engine includes it, and so does the stand-alone check program
// tests/native_run_host/run_host_check.cpp.
#pragma once

#include <cstdint>
#include <string>

#include "ksim_engine.h"

// Every per-run diagnostic (the ksim_engine_last_* getters).  ksim_engine_run and ksim_shard_group_run start with
// stats = RunStats{}: after a successful run every getter reports that run alone.  (gate_timeouts counts over the
// engine's life and stays in the engine.)
struct RunStats {
  int K = 0;         // workgroups per replica of the last replay launch that has a width (0: none had one)
  int memo = 0, hmemo = 0, rgo = 0, scan1 = 0;  // replicas replayed on k_memo / k_hmemo / k_random_go / k_scan1
  int launches = 0, streams = 0;                // replay launches, side streams they ran on (0: none)
  int wsum = 0;      // replicas replayed on k_wsum (the weighted combinations)
  int ovl = 0;       // replicas the overlapped report took (k_report_overlap)
  int gate = 0;      // the residency gate: 0 none, 1 opened, -1 given up at its bound (stderr note)
  std::string kernels;     // the replay kernels launched, '+'-joined in launch order, each name once
  bool step_path = false;  // the run went through k_step (run_mode 1)
  int64_t steps = 0;
  double ms = 0, report_ms = 0;
};

inline void note_kernel(RunStats& s, const char* name) {
  for (size_t p = 0; p < s.kernels.size();) {  // each name once
    size_t q = s.kernels.find('+', p);
    if (q == std::string::npos) q = s.kernels.size();
    if (s.kernels.compare(p, q - p, name) == 0) return;
    p = q + 1;
  }
  if (!s.kernels.empty()) s.kernels += '+';
  s.kernels += name;
}

// ksim_engine_last_run_path of an engine of R replicas.
inline int run_path(const RunStats& s, int R, int run_mode, bool sharded) {
  if (sharded) return KSIM_PATH_SHARDED;
  if (run_mode == 1 || s.step_path) return KSIM_PATH_STEP;
  if (s.rgo == R) return KSIM_PATH_RANDOM_GO;
  if (s.scan1 == R) return KSIM_PATH_SCAN1;
  if (s.wsum == R && R > 0) return KSIM_PATH_WSUM;
  if (s.memo == 0 && s.hmemo == 0) return KSIM_PATH_REPLAY;
  if (s.memo == R) return KSIM_PATH_MEMO;
  if (s.hmemo == R) return KSIM_PATH_HMEMO;
  return KSIM_PATH_MIXED;
}

// How a node-sharded engine's records travel between the shards.  One value, set where it is established:
//   none   not sharded (before ksim_engine_set_shard)
//   group  set_shard without a communicator id: an in-process group's shard (ksim_shard_group_run), or a world of one;
//          an engine that has exported its peer buffer but mapped no peers is still this
//   rccl   set_shard with a communicator id
//   host   ksim_engine_set_shard_exchange with a function
//   peer   ksim_engine_set_shard_peers has mapped the peers' buffers
enum class ShardTransport { none, group, rccl, host, peer };

// The entry points decide through these (DESIGN.md has the table; tests/native_run_host holds it as data).
inline bool shard_on(ShardTransport t) { return t != ShardTransport::none; }
inline bool runs_peer(ShardTransport t) { return t == ShardTransport::peer; }              // ksim_engine_run: k_hmemo
inline bool exchanges_on_host(ShardTransport t) { return t == ShardTransport::host; }      // run_sharded, step by step
inline bool exchanges_by_rccl(ShardTransport t) { return t == ShardTransport::rccl; }
// ksim_engine_run of a group's shard: only a world of one runs by itself, the others through ksim_shard_group_run
inline bool needs_group_run(ShardTransport t, int world) { return t == ShardTransport::group && world > 1; }
inline bool takes_exchange_fn(ShardTransport t) { return shard_on(t) && t != ShardTransport::rccl; }
// ksim_shard_peer_handle and the group entry points: no communicator and no exchange function.  A function installed
// on a peer-mapped engine (the one pair of calls that leaves two transports' marks) is kept and never called;
// `fn` says one is installed.
inline bool in_process(ShardTransport t, bool fn) { return (t == ShardTransport::group || t == ShardTransport::peer) && !fn; }
// ksim_engine_set_shard_peers: the own buffer exported (`exported`) and nothing mapped yet
inline bool can_map_peers(ShardTransport t, bool exported) {
  return exported && (t == ShardTransport::group || t == ShardTransport::host);
}
