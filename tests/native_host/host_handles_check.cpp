// The owning handles of ksim_host.hpp (DevBuf, DevEvent, DevStream, MappedFlags, GraphExec, PeerMap, the communicator's
// DevHandle) on the CPU: malloc-backed stand-ins for the HIP calls they make count the live objects of each kind and
// fail the k-th call on request.
// Exit status 0 and a line of tallies per check when everything holds; the first broken expectation aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

// ---- the stand-ins ----
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
typedef struct FakeStream* hipStream_t;
typedef struct FakeEvent* hipEvent_t;
typedef struct FakeGraphExec* hipGraphExec_t;
struct FakeStream { int flags; };
struct FakeEvent { unsigned flags; };
struct FakeGraphExec { int unused; };
constexpr unsigned hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1, hipHostMallocMapped = 2,
                   hipHostMallocCoherent = 0x40000000, hipDeviceMallocUncached = 3;

#define CHECK(x)                                                          \
  do {                                                                    \
    if (!(x)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      std::abort();                                                       \
    }                                                                     \
  } while (0)

struct Tally {
  std::set<void*> blocks, host;            // live device blocks (uncached ones too), live host-mapped blocks
  std::set<hipEvent_t> events;
  std::set<hipStream_t> streams;
  std::set<hipGraphExec_t> graphs;
  long calls = 0, fail_at = 0;             // fallible calls so far; the one to fail (0: none)
  long mallocs = 0, ext_mallocs = 0, frees = 0, copies = 0, copied_bytes = 0, memsets = 0, event_creates = 0,
       stream_creates = 0, host_mallocs = 0;
  size_t last_bytes = 0;
  std::set<void*> ipc;                     // live IPC mappings
  std::set<struct FakeComm*> comms;        // live communicators
  std::vector<int> ipc_ranks;              // the rank each open named, in call order
  long ipc_opens = 0, ipc_closes = 0, comm_destroys = 0;
  bool none_live() const {
    return blocks.empty() && host.empty() && events.empty() && streams.empty() && graphs.empty() && ipc.empty() &&
           comms.empty();
  }
};
static Tally T;

static bool injected() { return ++T.calls == T.fail_at; }
static void* garbage(size_t bytes) {  // fresh memory is not zero
  void* p = std::malloc(bytes);
  CHECK(p);
  std::memset(p, 0xab, bytes);
  return p;
}

static hipError_t hipMalloc(void** p, size_t bytes) {
  if (injected()) return hipErrorOutOfMemory;
  CHECK(bytes > 0);
  ++T.mallocs;
  T.last_bytes = bytes;
  T.blocks.insert(*p = garbage(bytes));
  return hipSuccess;
}
static hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned flags) {
  if (injected()) return hipErrorOutOfMemory;
  CHECK(bytes > 0 && flags == hipDeviceMallocUncached);
  ++T.ext_mallocs;
  T.last_bytes = bytes;
  T.blocks.insert(*p = garbage(bytes));
  return hipSuccess;
}
static hipError_t hipFree(void* p) {
  CHECK(T.blocks.erase(p) == 1);  // freed once, and only what was allocated
  ++T.frees;
  std::free(p);
  return hipSuccess;
}
static hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  if (injected()) return hipErrorOutOfMemory;
  CHECK(kind == hipMemcpyHostToDevice);
  ++T.copies;
  T.copied_bytes += (long)bytes;
  if (bytes) std::memcpy(dst, src, bytes);
  return hipSuccess;
}
static hipError_t hipMemsetAsync(void* dst, int byte, size_t bytes, hipStream_t) {
  if (injected()) return hipErrorOutOfMemory;
  ++T.memsets;
  std::memset(dst, byte, bytes);
  return hipSuccess;
}
// (the destroyers are template arguments of the handles: external linkage)
static hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned flags) {
  if (injected()) return hipErrorOutOfMemory;
  ++T.event_creates;
  T.events.insert(*ev = new FakeEvent{flags});
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t ev) {
  CHECK(T.events.erase(ev) == 1);
  delete ev;
  return hipSuccess;
}
static hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
  if (injected()) return hipErrorOutOfMemory;
  CHECK(flags == hipStreamNonBlocking);
  ++T.stream_creates;
  T.streams.insert(*s = new FakeStream{(int)flags});
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  CHECK(T.streams.erase(s) == 1);
  delete s;
  return hipSuccess;
}
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
  if (injected()) return hipErrorOutOfMemory;
  CHECK(bytes > 0 && flags == (hipHostMallocMapped | hipHostMallocCoherent));
  ++T.host_mallocs;
  T.host.insert(*p = garbage(bytes));
  return hipSuccess;
}
static hipError_t hipHostFree(void* p) {
  CHECK(T.host.erase(p) == 1);
  std::free(p);
  return hipSuccess;
}
static hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) {
  if (injected()) return hipErrorOutOfMemory;
  CHECK(T.host.count(h) == 1);
  *d = h;
  return hipSuccess;
}
// IPC: a handle names its rank in its first byte; an opened mapping is a block of its own, closed once
struct hipIpcMemHandle_t { char reserved[64]; };
constexpr unsigned hipIpcMemLazyEnablePeerAccess = 1;
static hipError_t hipIpcOpenMemHandle(void** p, hipIpcMemHandle_t h, unsigned flags) {
  if (injected()) return hipErrorOutOfMemory;
  CHECK(flags == hipIpcMemLazyEnablePeerAccess);
  ++T.ipc_opens;
  T.ipc_ranks.push_back(h.reserved[0]);
  T.ipc.insert(*p = garbage(8));
  return hipSuccess;
}
static hipError_t hipIpcCloseMemHandle(void* p) {
  CHECK(T.ipc.erase(p) == 1);  // closed once, and only what was opened: never the own buffer
  ++T.ipc_closes;
  std::free(p);
  return hipSuccess;
}
// the communicator's stand-in: its destroyer counts
typedef struct FakeComm* fakeComm_t;
struct FakeComm { int rank; };
hipError_t fake_comm_destroy(fakeComm_t c) {
  CHECK(T.comms.erase(c) == 1);
  ++T.comm_destroys;
  delete c;
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t g) {
  CHECK(T.graphs.erase(g) == 1);
  delete g;
  return hipSuccess;
}
static hipGraphExec_t fake_graph() {
  hipGraphExec_t g = new FakeGraphExec{0};
  T.graphs.insert(g);
  return g;
}

enum { KSIM_OK = 0, KSIM_EHIP = 3 };
#define KSIM_HIP(x)                        \
  do {                                     \
    if ((x) != hipSuccess) return KSIM_EHIP; \
  } while (0)

#include "ksim_host.hpp"

// ---- the checks ----
static void check_devbuf() {
  {
    DevBuf<int> b;
    bool grew = false;
    CHECK(b.ensure(10, &grew) == KSIM_OK && grew && b.cap == 10 && T.last_bytes == 10 * sizeof(int));
    int* first = b.p;
    CHECK(b.ensure(10, &grew) == KSIM_OK && !grew && b.p == first);  // n <= cap: the block stays
    CHECK(b.ensure(3, &grew) == KSIM_OK && !grew && b.p == first && b.cap == 10);
    CHECK(b.ensure(11, &grew) == KSIM_OK && grew && b.cap == 11 && T.mallocs == 2 && T.frees == 1);  // n > cap
    CHECK(T.blocks.size() == 1);

    DevBuf<double> z;
    CHECK(z.ensure(0, &grew) == KSIM_OK && grew && z.p && z.cap == 0 && T.last_bytes == sizeof(double));  // one element
    CHECK(z.ensure(0, &grew) == KSIM_OK && !grew);

    DevBuf<short> a;
    const long m0 = T.mallocs, f0 = T.frees;
    CHECK(a.alloc(5) == KSIM_OK && a.alloc(5) == KSIM_OK && a.alloc(2) == KSIM_OK);  // always afresh
    CHECK(T.mallocs == m0 + 3 && T.frees == f0 + 2 && a.cap == 2 && T.last_bytes == 2 * sizeof(short));

    DevBuf<int> u;
    const std::vector<int> v{7, 8, 9, 10, 11};
    const long c0 = T.copies, b0 = T.copied_bytes;
    CHECK(u.upload(v, nullptr) == KSIM_OK && u.cap == 5);
    CHECK(T.copies == c0 + 1 && T.copied_bytes == b0 + (long)(5 * sizeof(int)) && std::memcmp(u.p, v.data(), 5 * sizeof(int)) == 0);

    DevBuf<unsigned> f;
    CHECK(f.alloc(6) == KSIM_OK && f.p[0] == 0xababababu);
    CHECK(f.zero(nullptr) == KSIM_OK && f.p[0] == 0 && f.p[5] == 0);
    CHECK(f.fill(0xff, nullptr) == KSIM_OK && f.p[0] == 0xffffffffu && f.p[5] == 0xffffffffu);

    DevBuf<unsigned long long> x;
    CHECK(x.alloc(4, hipDeviceMallocUncached) == KSIM_OK && T.ext_mallocs == 1 && T.last_bytes == 32);

    // a failed allocation leaves the buffer empty, not dangling
    T.fail_at = T.calls + 1;
    CHECK(b.alloc(100) == KSIM_EHIP && !b.p && b.cap == 0);
    T.fail_at = 0;
  }
  CHECK(T.none_live());
  std::printf("devbuf: mallocs=%ld frees=%ld live=%zu\n", T.mallocs + T.ext_mallocs, T.frees, T.blocks.size());
}

static void check_move() {
  {
    DevBuf<int> a;
    CHECK(a.alloc(4) == KSIM_OK);
    int* p = a.p;
    DevBuf<int> b(std::move(a));
    CHECK(!a.p && a.cap == 0 && b.p == p && b.cap == 4);
    DevBuf<int> c;
    CHECK(c.alloc(9) == KSIM_OK);
    const long f0 = T.frees;
    c = std::move(b);  // frees what c held, takes b's
    CHECK(T.frees == f0 + 1 && !b.p && c.p == p && c.cap == 4 && T.blocks.size() == 1);
  }
  CHECK(T.none_live());
  {
    std::vector<DevBuf<int>> v(3);
    for (auto& b : v) CHECK(b.alloc(2) == KSIM_OK);
    const int* p0 = v[0].p;
    CHECK(v.capacity() < 50);
    v.resize(50);  // past its capacity: the elements move
    CHECK(v[0].p == p0 && T.blocks.size() == 3);
    for (size_t i = 3; i < v.size(); ++i) CHECK(!v[i].p);
    CHECK(v[49].alloc(1) == KSIM_OK && T.blocks.size() == 4);
  }
  CHECK(T.none_live());
  std::printf("move: live=%zu\n", T.blocks.size());
}

static void check_event_stream_flags_graph() {
  {
    DevEvent ev, quiet;
    CHECK(!ev && ev.ensure() == KSIM_OK && ev.ensure() == KSIM_OK && T.event_creates == 1 && ev.h->flags == hipEventDefault);
    CHECK(quiet.ensure(hipEventDisableTiming) == KSIM_OK && quiet.h->flags == hipEventDisableTiming);
    hipEvent_t raw = ev;
    DevEvent moved(std::move(ev));
    CHECK(!ev.h && moved.h == raw && T.events.size() == 2);
    std::vector<DevEvent> evs(2);
    for (auto& e : evs) CHECK(e.ensure() == KSIM_OK);
    evs.resize(40);
    CHECK(T.events.size() == 4);

    DevStream s;
    CHECK(!s && s.ensure() == KSIM_OK && s.ensure() == KSIM_OK && T.stream_creates == 1 && (hipStream_t)s == s.h);

    MappedFlags fl;
    CHECK(fl.ensure(8) == KSIM_OK && fl.ensure(8) == KSIM_OK && fl.ensure(5) == KSIM_OK && T.host_mallocs == 1);
    CHECK(fl.cap == 8 && fl.d == fl.h);
    for (int i = 0; i < 8; ++i) CHECK(fl.h[i] == 0);
    fl.h[3] = 77;
    int* old = fl.h;
    CHECK(fl.ensure(20) == KSIM_OK && T.host_mallocs == 2 && T.host.size() == 1 && T.host.count(old) == 0 && fl.cap == 20);
    for (int i = 0; i < 20; ++i) CHECK(fl.h[i] == 0);  // the new block starts zeroed
    T.fail_at = T.calls + 2;  // the device-pointer query of a larger block fails: nothing is held
    CHECK(fl.ensure(30) == KSIM_EHIP && !fl.h && !fl.d && fl.cap == 0 && T.host.empty());
    T.fail_at = 0;
    CHECK(fl.ensure(4) == KSIM_OK);

    GraphExec g;
    CHECK(!g);
    g.reset(fake_graph());
    g.reset(fake_graph());  // destroys the first
    CHECK(T.graphs.size() == 1);
    g.reset();
    CHECK(T.graphs.empty() && !g);
    g.reset(fake_graph());
  }
  CHECK(T.none_live());
  std::printf("handles: events=%ld streams=%ld host=%ld live=0\n", T.event_creates, T.stream_creates, T.host_mallocs);
}

// An engine in small: built like ksim_engine_create (a unique_ptr, an early return on the first error, released to
// the caller on success only).
struct Rec { double a; int b[3]; };
struct Mini {
  DevStream stream;
  DevEvent ev0, ev1, ev_mid;
  DevBuf<Rec> nodes, nodes_init;
  DevBuf<unsigned short> tags;
  DevBuf<int> base, scratch, fail, list;
  DevBuf<unsigned char> feas, cpum;
  DevBuf<double> th;
  DevBuf<unsigned long long> gran, peer;
  std::vector<DevBuf<int>> per;
  MappedFlags started;
};
constexpr int kPer = 5;
static int mini_create(Mini** out) {
  *out = nullptr;
  auto m = std::make_unique<Mini>();
  int rc = m->stream.ensure();
  const auto alloc = [&](auto& buf, size_t n) { if (!rc) rc = buf.alloc(n); };
  const auto zeroed = [&](auto& buf, size_t n) {
    alloc(buf, n);
    if (!rc) rc = buf.zero(m->stream);
  };
  zeroed(m->nodes, 12);
  zeroed(m->nodes_init, 12);
  zeroed(m->tags, 40);
  alloc(m->base, 4);
  alloc(m->scratch, 4);
  alloc(m->fail, 1);
  alloc(m->feas, 12);
  zeroed(m->cpum, 12);
  alloc(m->gran, 64);
  if (!rc) rc = m->peer.alloc(16, hipDeviceMallocUncached);
  if (!rc) rc = m->ev0.ensure();
  if (!rc) rc = m->ev1.ensure();
  if (!rc) rc = m->ev_mid.ensure(hipEventDisableTiming);
  if (rc) return rc;
  m->per.resize(kPer);
  for (auto& b : m->per)
    if ((rc = b.alloc(3))) return rc;
  const std::vector<int> ids{0, 1, 2};
  if ((rc = m->list.upload(ids, m->stream))) return rc;
  const std::vector<double> th(102, 0.5);
  if ((rc = m->th.upload(th, m->stream))) return rc;
  if ((rc = m->started.ensure(6))) return rc;
  *out = m.release();
  return KSIM_OK;
}

static void check_all_or_nothing() {
  CHECK(T.none_live());
  Mini* m = nullptr;
  const long c0 = T.calls;
  CHECK(mini_create(&m) == KSIM_OK && m);
  const long total = T.calls - c0;
  const size_t blocks = 12 + kPer;  // the dozen buffers and the per-replica ones
  CHECK(T.blocks.size() == blocks && T.events.size() == 3 && T.streams.size() == 1 && T.host.size() == 1);
  CHECK(m->list.p[2] == 2 && m->th.p[101] == 0.5 && m->nodes.p[11].b[2] == 0 && m->started.h[5] == 0);
  delete m;
  CHECK(T.none_live());
  // stream 1, 12 + kPer allocations, 4 memsets, 3 events, 2 copies, host block + its device pointer
  CHECK(total == 1 + 12 + kPer + 4 + 3 + 2 + 2);
  for (long k = 1; k <= total; ++k) {
    m = reinterpret_cast<Mini*>(&T);  // must come back null
    T.fail_at = T.calls + k;
    CHECK(mini_create(&m) == KSIM_EHIP);
    T.fail_at = 0;
    CHECK(!m);
    CHECK(T.none_live());
  }
  std::printf("all-or-nothing: calls=%ld failures_injected=%ld blocks=%zu events=3 streams=1 host=1 live_after=0\n", total,
              total, blocks);
}

// PeerMap over a world of 4: every rank but the own one is opened, or none stays open.
static void check_peer_map() {
  constexpr int kWorld = 4;
  constexpr size_t kStride = 128;  // a record is longer than the IPC handle it begins with
  std::vector<uint8_t> handles(kWorld * kStride, 0);
  for (int q = 0; q < kWorld; ++q) handles[q * kStride] = (uint8_t)q;
  DevBuf<unsigned long long> own;
  CHECK(own.alloc(16, hipDeviceMallocUncached) == KSIM_OK);
  long failures = 0;
  for (int rank = 0; rank < kWorld; ++rank) {
    for (int k = 1; k <= kWorld - 1; ++k) {  // the k-th open fails
      PeerMap m;
      const long o0 = T.ipc_opens, c0 = T.ipc_closes;
      T.ipc_ranks.clear();
      T.fail_at = T.calls + k;
      int bad = -1;
      hipError_t why = hipSuccess;
      CHECK(m.open(handles.data(), kStride, kWorld, rank, own.p, &bad, &why) == KSIM_EHIP);
      T.fail_at = 0;
      CHECK(T.ipc_opens == o0 + k - 1 && T.ipc_closes == c0 + k - 1);  // exactly the opened ones are closed
      CHECK(T.ipc.empty() && !m.mapped() && m.ptr.empty());             // the map is empty afterwards
      CHECK(T.blocks.count(own.p) == 1);                                 // the own buffer is untouched
      CHECK(why == hipErrorOutOfMemory && bad != rank && bad == (k - 1 < rank ? k - 1 : k));  // the k-th other rank
      for (int r : T.ipc_ranks) CHECK(r != rank);
      ++failures;
    }
    const long c0 = T.ipc_closes;
    {
      PeerMap m;
      T.ipc_ranks.clear();
      CHECK(m.open(handles.data(), kStride, kWorld, rank, own.p) == KSIM_OK && m.mapped());
      CHECK((int)m.ptr.size() == kWorld && m.ptr[rank] == own.p && (int)T.ipc.size() == kWorld - 1);
      CHECK((int)T.ipc_ranks.size() == kWorld - 1);
      for (int q = 0; q < kWorld; ++q) CHECK(q == rank || T.ipc.count(m.ptr[q]) == 1);
      PeerMap moved(std::move(m));
      CHECK(!m.mapped() && moved.mapped() && moved.ptr[rank] == own.p && T.ipc_closes == c0);
      {
        PeerMap gone(std::move(moved));  // dies here: closes world - 1, never the own slot
      }
      CHECK(T.ipc_closes == c0 + kWorld - 1 && T.ipc.empty());
    }  // m and moved die moved-from: they close nothing
    CHECK(T.ipc_closes == c0 + kWorld - 1 && T.blocks.count(own.p) == 1);
  }
  own.release();
  CHECK(T.none_live());
  std::printf("peermap: world=%d failures_injected=%ld opens=%ld closes=%ld live=0\n", kWorld, failures, T.ipc_opens,
              T.ipc_closes);
}

// The communicator's owner is a DevHandle over the library's destroyer: one destroy per communicator held, none for null.
static void check_comm_owner() {
  using Comm = DevHandle<fakeComm_t, fake_comm_destroy>;
  const auto fresh = [](int rank) {
    fakeComm_t c = new FakeComm{rank};
    T.comms.insert(c);
    return c;
  };
  {
    Comm none;  // never initialised (an in-process group's shard): nothing to destroy
    CHECK(!none);
  }
  CHECK(T.comm_destroys == 0);
  {
    Comm c;
    c.h = fresh(0);  // as ncclCommInitRank(&comm.h, ...) leaves it
    Comm moved(std::move(c));
    CHECK(!c && moved && T.comms.size() == 1);
    Comm failed;
    failed.h = nullptr;  // a failed init puts the null back
  }
  CHECK(T.comm_destroys == 1 && T.comms.empty());
  {
    Comm a, b;
    a.h = fresh(1);
    b.h = fresh(2);
    a.reset();
    a.reset();  // already null
    CHECK(T.comm_destroys == 2 && T.comms.size() == 1);
  }
  CHECK(T.comm_destroys == 3 && T.none_live());
  std::printf("comm: held=3 destroys=%ld null_destroys=0 live=0\n", T.comm_destroys);
}

int main() {
  check_devbuf();
  check_move();
  check_event_stream_flags_graph();
  check_all_or_nothing();
  check_peer_map();
  check_comm_owner();
  CHECK(T.none_live());
  std::printf("ok\n");
  return 0;
}
