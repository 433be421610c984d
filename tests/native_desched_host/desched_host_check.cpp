// desched_host_check -- the host arithmetic of a descheduling plan (csrc/ksim_desched_host.hpp) as a stand-alone
// program, built with -fsanitize=address,undefined (tests/test_desched_host_cpu.py).  No GPU, no HIP.
//
//   desched_host_check <out> <ratio>...
// <ratio>: hexadecimal floating-point literals (Python's float.hex()), so they arrive exactly.
// <out>:   one line "<ratio index> <n> <budget>" for every ratio and every n in 0..300, for the caller to compare
//          with the reference's formula.
// Before that it checks by itself: the event offsets against a plain prefix sum over ragged streams; the budget at
// ratio = +inf (0 without a bound pod, else every pod); 0 <= budget <= n for n up to INT32_MAX.  Prints
// "offsets=<cases> bounds=<pairs> lines=<l>", then "ok"; any broken expectation prints a line to stderr and exits 1.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ksim_desched_host.hpp"

static void expect(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "desched_host_check: %s\n", what);
  std::exit(1);
}

int main(int argc, char** argv) {
  expect(argc >= 2, "usage: desched_host_check <out> <ratio>...");
  const double inf = std::numeric_limits<double>::infinity();
  const int32_t imax = std::numeric_limits<int32_t>::max();

  const std::vector<std::vector<int>> streams = {
      {}, {0}, {7}, {0, 0, 0}, {0, 256, 257, 700, 1}, {5, 0, 9}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10},
      {imax, imax, 3},  // the offsets are 64-bit: two full streams do not wrap
  };
  for (const auto& n_events : streams) {
    const int R = (int)n_events.size();
    std::vector<long long> eoff = {-1, -1, -1};  // whatever it held is replaced
    const int max_ev = ksim_ds_host::event_offsets(n_events.data(), R, eoff);
    expect(eoff.size() == (size_t)R + 1 && eoff[0] == 0, "offsets: R + 1 entries from 0");
    long long sum = 0;
    int longest = 0;
    for (int r = 0; r < R; ++r) {
      expect(eoff[r] == sum, "offsets: the prefix sum");
      sum += n_events[r];
      if (n_events[r] > longest) longest = n_events[r];
    }
    expect(eoff[R] == sum, "offsets: the total");
    expect(max_ev == longest, "offsets: the largest stream");
  }

  // ratio = +inf: the reference's formula raises there, so these values are the contract
  expect(ksim_ds_host::budget(inf, 0) == 0, "inf, no bound pod");
  for (int32_t n = 1; n <= 300; ++n) expect(ksim_ds_host::budget(inf, n) == n, "inf, n bound pods");
  expect(ksim_ds_host::budget(inf, imax) == imax, "inf, INT32_MAX bound pods");

  long pairs = 0;
  std::vector<int32_t> ns = {0, 1, 2, 3, 299, 300, imax - 1, imax};
  for (int k = 2; k < 31; ++k)
    for (int d = -1; d <= 1; ++d) ns.push_back((int32_t)((1ll << k) + d));
  const double ratios[] = {0.0, 1e-300, 1e-9, 0.05, 0.3, 0.5, 1.0 - 1e-16, 1.0, 1.0 + 1e-12, 7.0, 1e300, inf};
  for (const int32_t n : ns)
    for (const double q : ratios) {
      const int32_t b = ksim_ds_host::budget(q, n);
      expect(b >= 0 && b <= n, "0 <= budget <= n");
      expect(q < 1.0 || b == n, "ratio >= 1 takes every pod");
      expect(q > 0.0 || b == 0, "ratio 0 takes none");
      expect(!(q > 0.0 && n > 0) || b >= 1, "a positive ratio of some pods takes one at least");
      ++pairs;
    }

  std::FILE* of = std::fopen(argv[1], "w");
  expect(of != nullptr, "cannot open the output file");
  long lines = 0;
  for (int i = 2; i < argc; ++i) {
    char* end = nullptr;
    const double q = std::strtod(argv[i], &end);
    expect(end != argv[i] && *end == '\0' && q >= 0.0, "a ratio does not parse");
    for (int32_t n = 0; n <= 300; ++n, ++lines) std::fprintf(of, "%d %d %d\n", i - 2, (int)n, (int)ksim_ds_host::budget(q, n));
  }
  expect(std::fclose(of) == 0, "cannot write the output file");
  std::printf("offsets=%zu bounds=%ld lines=%ld\nok\n", streams.size(), pairs, lines);
  return 0;
}
