// report_merge_check -- the host merge of the per-event cluster report (csrc/ksim_report_host.hpp) as a stand-alone
// program, built with -fsanitize=address,undefined (tests/test_report_merge_cpu.py).  No GPU, no HIP.
//
//   report_merge_check <cases> <out>
// <cases>: any number of { int32 world, int32 n, world * n ksim_report_part (shard-major: parts[k][i]) }.
// <out>:   per case n * { ksim_report, ksim_power_report }, raw, in the order read.
// Before the cases it checks the record's size and the argument errors of the merge.  Prints "cases=<c> records=<r>",
// then "ok"; any broken expectation prints a line to stderr and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ksim_report_host.hpp"

static void expect(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "report_merge_check: %s\n", what);
  std::exit(1);
}

int main(int argc, char** argv) {
  expect(argc == 3, "usage: report_merge_check <cases> <out>");
  static_assert(sizeof(ksim_report_part) == 208, "ksim_report_part");
  static_assert(sizeof(ksim_report) == 112 && sizeof(ksim_power_report) == 32, "report structs");

  {  // argument errors: nothing is read or written
    ksim_report_part one{};
    const ksim_report_part* ptr[17];
    for (auto& p : ptr) p = &one;
    ksim_report out{};
    ksim_power_report pw{};
    expect(ksim_rep_host::merge(nullptr, 1, 1, &out, &pw) == KSIM_EINVAL, "null parts");
    expect(ksim_rep_host::merge(ptr, 1, 1, nullptr, &pw) == KSIM_EINVAL, "null out");
    expect(ksim_rep_host::merge(ptr, 0, 1, &out, &pw) == KSIM_EINVAL, "world 0");
    expect(ksim_rep_host::merge(ptr, 17, 1, &out, &pw) == KSIM_EINVAL, "world 17");
    expect(ksim_rep_host::merge(ptr, 1, -1, &out, &pw) == KSIM_EINVAL, "n < 0");
    const ksim_report_part* hole[2] = {&one, nullptr};
    expect(ksim_rep_host::merge(hole, 2, 1, &out, &pw) == KSIM_EINVAL, "a null shard");
    expect(ksim_rep_host::merge(ptr, 16, 1, &out, nullptr) == KSIM_OK, "world 16, no power report");
    expect(ksim_rep_host::merge(ptr, 1, 0, &out, &pw) == KSIM_OK, "n = 0");
  }

  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* of = std::fopen(argv[2], "wb");
  expect(in && of, "cannot open the files");
  long cases = 0, records = 0;
  for (;;) {
    int32_t hdr[2];
    const size_t got = std::fread(hdr, sizeof(int32_t), 2, in);
    if (got == 0) break;
    expect(got == 2, "truncated case header");
    const int world = hdr[0], n = hdr[1];
    expect(world >= 1 && world <= 16 && n >= 0 && n <= (1 << 20), "case header out of range");
    std::vector<std::vector<ksim_report_part>> parts(world, std::vector<ksim_report_part>((size_t)n));
    std::vector<const ksim_report_part*> ptr(world);
    for (int k = 0; k < world; ++k) {
      expect(std::fread(parts[k].data(), sizeof(ksim_report_part), (size_t)n, in) == (size_t)n, "truncated case");
      ptr[k] = parts[k].data();
    }
    std::vector<ksim_report> out((size_t)n);
    std::vector<ksim_power_report> pw((size_t)n);
    expect(ksim_rep_host::merge(ptr.data(), world, n, out.data(), pw.data()) == KSIM_OK, "merge failed");
    for (int i = 0; i < n; ++i) {
      expect(std::fwrite(&out[i], sizeof(ksim_report), 1, of) == 1, "write");
      expect(std::fwrite(&pw[i], sizeof(ksim_power_report), 1, of) == 1, "write");
    }
    ++cases;
    records += n;
  }
  std::fclose(in);
  expect(std::fclose(of) == 0, "close");
  std::printf("cases=%ld records=%ld\nok\n", cases, records);
  return 0;
}
