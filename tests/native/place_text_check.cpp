// The two texts of swg_paf_place (sweepga_amd/csrc/host/place_text.cpp) without a GPU and without the library: a stand-alone
// program over rows at the ends of every field's range -- signed starts down to INT64_MIN, lengths of 2^32 - 1, counts of 2^64 - 1,
// no rows at all -- meant to be built with the host sanitizers.  The names come from a table of its own (the handle is never
// looked at).  Prints one JSON line; exit status 1 on a difference.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

static const char* const NAMES[3] = {"a#1#x", "b#1#y", ""};
extern "C" const char* swg_paf_sequence_name(const swg_paf*, uint32_t id) { return NAMES[id]; }
int swg_alnstats_error(int code, const char*, ...) { return code; }  // (texts_hand_over names it; nothing here calls it)

static int failures = 0;
static void expect(const std::string& got, const std::string& want, const char* what) {
  if (got == want) return;
  ++failures;
  std::fprintf(stderr, "%s:\n got  %s\n want %s\n", what, got.c_str(), want.c_str());
}

int main() {
  const std::string rows_header =
      "#sequence\tlength\tpartner\tpartner_length\torient\tstart\tend\trank\tbases\tfwd\trev\ttotal\trunner\trecords\tq_lo\tq_hi\tt_lo\tt_hi\n";
  const std::string summary_header = "#genome\tpartner_genome\tsequences\treversed\tlength\tbases\ttotal_bases\n";
  const uint32_t TOP = 0xffffffffu;
  const std::vector<uint32_t> seq_len = {1000, TOP, 0};
  expect(swg_place_rows_text(nullptr, seq_len, {}), rows_header, "no rows");
  expect(swg_place_summary_text({}, {}), summary_header, "no pairs");
  std::vector<swg_placement> rows(3);
  rows[0] = swg_placement{0, 1, 0, 1, 250, -750, 100, 0, 100, 100, 0, 1, 100, 200, 50, 150, 0, 1, {0, 0, 0}};
  rows[1] = swg_placement{1, 0, 1, 0, 2ll * TOP, (long long)TOP, UINT64_MAX, UINT64_MAX, 0, UINT64_MAX, UINT64_MAX, UINT64_MAX, 0, TOP, 0, TOP, TOP, 0, {0, 0, 0}};
  rows[2] = swg_placement{2, 2, 0, 0, INT64_MIN, INT64_MIN, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};
  const std::string u64 = "18446744073709551615";
  expect(swg_place_rows_text(nullptr, seq_len, rows),
         rows_header + "a#1#x\t1000\tb#1#y\t4294967295\t-\t-750\t250\t0\t100\t0\t100\t100\t0\t1\t100\t200\t50\t150\n" +
             "b#1#y\t4294967295\ta#1#x\t1000\t+\t4294967295\t8589934590\t4294967295\t" + u64 + "\t" + u64 + "\t0\t" + u64 + "\t" + u64 + "\t" + u64 +
             "\t0\t4294967295\t0\t4294967295\n" + "\t0\t\t0\t+\t-9223372036854775808\t-9223372036854775808\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n",
         "rows");
  const std::vector<swg_place_pair> pairs = {{0, 1, 3, 1, 3000, 300, 300}, {1, 0, UINT64_MAX, 0, UINT64_MAX, 0, UINT64_MAX}};
  expect(swg_place_summary_text({"a#1#", "b#1#"}, pairs),
         summary_header + "a#1#\tb#1#\t3\t1\t3000\t300\t300\n" + "b#1#\ta#1#\t" + u64 + "\t0\t" + u64 + "\t0\t" + u64 + "\n", "summary");
  std::printf("{\"ok\": %s, \"failures\": %d}\n", failures ? "false" : "true", failures);
  return failures ? 1 : 0;
}
