// The two texts of swg_paf_windows (sweepga_amd/csrc/host/windows_text.cpp) without a GPU and without the library: a stand-alone
// program meant to be built with the host sanitizers.  It reads rows and summary entries as decimal numbers from standard input
// (`R` + 12 numbers = one swg_window_row, `S` + 12 numbers = one swg_window_seq, in the structures' field order) and prints text 0,
// then a line `--`, then text 1: tests/test_windows_cpu.py feeds it what tests/windows_model.py computed and compares the bytes
// with the model's formatter.  The names and lengths come from a table of its own (the handle is never looked at).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

static const char* const NAMES[4] = {"a#1#x", "b#1#y", "", "c#2#z"};
extern "C" const char* swg_paf_sequence_name(const swg_paf*, uint32_t id) { return NAMES[id]; }
int swg_alnstats_error(int code, const char*, ...) { return code; }  // (texts_hand_over names it; nothing here calls it)

int main() {
  const std::vector<uint32_t> seq_len = {1000, 0xffffffffu, 0, 77};
  std::vector<swg_window_row> rows;
  std::vector<swg_window_seq> seqs;
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    uint64_t v[12];
    for (uint64_t& x : v)
      if (std::scanf("%" SCNu64, &x) != 1) return 2;
    if (kind == 'R')
      rows.push_back(swg_window_row{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], {(uint32_t)v[4], (uint32_t)v[5]},
                                    {(uint32_t)v[6], (uint32_t)v[7]}, {v[8], v[9]}, {v[10], v[11]}});
    else if (kind == 'S')
      seqs.push_back(swg_window_seq{(uint32_t)v[0], (uint32_t)v[1], {(uint32_t)v[2], (uint32_t)v[3]}, {v[4], v[5]}, {v[6], v[7]}, {v[8], v[9]}, {v[10], v[11]}});
    else
      return 2;
  }
  const std::string a = swg_windows_rows_text(nullptr, rows), b = swg_windows_summary_text(nullptr, seq_len, seqs);
  std::fwrite(a.data(), 1, a.size(), stdout);
  std::fputs("--\n", stdout);
  std::fwrite(b.data(), 1, b.size(), stdout);
  return 0;
}
