// The tag finder and the row formatter of swg_paf_lift_exact (sweepga_amd/csrc/host/cigar_text.cpp) without a GPU and without the
// library: a stand-alone program meant to be built with the host sanitizers.  Standard input, case by case:
//   T <newline> one PAF line        ->  `1 <tab> value` or `0`; the line is copied into a heap block of exactly its length first, so
//                                        that a read past either end is the address sanitizer's to find
//   R <newline> ten numbers (the fields of swg_lift_exact_row in order) <newline> label <newline> source name
//                                    ->  the row's line, with the destination name from a table of this program's own
// tests/test_lift_exact_cpu.py feeds it and compares the bytes with tests/lift_exact_model.py.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

static const char* const NAMES[3] = {"a#1#x", "", "c#2#z"};
int swg_alnstats_error(int code, const char*, ...) { return code; }  // (texts_hand_over names it; nothing here calls it)

int main() {
  std::string kind, line;
  while (std::getline(std::cin, kind)) {
    if (kind == "T") {
      if (!std::getline(std::cin, line)) return 2;
      char* block = static_cast<char*>(std::malloc(line.size() ? line.size() : 1));
      if (!block) return 3;
      std::memcpy(block, line.data(), line.size());
      uint64_t len = 99;
      const char* v = swg_cigar_tag_find(block, line.size(), &len);
      if (v) {
        std::fputs("1\t", stdout);
        std::fwrite(v, 1, len, stdout);
        std::fputc('\n', stdout);
      } else {
        if (len != 0) return 4;
        std::fputs("0\n", stdout);
      }
      std::free(block);
    } else if (kind == "R") {
      std::string label, name;
      if (!std::getline(std::cin, line) || !std::getline(std::cin, label) || !std::getline(std::cin, name)) return 2;
      std::istringstream in(line);
      uint32_t v[10];
      for (uint32_t& x : v)
        if (!(in >> x)) return 2;
      const swg_lift_exact_row w{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]};
      std::string o;
      swg_lift_exact_row_text(o, NAMES[w.dst_seq], label, name, w);
      std::fwrite(o.data(), 1, o.size(), stdout);
    } else {
      return 2;
    }
  }
  return 0;
}
