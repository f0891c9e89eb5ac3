// The line writer and the batch planner of the slice PAF (sweepga_amd/csrc/host/slice_text.cpp) without a GPU and without the
// library: a stand-alone program meant to be built with the host sanitizers, together with slice_text.cpp.  Standard input, case by
// case:
//   L <newline> ten numbers: q_start q_end t_start t_end flags aligned matches block record text_len <newline> query name <newline>
//     target name <newline> label <newline> the slice's CIGAR followed by foreign bytes <newline> the record's own line
//                                     ->  the slice's line.  The record's line and the CIGAR are copied into heap blocks of exactly
//     their size first, so that a read past either end is the address sanitizer's to find.
//   P <newline> batch_bytes m cost_0 .. cost_{m-1}   ->  the batches' first regions and m, space-separated, one line
// tests/test_lift_paf_cpu.py feeds it and compares the bytes with tests/lift_paf_model.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

// what the PAF seams of slice_text.cpp link against; nothing here calls them
int swg_alnstats_error(int code, const char*, ...) { return code; }
extern "C" {
const char* swg_last_error(const swg_ctx*) { std::abort(); }
const swg_records* swg_paf_records(const swg_paf*) { std::abort(); }
const uint64_t* swg_paf_seq_offsets(const swg_paf*) { std::abort(); }
const uint64_t* swg_paf_record_offsets(const swg_paf*, int) { std::abort(); }
const char* swg_paf_sequence_name(const swg_paf*, uint32_t) { std::abort(); }
}
void swg_paf_lines_view(const swg_paf*, const char**, const uint64_t**, const uint32_t**) { std::abort(); }
int swg_lift_bed_parse(const char*, const swg_paf*, const char*, uint64_t, std::vector<swg_lift_region>*, std::vector<std::string>*) { std::abort(); }
int swg_lift_run(swg_ctx*, const swg_records*, bool, const uint8_t*, const swg_lift_region*, uint64_t, swg_lift_request*) { std::abort(); }
int swg_lift_hit_run(swg_ctx*, const swg_records*, bool, const uint8_t*, const swg_lift_region*, uint64_t, uint32_t, uint32_t, uint32_t*, uint64_t,
                     uint64_t*) {
  std::abort();
}
int swg_lift_slice_run(swg_ctx*, const swg_records*, bool, const uint8_t*, const swg_lift_region*, uint64_t, const swg_cigar_set*, swg_lift_slice_request*) {
  std::abort();
}
const char* swg_cigar_tag_find(const char*, uint64_t, uint64_t*) { std::abort(); }
uint64_t swg_ucsc_default_batch(swg_ctx*) { std::abort(); }

static char* heap_copy(const std::string& s) {
  char* b = static_cast<char*>(std::malloc(s.size() ? s.size() : 1));
  if (!b) std::exit(3);
  std::memcpy(b, s.data(), s.size());
  return b;
}

int main() {
  std::string kind, line;
  while (std::getline(std::cin, kind)) {
    if (kind == "L") {
      std::string q_name, t_name, label, cigar, own;
      if (!std::getline(std::cin, line) || !std::getline(std::cin, q_name) || !std::getline(std::cin, t_name) || !std::getline(std::cin, label) ||
          !std::getline(std::cin, cigar) || !std::getline(std::cin, own))
        return 2;
      std::istringstream in(line);
      uint64_t v[10];
      for (uint64_t& x : v)
        if (!(in >> x)) return 2;
      swg_lift_slice s{};
      s.q_start = (uint32_t)v[0], s.q_end = (uint32_t)v[1], s.t_start = (uint32_t)v[2], s.t_end = (uint32_t)v[3], s.flags = (uint32_t)v[4];
      s.aligned = (uint32_t)v[5], s.matches = (uint32_t)v[6], s.block = v[7], s.record = (uint32_t)v[8], s.text_len = (uint32_t)v[9];
      if (s.text_len > cigar.size()) return 2;
      char* cg = heap_copy(cigar.substr(0, s.text_len));
      char* rec_line = heap_copy(own);
      std::string o;
      swg_slice_line_text(o, q_name.c_str(), t_name.c_str(), rec_line, own.size(), s, cg, label);
      std::free(rec_line);
      std::free(cg);
      std::fwrite(o.data(), 1, o.size(), stdout);
    } else if (kind == "P") {
      if (!std::getline(std::cin, line)) return 2;
      std::istringstream in(line);
      uint64_t batch, m;
      if (!(in >> batch >> m)) return 2;
      uint64_t* cost = static_cast<uint64_t*>(std::malloc(m ? m * sizeof(uint64_t) : 1));
      if (!cost) return 3;
      for (uint64_t r = 0; r < m; ++r)
        if (!(in >> cost[r])) return 2;
      std::vector<uint64_t> first;
      swg_slice_plan_batches(cost, m, batch, &first);
      std::free(cost);
      for (size_t b = 0; b < first.size(); ++b) std::printf(b ? " %llu" : "%llu", (unsigned long long)first[b]);
      std::fputc('\n', stdout);
    } else {
      return 2;
    }
  }
  return 0;
}
