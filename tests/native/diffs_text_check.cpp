// The row formatter, the merge of pair sums and the summary text of the difference list (sweepga_amd/csrc/host/diffs_text.cpp) without a
// GPU and without the library: a stand-alone program meant to be built with the host sanitizers, together with diffs_text.cpp,
// ucsc_text.cpp and cigar_text.cpp.  Standard input, case by case:
//   R <newline> eight numbers: record kind_flags t_start t_end q_start q_end left right <newline> target name <newline> query name
//                                       ->  the header line and the row's line
//   M <newline> a b <newline> a + b lines `q_genome t_genome` and twelve sums   ->  the first a pairs merged into nothing, then the other
//     b merged into that: one line per pair.  Both lists are copied into heap blocks of exactly their size first, so that a read past
//     either end is the address sanitizer's to find.
//   Y <newline> G P S <newline> G genome names, P pair lines, S lines `index count` of the spectrum   ->  the summary text
// tests/test_diffs_cpu.py feeds it and compares the bytes with tests/diffs_model.py.
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

// what the PAF seams of diffs_text.cpp and ucsc_text.cpp link against; nothing here calls them
int swg_alnstats_error(int code, const char*, ...) { return code; }
extern "C" {
const char* swg_last_error(const swg_ctx*) { std::abort(); }
const swg_records* swg_paf_records(const swg_paf*) { std::abort(); }
const uint64_t* swg_paf_seq_offsets(const swg_paf*) { std::abort(); }
const uint64_t* swg_paf_record_offsets(const swg_paf*, int) { std::abort(); }
const char* swg_paf_sequence_name(const swg_paf*, uint32_t) { std::abort(); }
const char* swg_paf_genome_two_prefix(const swg_paf*, uint32_t) { std::abort(); }
}
int swg_paf_seq_last_lengths(const swg_paf*, std::vector<uint32_t>*) { std::abort(); }
void swg_paf_lines_view(const swg_paf*, const char**, const uint64_t**, const uint32_t**) { std::abort(); }
int swg_ucsc_run(swg_ctx*, const swg_records*, bool, const uint32_t*, const uint8_t*, const swg_cigar_set*, swg_ucsc_request*) { std::abort(); }
int swg_diff_run(swg_ctx*, const swg_records*, bool, const uint32_t*, uint32_t, const uint8_t*, const swg_cigar_set*, swg_diff_request*) { std::abort(); }
uint64_t swg_ucsc_default_batch(swg_ctx*) { std::abort(); }

static bool read_pair(swg_diff_pair* g) {
  std::string line;
  if (!std::getline(std::cin, line)) return false;
  std::istringstream in(line);
  unsigned long long a, b, v;
  if (!(in >> a >> b)) return false;
  g->q_genome = (uint32_t)a, g->t_genome = (uint32_t)b;
  uint64_t* d = &g->entries;
  for (int f = 0; f < 12; ++f) {
    if (!(in >> v)) return false;
    d[f] = v;
  }
  return true;
}

static void print_pairs(const std::vector<swg_diff_pair>& pairs) {
  for (const swg_diff_pair& g : pairs) {
    std::printf("%u %u", g.q_genome, g.t_genome);
    const uint64_t* v = &g.entries;
    for (int f = 0; f < 12; ++f) std::printf(" %llu", (unsigned long long)v[f]);
    std::fputc('\n', stdout);
  }
}

int main() {
  std::string kind, line;
  while (std::getline(std::cin, kind)) {
    if (kind == "R") {
      std::string t_name, q_name;
      if (!std::getline(std::cin, line) || !std::getline(std::cin, t_name) || !std::getline(std::cin, q_name)) return 2;
      std::istringstream in(line);
      uint64_t v[8];
      for (uint64_t& x : v)
        if (!(in >> x)) return 2;
      swg_diff_row w;
      w.record = (uint32_t)v[0], w.kind_flags = (uint32_t)v[1], w.t_start = (uint32_t)v[2], w.t_end = (uint32_t)v[3];
      w.q_start = (uint32_t)v[4], w.q_end = (uint32_t)v[5], w.left = (uint32_t)v[6], w.right = (uint32_t)v[7];
      std::string o;
      swg_diffs_rows_header(o);
      swg_diffs_row_text(o, t_name.c_str(), q_name.c_str(), w);
      std::fwrite(o.data(), 1, o.size(), stdout);
    } else if (kind == "M") {
      if (!std::getline(std::cin, line)) return 2;
      std::istringstream in(line);
      uint64_t n[2];
      if (!(in >> n[0] >> n[1])) return 2;
      std::vector<swg_diff_pair> total;
      for (int part = 0; part < 2; ++part) {
        swg_diff_pair* add = static_cast<swg_diff_pair*>(std::malloc(n[part] ? n[part] * sizeof(swg_diff_pair) : 1));
        if (!add) return 3;
        for (uint64_t j = 0; j < n[part]; ++j)
          if (!read_pair(&add[j])) return 2;
        swg_diffs_merge_pairs(&total, add, n[part]);
        std::free(add);
      }
      print_pairs(total);
      std::puts("--");
    } else if (kind == "Y") {
      if (!std::getline(std::cin, line)) return 2;
      std::istringstream in(line);
      uint64_t G, P, S;
      if (!(in >> G >> P >> S)) return 2;
      std::vector<std::string> names(G);
      for (std::string& nm : names)
        if (!std::getline(std::cin, nm)) return 2;
      std::vector<swg_diff_pair> pairs(P);
      for (swg_diff_pair& g : pairs)
        if (!read_pair(&g)) return 2;
      uint64_t* spectrum = static_cast<uint64_t*>(std::calloc(4 * SWG_DIFF_BINS, sizeof(uint64_t)));
      if (!spectrum) return 3;
      for (uint64_t s = 0; s < S; ++s) {
        unsigned long long at, count;
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream sp(line);
        if (!(sp >> at >> count) || at >= 4 * SWG_DIFF_BINS) return 2;
        spectrum[at] = count;
      }
      const std::string o = swg_diffs_summary_text(names, pairs, spectrum);
      std::free(spectrum);
      std::fwrite(o.data(), 1, o.size(), stdout);
    } else {
      return 2;
    }
  }
  return 0;
}
